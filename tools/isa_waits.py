#!/usr/bin/env python3
"""Memory-op / wait skeleton of one kernel's ISA, in program order (no GPU needed):
     python tools/isa_waits.py spark-tts_amd/csrc/smi_llm.hip 'k_gemm<1, 1, 8, 2, 2, 1, 1, 0, 1, 6, 2>' [first_line [last_line]]
   Prints every global/flat/scratch load and store, s_load, s_waitcnt, LDS write, barrier, branch, branch label and MFMA with
   its line number inside the kernel, plus the kernel-argument preload length (dwords of leading scalar parameters that are in
   SGPRs at wave start: the hot entries, k_gemm_hot / k_down1_hot / k_attn_hot; lines 2 .. 8 of
   such a kernel are the compatibility block for firmware without preload) and ScratchSize / VGPRs / code length.
   What to look for (profiles/README.md):
   a `s_waitcnt vmcnt(0)` right behind a load inside a loop (one memory round trip per trip), `scratch_` / `flat_load`
   (an array or a `cond ? *p : 0` the compiler could not keep in registers), waits that sit in front of the MFMAs but
   belong to loads only the epilogue needs (vmcnt counts in order: every wait also covers everything issued before it);
   in a hot entry, a `s_waitcnt lgkmcnt` on the work path (follow the first s_cbranch: the helper blocks' path comes first in
   the text) in front of the first weight / K / V / partial global_load -- a kernel-argument round trip at entry.

   A source that ends in .s is read as the assembly itself (hipcc -S --cuda-device-only with the Makefile's flags): one
   compilation for many kernels.

   --entry (a hot entry) counts the work path instead: from the first instruction behind the compatibility block, the first
   s_cbranch taken (the helper test), every later conditional branch not taken, s_branch followed, up to the first
   `s_waitcnt vmcnt`:
     python tools/isa_waits.py --entry build.s 'k_down1_hot<10>'
   -> instructions to the first load, to the last load in front of that wait, the VALU (64-bit ones apart) and SALU
   instructions and the `s_waitcnt lgkmcnt` in front of that last load.  profiles/entry_loads_vs_parent.txt has the table;
   tests/test_entry_waits_cpu.py pins the waits (not the counts: those are the compiler's) on the built library."""
import re, subprocess, sys, tempfile, os

LOAD = re.compile(r"^(global_load|flat_load|buffer_load|scratch_load)")
WIDE = re.compile(r"_[uib]64|v_mad_u64_u32|v_mad_i64_i32|v_lshl_add_u64")


def work_path(ins, labels):
    """ins: the kernel's instructions in text order; labels: {label: index of the instruction behind it}.  -> the indices on the
    work path from the first instruction behind the compatibility block (its closing s_branch is followed) up to and including the
    first `s_waitcnt vmcnt`"""
    i, first, path, seen, begun = 0, True, [], set(), False
    while i < len(ins) and i not in seen:
        seen.add(i)
        t = ins[i]
        m = re.match(r"^(s_branch|s_cbranch_\w+)\s+(\S+)", t)
        if begun:
            path.append(i)
        if m and m.group(1) == "s_branch":
            if m.group(2) not in labels:
                break
            i, begun = labels[m.group(2)], True      # (the first s_branch closes the compatibility block)
            continue
        if m and first and begun:
            first = False
            if m.group(2) not in labels:
                break
            i = labels[m.group(2)]
            continue
        if begun and t.startswith("s_waitcnt") and "vmcnt" in t:
            break
        if t.startswith("s_endpgm"):
            break
        i += 1
    return path


def entry_counts(ins, labels):
    path = work_path(ins, labels)
    loads = [k for k, i in enumerate(path) if LOAD.match(ins[i])]
    if not loads:
        return None
    upto = path[: loads[-1] + 1]
    return {"first_load": loads[0] + 1, "last_load": loads[-1] + 1, "loads": len(loads),
            "valu": sum(ins[i].startswith("v_") for i in upto), "valu64": sum(bool(ins[i].startswith("v_") and WIDE.search(ins[i])) for i in upto),
            "salu": sum(bool(re.match(r"^s_(?!load|waitcnt|cbranch|branch|nop|buffer_load)", ins[i])) for i in upto),
            "scalar_waits": [k + 1 for k, i in enumerate(upto) if ins[i].startswith("s_waitcnt") and "lgkmcnt" in ins[i]],
            "to_vmcnt": len(path)}


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--entry"]
    entry = "--entry" in sys.argv[1:]
    src, want = args[0], args[1]
    lo = int(args[2]) if len(args) > 2 else 0
    hi = int(args[3]) if len(args) > 3 else 10 ** 9
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if src.endswith(".s"):
        lines = open(src).read().split("\n")
    else:
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, "k.s")
            subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{root}/include",
                            f"-I{root}/spark-tts_amd/csrc", "-ffp-contract=off", "-mllvm", "-amdgpu-kernarg-preload-count=16",   # as csrc/Makefile
                            "-S", "--cuda-device-only", "-o", out, src],
                           check=True, stderr=subprocess.DEVNULL)
            lines = open(out).read().split("\n")
    names = {}
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            names[i] = m.group(1)
    dem = subprocess.run(["c++filt"] + list(names.values()), capture_output=True, text=True).stdout.split("\n")
    norm = lambda s: s.replace("(anonymous namespace)::", "").replace(" ", "")
    start = next((i for (i, _), dn in zip(names.items(), dem) if norm(want) in norm(dn)), None)
    if start is None:
        sys.exit("kernel not found; candidates:\n" + "\n".join(sorted(set(norm(x).split("(")[0] for x in dem if "k_" in x))))
    pat = re.compile(r"global_|flat_|scratch_|s_load|s_waitcnt|ds_write|s_barrier|mfma|^\.LBB|s_endpgm|s_cbranch|s_branch")
    n = 0
    ins, labels = [], {}
    for l in lines[start + 1:]:
        n += 1
        if re.match(r"^_Z\w+:", l):
            break
        t = l.strip()
        m = re.match(r"^(\.LBB\w+):", t)
        if m:
            labels[m.group(1)] = len(ins)
        elif t and not t.startswith((";", ".")) and not re.search(r"; (ScratchSize|NumVgprs|NumAgprs|codeLenInByte|Occupancy)\b", t):
            ins.append(t.split(";")[0].strip())
        if not entry and lo <= n <= hi and pat.search(t) and not t.startswith(";"):
            print(f"{n:5d}  {t.split(';')[0].strip()[:100]}")
        m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", t)
        if m:
            print("       ; kernarg preload length:", m.group(1), "dwords")
        m = re.search(r"; (ScratchSize|NumVgprs|NumAgprs|codeLenInByte|Occupancy)\b.*", t)
        if m:
            print("      ", m.group(0))
            if "Occupancy" in m.group(0):
                break
    if entry:
        c = entry_counts(ins, labels)
        if c is None:
            sys.exit("no load on the work path in front of the first s_waitcnt vmcnt")
        print(f"       work path: first load at instruction {c['first_load']}, last of {c['loads']} loads in front of the first s_waitcnt vmcnt at "
              f"{c['last_load']} (the wait: {c['to_vmcnt']}); up to that load {c['valu']} VALU ({c['valu64']} 64-bit), {c['salu']} SALU; "
              f"s_waitcnt lgkmcnt at {c['scalar_waits'] or 'none'}")
