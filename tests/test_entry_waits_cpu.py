"""A one-row decode kernel's first loads -- the operand staging load, the RMSNorm partials and the weight tiles of the QKV kernel, q /
K / V of the attention kernel, the per-head partials and weight tiles of gate_up, the weight and operand pieces of down_proj --
are addressed from preloaded kernel arguments only, so nothing has to come back from the kernel-argument segment before they are
requested.  A struct field read too early (or an SGPR pair the compiler reuses while a kernel-argument load still writes it)
would put a `s_waitcnt lgkmcnt` in front of them: the results would be the same, the launch a scalar round trip (~0.25 us) slower.
So the wait structure of the BUILT library is read here, for every hot entry:

  the work path    from the first instruction behind the compatibility block that firmware without preload runs; the first
                   conditional branch (the helper-block test) taken, every later one not taken, unconditional branches followed,
                   up to the first `s_waitcnt vmcnt` (the walk must END there: a walk that runs into the end of the program or
                   into an instruction it has already seen fails the test)
  the pin          no `s_waitcnt lgkmcnt` on the work path in front of the LAST load issued before that wait
  one exemption    gate_up (the PRO_FUSEDO forms of k_gemm_hot) touches the next layer's QKV weights from its last wave, right
                   behind its own weight loads: ONE `global_load_dword` behind the last non-temporal (weight) load, which nothing
                   reads until the MFMA loop is over.  Its address needs two struct lines, so two waits stand in front of it --
                   behind all partial and weight requests.  For those entries the pin holds up to the last load in front of the touch.

(The fused attention kernel's o_proj waves branch off that path: their weight loads have a block of their own.)  The one-row QKV
also requests its row descriptor by an `s_load_dwordx2` written in inline asm and waits for it in a second asm statement; the
compiler does not know that the destination pair is pending in between, so no instruction between the two may name it.  Scratch
memory stays unused.  Only the waits are pinned: instruction counts are the compiler's (tools/isa_waits.py --entry prints them,
profiles/entry_loads_vs_parent.txt records them).
No GPU and no compilation: the gfx950 code objects are taken out of libsparkmi.so and disassembled."""
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "spark-tts_amd", "sparkmi", "libsparkmi.so")
OBJDUMP = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")) if p and os.path.exists(p)), None)

HOT = ("k_gemm_hot", "k_down1_hot", "k_attn_hot")   # QKV and gate_up, down_proj, fused attention
QKV = "k_gemm_hotILi1ELi1ELi16ELi2ELi1ELi1ELi2E"    # <MT 1, NTB 1, NW 16, U 2, WB 1, PRO_NORM, EPI_QKV, ..>
GATE_UP = "k_gemm_hotILi1ELi1ELi8ELi2ELi2ELi2ELi1E"  # <1, 1, 8, 2, 2, PRO_FUSEDO, EPI_SWIGLU, ..>: the entries with the exempt touch load
LOAD = re.compile(r"^(global_load|flat_load|buffer_load|scratch_load)")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: (instructions [(offset, text, branch target offset or None)], scratch bytes)} of every hot entry"""
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    if OBJDUMP is None:
        pytest.skip("llvm-objdump of the ROCm tree not found")
    d = tmp_path_factory.mktemp("co")
    lib = shutil.copy(LIB, d)                                   # the bundles are written beside the file they come from
    subprocess.run([OBJDUMP, "--offloading", lib], check=True, capture_output=True, timeout=120)
    out = {}
    for co in glob.glob(os.path.join(d, "*gfx950*")):
        desc = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", co], check=True, capture_output=True, text=True, timeout=120).stdout
        scratch = {m.group(1): int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2)).group(1))
                   for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", desc, re.S)}
        if not any(h in k for k in scratch for h in HOT):
            continue
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True, timeout=300).stdout
        name, start = None, 0
        for line in txt.split("\n"):
            m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
            if m:
                name, start = m.group(2), int(m.group(1), 16)
                if any(h in name for h in HOT):
                    out[name] = ([], scratch[name])
                continue
            m = re.match(r"^\s+(\S.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
            if m and name in out:
                t = re.search(r"<[^>+]+(?:\+0x([0-9a-f]+))?>\s*$", m.group(3))
                target = (int(t.group(1), 16) if t.group(1) else 0) if t and m.group(1).startswith(("s_branch", "s_cbranch")) else None
                out[name][0].append((int(m.group(2), 16) - start, m.group(1), target))
    assert out, "no hot entry found in the library: the extraction or the disassembly's format has changed"
    return out


def work_path(ins):
    """instruction texts from the first one behind the compatibility block up to and including the first `s_waitcnt vmcnt`"""
    at = {off: i for i, (off, _, _) in enumerate(ins)}
    i, begun, first, path, seen = 0, False, True, [], set()
    while True:
        assert i < len(ins) and i not in seen, "the walk left the program or came back to an instruction before any s_waitcnt vmcnt"
        seen.add(i)
        _, t, target = ins[i]
        if begun:
            path.append(t)
        assert not t.startswith("s_endpgm"), "the work path ends without a s_waitcnt vmcnt"
        if t.startswith("s_branch"):
            assert target in at, t
            i, begun = at[target], True          # the first s_branch closes the compatibility block
            continue
        if t.startswith("s_cbranch") and begun and first:
            assert target in at, t
            i, first = at[target], False         # the helper-block test: the work path is the taken side
            continue
        if begun and t.startswith("s_waitcnt") and "vmcnt" in t:
            return path
        i += 1


def pinned_loads(name, path):
    """indices in `path` of the loads the pin covers: all of them, minus gate_up's one touch load"""
    loads = [i for i, t in enumerate(path) if LOAD.match(t)]
    if GATE_UP in name:
        nt = [i for i in loads if re.search(r"\bnt\b", path[i])]
        assert len(nt) == 4, f"{name}: {len(nt)} non-temporal weight loads in front of the first s_waitcnt vmcnt, 4 expected"
        behind = [i for i in loads if i > nt[-1]]
        assert len(behind) <= 1 and all(path[i].startswith("global_load_dword ") for i in behind), \
            f"{name}: the exemption is ONE global_load_dword behind the weight loads, found {[path[i] for i in behind]}"
        loads = [i for i in loads if i <= nt[-1]]
    return loads


def sregs(text):
    regs = set()
    for a, b in re.findall(r"\bs\[(\d+):(\d+)\]", text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r"\bs(\d+)\b", text))
    return regs


@pytest.mark.parametrize("frag", HOT)
def test_no_scalar_wait_in_front_of_the_first_loads(kernels, frag):
    sel = {k: v for k, v in kernels.items() if frag in k}
    assert sel, f"no {frag} kernel in the library"
    for name, (ins, _) in sel.items():
        assert ins[0][1].startswith("s_load") and any(t.startswith("s_branch") for _, t, _ in ins[:8]), \
            f"{name}: no compatibility block at entry -- is the kernel still built with kernel-argument preload?"
        path = work_path(ins)
        loads = pinned_loads(name, path)
        assert loads, f"{name}: no load in front of the first s_waitcnt vmcnt on the work path"
        waits = [(i + 1, t) for i, t in enumerate(path[: loads[-1]]) if t.startswith("s_waitcnt") and "lgkmcnt" in t]
        assert not waits, (f"{name}: s_waitcnt lgkmcnt on the work path in front of the last of the {len(loads)} loads issued before the "
                           f"first s_waitcnt vmcnt (instruction {loads[-1] + 1}; the wait is instruction {len(path)}): {waits}")
        assert not any(t.startswith(("scratch_", "flat_load")) for t in path), f"{name}: scratch / flat access at entry"


def test_qkv_requests_operand_partials_and_weights_in_front_of_its_first_wait(kernels):
    """the sanity check of the pin itself: it covers the staging load, the four partials and the two weight tiles"""
    sel = {k: v for k, v in kernels.items() if QKV in k}
    assert len(sel) == 2, sorted(sel)   # bf16 and f32 cache
    for name, (ins, _) in sel.items():
        path = work_path(ins)
        loads = [path[i] for i in pinned_loads(name, path)]
        assert len(loads) == 7 and sum(t.startswith("global_load_dwordx4") for t in loads) == 3 and \
            sum(bool(re.search(r"\bnt\b", t)) for t in loads) == 2 and sum(t.startswith("global_load_dword ") for t in loads) == 4, (name, loads)


def test_qkv_row_descriptor_pair_is_not_named_between_its_load_and_its_wait(kernels):
    sel = {k: v for k, v in kernels.items() if QKV in k}
    assert len(sel) == 2, sorted(sel)
    for name, (ins, _) in sel.items():
        texts = [t for _, t, _ in ins]
        begin = next(i for i, t in enumerate(texts) if t.startswith("s_branch")) + 1      # behind the compatibility block
        cand = [i for i in range(begin, len(texts))
                if re.match(r"^s_load_dwordx2 s\[\d+:\d+\], s\[\d+:\d+\], 0x0$", texts[i]) and "s[0:1], 0x0" not in texts[i]]
        assert len(cand) == 1, f"{name}: one s_load_dwordx2 of the row descriptor expected behind the entry, found {[texts[i] for i in cand]}"
        dst = sregs(texts[cand[0]].split(",")[0])
        end = next((i for i in range(cand[0] + 1, len(texts)) if texts[i].startswith("s_waitcnt") and "lgkmcnt(0)" in texts[i]), None)
        assert end is not None, f"{name}: no s_waitcnt lgkmcnt(0) behind the descriptor's load"
        named = [(i - cand[0], texts[i]) for i in range(cand[0] + 1, end) if sregs(texts[i]) & dst]
        assert not named, f"{name}: s{sorted(dst)} is named between the descriptor's load and its wait (stale bits): {named}"
        assert sregs(texts[end + 1]) & dst, f"{name}: the instruction behind the wait does not read the descriptor: {texts[end + 1]}"


@pytest.mark.parametrize("frag", HOT)
def test_hot_entries_use_no_scratch(kernels, frag):
    sel = {k: v[1] for k, v in kernels.items() if frag in k}
    assert sel and all(v == 0 for v in sel.values()), sel
