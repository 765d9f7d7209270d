#!/usr/bin/env python3
"""Which kernel form every layer GEMM and the lm_head start with, per row count, as a kernel trace shows it.

  run     (GPU, under `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gemm_forms_trace.py run OUT.json`):
          eager sessions (use_graph=False) on the diagnostics library -- or on the library SPARKMI_LIB names --, M live rows in
          identity slots, three decode steps at every row count at which a pick changes (either side); one prompt of 66, 513 and
          514 tokens; one-row decode with SPARKMI_NO_FUSE_O=1 and SPARKMI_TUNE2=3145728 at 1 and 4 rows.  Shapes: tiny_llm()
          (TPC 2, 4 heads) and the 0.5B widths with three layers (TPC 10, 14 heads; first, middle and last layer).  One torch
          kernel separates the segments in the trace; OUT.json lists the segments' names in order.
  reduce  (anywhere): reduce TRACE_DIR SEGMENTS.json OUT.json [LAUNCH_NOTE] -- the trace as {case: [[kernel, grid x, y, z,
          workgroup, LDS bytes as the trace reports them, dynamic LDS bytes], ...]} in launch order (kernel names without
          namespace, argument list and blanks; grid in blocks).  The kernel trace of ROCm 7.2 reports a kernel's static LDS
          only, so the dynamic bytes come from LAUNCH_NOTE: one line "grid x y z, threads, dynamic LDS" per launch of the
          library, in launch order, written by a throwaway note in the library's launch macro (never committed); without it
          the last column is absent.
tests/golden/gemm_forms.json is the reduction of the parent commit's trace; the same run on a later build must give the same
bytes, and tests/test_gemm_forms_cpu.py holds smi_llm_gemm_forms to it.
"""
import csv
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "spark-tts_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 32, 33, 64]
ROWS_F32 = [1, 16, 17]
PROMPTS = [66, 513, 514]
TUNE2_DOWN_GEMM = 3145728      # kTune2GemmDown1 | kTune2GemmDownS: down_proj on k_gemm<.., H = 4>
MAX_POS = 576


def shapes():
    from sparkmi import config as C
    import dataclasses
    return {"tiny": C.tiny_llm(), "half": dataclasses.replace(C.spark_0p5b_llm(), num_hidden_layers=3)}


def run(out_path):
    import numpy as np
    import torch
    from sparkmi import weights as W
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    from sparkmi.llm import SparkLLM

    names = []
    mark = torch.zeros(4099, device="cuda:0")

    def segment(name):
        torch.cuda.synchronize()
        mark.add_(1.0)              # the one torch kernel between two segments
        torch.cuda.synchronize()
        names.append(name)

    def engine(cfg, arena, kv, env):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return SparkLLM(cfg, None, "cuda:0", max_slots=64, max_positions=MAX_POS, arena=arena, kv_dtype=kv, use_graph=False, diag=True)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def decode_case(llm, cfg, name, M):
        rng = np.random.Generator(np.random.PCG64(M))
        prompts = rng.integers(0, cfg.vocab_size, size=(M, 3)).tolist()
        segment("setup")
        llm.session_begin(None)
        assert llm.admit(prompts) == list(range(M)), "rows are not in identity slots"
        segment(name)
        llm.decode(3)
        segment("setup")
        llm.retire_many(list(range(M)))

    segment("setup")
    for sname, cfg in shapes().items():
        syn = W.SyntheticLLM(cfg)
        arena = torch.from_numpy(pack_llm_arena(cfg, syn, llm_cfg_struct(cfg, 1, MAX_POS, "bf16", False))).to("cuda:0")
        for kv, rows in (("bf16", ROWS), ("f32", ROWS_F32)):
            llm = engine(cfg, arena, kv, {})
            for M in rows:
                decode_case(llm, cfg, f"{sname}/{kv}/decode/M={M}", M)
            if kv == "bf16":
                for n in PROMPTS:
                    prompt = np.random.Generator(np.random.PCG64(n)).integers(0, cfg.vocab_size, size=n).tolist()
                    segment(f"{sname}/{kv}/prefill/tokens={n}")
                    llm.prefill([prompt])
                    segment("setup")
            llm.close()
        llm = engine(cfg, arena, "bf16", {"SPARKMI_NO_FUSE_O": "1"})
        decode_case(llm, cfg, f"{sname}/bf16/decode/no_fuse_o/M=1", 1)
        llm.close()
        llm = engine(cfg, arena, "bf16", {"SPARKMI_TUNE2": str(TUNE2_DOWN_GEMM)})
        for M in (1, 4):
            decode_case(llm, cfg, f"{sname}/bf16/decode/tune2={TUNE2_DOWN_GEMM}/M={M}", M)
        llm.close()
    segment("end")
    with open(out_path, "w") as f:
        json.dump(names, f)
    print(f"{len(names)} segments, {sum(n != 'setup' and n != 'end' for n in names)} cases -> {out_path}")


def short_name(name):
    """'void (anonymous namespace)::k_gemm<1, 1, ...>((anonymous namespace)::GemmP)' -> 'k_gemm<1,1,...>'"""
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    depth, end = 0, len(name)
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            end = i
            break
    return name[:end].replace(" ", "").removesuffix(".kd")


def reduce(trace_dir, segments_path, out_path, note_path=None):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, f"one kernel trace expected under {trace_dir}: {files}"
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = json.load(open(segments_path))
    note = [[int(x) for x in line.split()] for line in open(note_path)] if note_path else None
    cases, seg, cur, n = {}, -1, None, 0
    for r in rows:
        k = short_name(r["Kernel_Name"])
        if not k.startswith("k_"):          # every kernel of the library is k_*
            if "CUDAFunctorOnSelf_add" not in k:
                continue                    # the runtime's copy / fill kernels, the separator tensor's own fill
            seg += 1
            assert seg < len(names), "more separators in the trace than segments"
            cur = None if names[seg] in ("setup", "end") else cases.setdefault(names[seg], [])
            continue
        wg = [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"]
        grid = [int(r[f"Grid_Size_{a}"]) // w for a, w in zip("XYZ", wg)]
        entry = [k, grid[0], grid[1], grid[2], wg[0] * wg[1] * wg[2], int(r["LDS_Block_Size"])]
        if note is not None:                # launch n of the library: the note's line n
            assert n < len(note) and note[n][:4] == entry[1:5], f"launch {n} ({entry}): the note says {note[n] if n < len(note) else None}"
            entry.append(note[n][4])
        n += 1
        if cur is not None:
            cur.append(entry)
    assert seg == len(names) - 1, f"{seg + 1} separators in the trace, {len(names)} segments"
    assert note is None or n == len(note), f"{n} launches in the trace, {len(note)} in the note"
    with open(out_path, "w") as f:
        f.write("{\n")
        f.write(",\n".join(f" {json.dumps(c)}: {json.dumps(e, separators=(',', ':'))}" for c, e in cases.items()))
        f.write("\n}\n")
    print(f"{len(cases)} cases, {sum(len(c) for c in cases.values())} launches -> {out_path}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) in (5, 6) and sys.argv[1] == "reduce":
        reduce(*sys.argv[2:])
    else:
        sys.exit(__doc__)
