#!/usr/bin/env python3
"""Cost of n takes of one prompt at the 0.5B shape (GPU box):  python tools/fork_time.py [--reps 3] [--out FILE]

For a prompt of L tokens (L in 128, 460) and n takes (n in 1, 2, 4, 8, 16, 32), times one admission into an empty session --
SparkLLM.admit([p] * n) ("expanded": n prefills) against SparkLLM.admit([p], n_return=[n]) ("forked": one prefill, the KV
fork copy, one n-row step) -- on a contiguous and on a paged KV cache (64-token pages), and reads the KV pages the admission
took.  Wall time of the call with the stream drained before and after (an admission ends with a host round trip of its own),
best of --reps after one untimed warm-up admission per configuration.  Prints the build hash (bench.py's build_hash) and
one line per (cache, L, n); --out also writes the table and the raw JSON there."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
LENS = (128, 460)
TAKES = (1, 2, 4, 8, 16, 32)
PAGE = 64
MAX_POS = 512


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_hash
    from sparkmi import config as Cf, weights as W
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    from sparkmi.llm import SparkLLM
    cfg = Cf.spark_0p5b_llm()
    arena = torch.from_numpy(pack_llm_arena(cfg, W.SyntheticLLM(cfg), llm_cfg_struct(cfg, 1, MAX_POS, "bf16", True))).to("cuda:0")
    lines = [f"tools/fork_time.py, build {build_hash()}, 0.5B shape, bf16 KV, max_positions {MAX_POS}, "
             f"paged: {PAGE}-token pages; wall ms per admission (best of {a.reps}) and KV pages taken"]
    print(lines[0], flush=True)
    rows = []
    for paged in (False, True):
        n_max = max(TAKES)
        kw = dict(kv_page_tokens=PAGE, kv_pages=n_max * (MAX_POS // PAGE)) if paged else {}
        llm = SparkLLM(cfg, None, "cuda:0", max_slots=n_max, max_positions=MAX_POS, arena=arena, kv_dtype="bf16", **kw)
        for L in LENS:
            p = np.random.Generator(np.random.PCG64(L)).integers(0, cfg.vocab_size, size=L).tolist()
            res = {}
            for n in TAKES:
                for mode in ("expanded", "forked"):
                    def admit():
                        return llm.admit([p] * n) if mode == "expanded" else llm.admit([p], None, n_return=[n])
                    llm.session_begin()
                    admit()                                          # warm-up: plan / workspace growth, first launches
                    best, pages = float("inf"), 0
                    for _ in range(a.reps):
                        llm.session_begin()
                        torch.cuda.synchronize()
                        free0 = llm.kv_pages()[1]
                        t0 = time.perf_counter()
                        admit()
                        torch.cuda.synchronize()
                        best = min(best, (time.perf_counter() - t0) * 1e3)
                        pages = free0 - llm.kv_pages()[1]
                    res[(n, mode)] = (best, pages)
                    rows.append(dict(cache="paged" if paged else "contiguous", L=L, n=n, mode=mode, ms=round(best, 3), pages=pages))
                e, f = res[(n, "expanded")], res[(n, "forked")]
                line = (f"{'paged' if paged else 'contiguous':10s} L={L:3d} n={n:2d}: expanded {e[0]:7.2f} ms"
                        + (f" {e[1]:3d} pages" if paged else "") + f"   forked {f[0]:7.2f} ms" + (f" {f[1]:3d} pages" if paged else "")
                        + f"   ({e[0] / f[0]:.2f}x)")
                lines.append(line)
                print(line, flush=True)
        llm.close()
        del llm
        torch.cuda.synchronize()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps({"build": build_hash(), "rows": rows}) + "\n")


if __name__ == "__main__":
    main()
