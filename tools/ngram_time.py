#!/usr/bin/env python3
"""Cost of no_repeat_ngram_size on the 0.5B-shape decode step (GPU box):  python tools/ngram_time.py [--rounds 3]

Per context length (prompts of 200 and 900 ids: the timed steps run at contexts of about 280 and 1000) and live-row count
(1, 8, 32) a session admits its rows with no record ("plain": the step graph without the feature bit) or with
no_repeat_ngram_size = 3 on every greedy row ("ngram": the lm_head writes the logits rows, k_ngram_ban and k_penalize run),
captures its step graphs, then times graph replays of 64 decode steps with HIP events on the session's stream (best of 3).
Each mode runs in a fresh child process and the modes alternate over the rounds (clock and thermal drift fall on both alike);
the arena is packed once and handed to the children as a file.  Prints one line per case: the median over rounds of both,
the difference, and every round's figure (their spread is what the difference is judged against)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
ROWS = (1, 8, 32)
PROMPTS = (200, 900)
MAX_POS = 1280


def child(arena_path: str, mode: str) -> None:
    import numpy as np
    import torch
    from sparkmi import config as Cf
    from sparkmi.llm import SparkLLM
    cfg = Cf.spark_0p5b_llm()
    arena = torch.from_numpy(np.load(arena_path, mmap_mode="r").copy()).to("cuda:0")
    out = {}
    for P, B in ((P, B) for P in PROMPTS for B in ROWS):
        llm = SparkLLM(cfg, None, "cuda:0", max_slots=B, max_positions=MAX_POS, arena=arena, kv_dtype="bf16")
        prompts = [np.random.Generator(np.random.PCG64(1 + b)).integers(0, cfg.vocab_size, size=P).tolist() for b in range(B)]
        llm.session_begin()
        llm.admit(prompts, [{"no_repeat_ngram_size": 3} for _ in range(B)] if mode == "ngram" else None)
        llm.decode(16)                                   # captures the one-step and the 8-step graphs
        st = torch.cuda.current_stream()
        best = float("inf")
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            llm.decode(64)
            e1.record(st)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / 64)
        out[f"{P}/{B}"] = best
        del llm
        torch.cuda.synchronize()
    print(json.dumps(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", nargs=2, metavar=("ARENA", "MODE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return
    import numpy as np
    from sparkmi import config as Cf, weights as W
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    cfg = Cf.spark_0p5b_llm()
    res = {"plain": [], "ngram": []}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "arena.npy")
        np.save(path, pack_llm_arena(cfg, W.SyntheticLLM(cfg), llm_cfg_struct(cfg, 1, MAX_POS, "bf16", True)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "spark-tts_amd")]))
        for r in range(a.rounds):
            for mode in (("plain", "ngram") if r % 2 == 0 else ("ngram", "plain")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, mode], env=env,
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(f"{mode} child exited with {p.returncode}\n{p.stderr[-3000:]}")
                res[mode].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(f"round {r} {mode}: {res[mode][-1]}", file=sys.stderr, flush=True)
    for k in [f"{P}/{B}" for P in PROMPTS for B in ROWS]:
        u = float(np.median([x[k] for x in res["plain"]]))
        v = float(np.median([x[k] for x in res["ngram"]]))
        print(f"prompt/rows {k:>6}: plain {u:7.1f} us/step   ngram {v:7.1f} us/step   ({v - u:+.1f} us; "
              f"rounds: {[round(x[k], 1) for x in res['plain']]} / {[round(x[k], 1) for x in res['ngram']]})", flush=True)


if __name__ == "__main__":
    main()
