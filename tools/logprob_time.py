#!/usr/bin/env python3
"""Cost of the per-token log-probabilities on the 0.5B-shape decode step (GPU box):  python tools/logprob_time.py [--rounds 3]

Per live-row count (1, 8, 32) a session admits its rows without the flag ("plain": today's step graph) or with
return_log_probs on every row ("flagged": the lm_head writes the logits rows and k_logprob runs), captures its step graphs,
then times graph replays of 64 decode steps with HIP events on the session's stream (best of 5).  Each mode runs in a fresh
child process and the modes alternate over the rounds (clock and thermal drift fall on both alike); the arena is packed once
and handed to the children as a file.  Prints one line per row count: the median over rounds of both, and the difference."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
ROWS = (1, 8, 32)
FLAG = {"return_log_probs": True}


def child(arena_path: str, mode: str) -> None:
    import numpy as np
    import torch
    from sparkmi import config as Cf
    from sparkmi.llm import SparkLLM
    cfg = Cf.spark_0p5b_llm()
    arena = torch.from_numpy(np.load(arena_path, mmap_mode="r").copy()).to("cuda:0")
    out = {}
    for B in ROWS:
        llm = SparkLLM(cfg, None, "cuda:0", max_slots=B, max_positions=512, arena=arena, kv_dtype="bf16")
        prompts = [np.random.Generator(np.random.PCG64(1 + b)).integers(0, cfg.vocab_size, size=128).tolist() for b in range(B)]
        llm.session_begin()
        llm.admit(prompts, [dict(FLAG) for _ in range(B)] if mode == "flagged" else None)
        llm.decode(16)                                   # captures the one-step and the 8-step graphs
        st = torch.cuda.current_stream()
        best = float("inf")
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            llm.decode(64)
            e1.record(st)
            e1.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / 64)
        out[B] = best
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
    res = {"plain": [], "flagged": []}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "arena.npy")
        np.save(path, pack_llm_arena(cfg, W.SyntheticLLM(cfg), llm_cfg_struct(cfg, 1, 512, "bf16", True)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "spark-tts_amd")]))
        for r in range(a.rounds):
            for mode in (("plain", "flagged") if r % 2 == 0 else ("flagged", "plain")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, mode], env=env,
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(f"{mode} child exited with {p.returncode}\n{p.stderr[-3000:]}")
                res[mode].append({int(k): v for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()})
    for B in ROWS:
        u = float(np.median([x[B] for x in res["plain"]]))
        v = float(np.median([x[B] for x in res["flagged"]]))
        print(f"{B:3d} rows: plain {u:7.1f} us/step   flagged {v:7.1f} us/step   (+{v - u:.1f} us; "
              f"rounds: {[round(x[B], 1) for x in res['plain']]} / {[round(x[B], 1) for x in res['flagged']]})", flush=True)


if __name__ == "__main__":
    main()
