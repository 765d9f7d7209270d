#!/usr/bin/env python3
"""Cost and saving of allowed-token constraints on the 0.5B-shape decode step (GPU box):
    python tools/constrain_time.py [--rounds 3] [--profile]

Per live-row count (1, 8, 32) a session admits its rows with no allow record ("plain": today's step graph) or with every row
constrained to [151643, 166000) ("constrained": the restricted lm_head reads only the tiles of that range), greedy and sampled
(temperature 0.8, top-k 50, top-p 0.95, seeded), captures its step graphs, then times graph replays of 64 decode steps with HIP
events on the session's stream (best of 5).  Each mode runs in a fresh child process and the modes alternate over the rounds;
the arena is packed once and handed to the children as a file.  Prints one line per (selection, row count): the median over
rounds of both modes and the difference.  --profile adds one child per mode under `rocprofv3 --kernel-trace --stats` (csv output; a run of
its own) and prints the lm_head kernels' average time from its kernel statistics."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
ROWS = (1, 8, 32)
SPEECH = (151643, 166000)
SAMPLED = {"do_sample": True, "temperature": 0.8, "top_k": 50, "top_p": 0.95}


def child(arena_path: str, mode: str) -> None:
    import numpy as np
    import torch
    from sparkmi import config as Cf
    from sparkmi.llm import ALLOW_KEY, SparkLLM
    cfg = Cf.spark_0p5b_llm()
    arena = torch.from_numpy(np.load(arena_path, mmap_mode="r").copy()).to("cuda:0")
    out = {}
    for sel in ("greedy", "sampled"):
        for B in ROWS:
            llm = SparkLLM(cfg, None, "cuda:0", max_slots=B, max_positions=512, arena=arena, kv_dtype="bf16")
            prompts = [np.random.Generator(np.random.PCG64(1 + b)).integers(0, 151643, size=128).tolist() for b in range(B)]
            recs = []
            for b in range(B):
                d = dict(SAMPLED, seed=10 + b) if sel == "sampled" else {"do_sample": False}
                if mode == "constrained":
                    d[ALLOW_KEY] = range(*SPEECH)
                recs.append(d)
            llm.session_begin()
            llm.admit(prompts, recs)
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
            out[f"{sel}:{B}"] = best
            del llm
            torch.cuda.synchronize()
    print(json.dumps(out))


def profile(path: str, env: dict, mode: str) -> None:
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", os.path.join(d, "run"), "--",
               sys.executable, os.path.abspath(__file__), "--child", path, mode]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"rocprofv3 ({mode}) exited with {p.returncode}\n{p.stderr[-3000:]}")
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            found = glob.glob(os.path.join(d, "**", "*"), recursive=True)
            sys.exit(f"rocprofv3 ({mode}): no kernel statistics among {found[:20]}\n{p.stdout[-1500:]}\n{p.stderr[-1500:]}")
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "k_lm" in name:
                    print(f"  {mode:11s} {name[:60]:60s} calls {row.get('Calls')}  avg {float(row.get('AverageNs', 0)) / 1e3:.2f} us",
                          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--child", nargs=2, metavar=("ARENA", "MODE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return
    import numpy as np
    from sparkmi import config as Cf, weights as W
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    cfg = Cf.spark_0p5b_llm()
    res = {"plain": [], "constrained": []}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "arena.npy")
        np.save(path, pack_llm_arena(cfg, W.SyntheticLLM(cfg), llm_cfg_struct(cfg, 1, 512, "bf16", True)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "spark-tts_amd")]))
        for r in range(a.rounds):
            for mode in (("plain", "constrained") if r % 2 == 0 else ("constrained", "plain")):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, mode], env=env,
                                   capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(f"{mode} child exited with {p.returncode}\n{p.stderr[-3000:]}")
                res[mode].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for key in (res["plain"][0] if a.rounds > 0 else ()):
            u = float(np.median([x[key] for x in res["plain"]]))
            v = float(np.median([x[key] for x in res["constrained"]]))
            sel, B = key.split(":")
            print(f"{sel:7s} {int(B):3d} rows: plain {u:7.1f} us/step   constrained {v:7.1f} us/step   ({v - u:+.1f} us; rounds: "
                  f"{[round(x[key], 1) for x in res['plain']]} / {[round(x[key], 1) for x in res['constrained']]})", flush=True)
        if a.profile:
            print("lm_head kernels (rocprofv3 --kernel-trace --stats; every step of one child: greedy and sampled, 1 / 8 / 32 rows):")
            for mode in ("plain", "constrained"):
                profile(path, env, mode)


if __name__ == "__main__":
    main()
