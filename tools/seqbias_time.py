#!/usr/bin/env python3
"""Cost of the sequence-bias stage and the stop match on the 0.5B-shape decode step (GPU box):
    python tools/seqbias_time.py [--rounds 3] [--parent-lib PATH/libsparkmi.so]

Per live-row count (1, 8, 32) a session admits its rows with no record ("plain": the step graph without the sequence bits), with
bias entries on every row ("bias": the lm_head writes the logits rows, k_penalize runs stage 0b and rebuilds the maxima), with
stop sequences alone ("stop": k_finalize gets the records) or with both ("both"), captures its step graphs, then times graph
replays of 64 decode steps with HIP events on the session's stream (best of 5).  Each mode runs in a fresh child process and
the modes alternate over the rounds (clock and thermal drift fall on all alike); the arena is packed once and handed to the
children as a file.  ``--parent-lib``: a build of the commit before the feature, timed as a mode of its own ("parent": the
plain session on that library, SPARKMI_LIB in the child) -- the unrecorded path against its parent, in the same alternation.
Prints one line per row count: the median over rounds of every mode, the differences to "plain", and the rounds."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
ROWS = (1, 8, 32)


def record(mode: str, prompt, V: int):
    """Eight bias entries (length 1, 2 and 3, one -inf, some matching the prompt tail) and / or three stop sequences that never fire"""
    rec = {}
    if mode in ("bias", "both"):
        rec["sequence_bias"] = [((7,), -2.0), ((V - 9,), 1.5), ((prompt[-1], 11), 3.0), ((prompt[-2], prompt[-1], 12), -1.0),
                                ((5, 6, 13), 2.0), ((V // 2,), -0.5), ((V // 3, 14), 4.0)]
        rec["bad_words_ids"] = [[V // 5]]
    if mode in ("stop", "both"):
        rec["stop_sequences"] = [[V - 1, V - 1, V - 1], [V - 2, V - 1], [V - 3] * 8]
    return rec or None


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
        recs = [record(mode, p, cfg.vocab_size) for p in prompts]
        llm.admit(prompts, recs if recs[0] is not None else None)
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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--modes", default="plain,bias,stop,both")
    ap.add_argument("--child", nargs=2, metavar=("ARENA", "MODE"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return
    import numpy as np
    from sparkmi import config as Cf, weights as W
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    cfg = Cf.spark_0p5b_llm()
    modes = [m for m in a.modes.split(",") if m] + (["parent"] if a.parent_lib else [])
    res = {m: [] for m in modes}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "arena.npy")
        np.save(path, pack_llm_arena(cfg, W.SyntheticLLM(cfg), llm_cfg_struct(cfg, 1, 512, "bf16", True)))
        env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "spark-tts_amd")]))
        for r in range(a.rounds):
            for mode in (modes if r % 2 == 0 else modes[::-1]):
                e = dict(env, SPARKMI_LIB=os.path.abspath(a.parent_lib)) if mode == "parent" else env
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "plain" if mode == "parent" else mode],
                                   env=e, capture_output=True, text=True, timeout=900)
                if p.returncode != 0:
                    sys.exit(f"{mode} child exited with {p.returncode}\n{p.stderr[-3000:]}")
                res[mode].append({int(k): v for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items()})
    for B in ROWS:
        med = {m: float(np.median([x[B] for x in res[m]])) for m in modes}
        base = med.get("plain", next(iter(med.values())))
        print(f"{B:3d} rows: " + "   ".join(f"{m} {med[m]:7.1f} us/step ({med[m] - base:+.1f})" for m in modes) +
              "   rounds: " + " / ".join(str([round(x[B], 1) for x in res[m]]) for m in modes), flush=True)


if __name__ == "__main__":
    main()
