#!/usr/bin/env python3
"""The look-ahead limiter on the device against the host and against the stage it replaces (GPU box):
    python tools/limiter_time.py [--pairs 9] [--out FILE]

For 1 x 3 s, 32 x 3 s and 1 x 60 s at 16 kHz (speech-like rows with a click each second, brought to -14 LUFS so that the limiter has
work to do; the rows are on the device before and after, as they are behind the vocoder; every call reads one buffer and writes a
second one, so every call sees the same rows):

  new      `DeviceAudio.loudness_rows` with a ceiling that cannot bind + `limit_rows` ("true", 40 / 400 samples): what
           `limiter="true"` with `loudness=` enqueues (four launches + two for the window + three)
  parent   `loudness_rows` + `gain_rows`: what `loudness=` alone enqueues, today and in the parent commit (five launches)
  limiter  `limit_rows` alone with the gain read from the stats, and its parts: "sample" mode (no oversampling) and A = R = 0 (no
           smoothing window), which tell where the time goes
  host     tests/limit_ref.py's `limit`: numpy float64, the same arithmetic in the same order, on rows already in host memory (no
           copy counted)

A device figure is a host clock around `reps` back-to-back calls that end in one synchronise, divided by `reps`; `alone` is one
call from a drained device to a drained device.  Device and host alternate pair by pair in one process; each figure is the median
over the pairs with min .. max beside it.  The device's rows are compared with the host's bit for bit before anything is timed.
No figure here is a pass / fail condition."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000
TARGET = -14.0
SHAPES = ((1, 3.0, 200, 3), (32, 3.0, 100, 1), (1, 60.0, 50, 1))   # rows, seconds, calls a timed window, host runs a pair


def stat(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import limit_ref as L
    from bench import build_hash
    from sparkmi import audio
    sync = torch.cuda.synchronize
    da = audio.DeviceAudio("cuda:0")
    A, R = audio.limiter_reach(SR)
    win, taps = audio.limiter_window(A, R), L.taps()
    f = lambda s: f"{s[0]:9.4f} ({s[1]:.4f} .. {s[2]:.4f})"   # noqa: E731
    head = (f"tools/limiter_time.py, build {build_hash()}; ms per call at {SR} Hz, target {TARGET:g} LUFS, ceiling {audio.PEAK_CEILING:.4f}, "
            f"A = {A}, R = {R}; median of {a.pairs} alternating pairs (min .. max)")
    lines = [head]
    print(head, flush=True)
    rng = np.random.default_rng(5)
    for B, seconds, reps, host_runs in SHAPES:
        n = int(seconds * SR)
        t = np.arange(n) / SR
        rows = []
        for i in range(B):
            x = ((0.05 + 0.25 * (np.sin(2 * np.pi * (0.3 + 0.1 * i) * t) > 0)) * np.sin(2 * np.pi * (140.0 + 9 * i) * t)
                 + 0.01 * rng.standard_normal(n))
            x[SR // 2 + 37 * i:: SR] = 0.8
            rows.append(x.astype(np.float32))
        x0 = torch.from_numpy(np.stack(rows)).to("cuda:0")
        x = x0.clone()
        lens, targets = [n] * B, [TARGET] * B

        def new():
            st = da.loudness_rows(x0, lens, targets=targets, ceiling=1e30, sr=SR)
            return st, da.limit_rows(x0, lens, gains=st, lookahead=A, release=R, out=x)

        def parent():
            st = da.loudness_rows(x0, lens, targets=targets, sr=SR)
            return da.gain_rows(x0, lens, st, out=x)

        st = da.loudness_rows(x0, lens, targets=targets, ceiling=1e30, sr=SR)
        parts = {"limit_rows, true, A, R": lambda: da.limit_rows(x0, lens, gains=st, lookahead=A, release=R, out=x),
                 "limit_rows, sample, A, R": lambda: da.limit_rows(x0, lens, gains=st, mode="sample", lookahead=A, release=R, out=x),
                 "limit_rows, true, 0, 0": lambda: da.limit_rows(x0, lens, gains=st, lookahead=0, release=0, out=x)}
        y, ls = parts["limit_rows, true, A, R"]()
        sync()
        g = st.cpu().numpy()[:, 2]
        host = lambda b: L.limit(rows[b], g[b], audio.PEAK_CEILING, taps, A, R, win)   # noqa: E731
        got, gls = y.cpu().numpy(), ls.cpu().numpy()
        check = list(range(B)) if n <= 100000 else [0]
        same = sum(int(np.array_equal(got[b].view(np.uint32), host(b)["out"].view(np.uint32))
                       and np.array_equal(gls[b].view(np.uint64), host(b)["stats"].view(np.uint64))) for b in check)
        assert same == len(check), (same, len(check))
        note = (f"{B} x {seconds:g} s ({n} samples a row; gain {g.min():.2f} .. {g.max():.2f}, true peak in {gls[:, 0].min():.2f} .. {gls[:, 0].max():.2f}, "
                f"{int(gls[:, 3].sum())} of {B * n} samples reduced, at most {-20 * np.log10(gls[:, 2].min()):.1f} dB; {same} of {len(check)} "
                f"rows and stats checked bit-equal to the host's):")
        res = {k: [] for k in ["new", "new alone", "parent", "parent alone", *parts, "host"]}
        for fn in (new, parent, *parts.values()):
            for _ in range(3):
                fn()
            sync()
        for _ in range(a.pairs):
            for name, fn in (("new", new), ("parent", parent)):
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                sync()
                t1 = time.perf_counter()
                fn()
                sync()
                t2 = time.perf_counter()
                res[name].append((t1 - t0) * 1e3 / reps); res[name + " alone"].append((t2 - t1) * 1e3)
            for name, fn in parts.items():
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                sync()
                res[name].append((time.perf_counter() - t0) * 1e3 / reps)
            t0 = time.perf_counter()
            for b in range(host_runs if B == 1 else B):
                host(b % B)
            res["host"].append((time.perf_counter() - t0) * 1e3 / (host_runs if B == 1 else 1))
        for line in (note,
                     f"  new: loudness_rows + limit_rows, {reps} back to back    {f(stat(res['new']))}",
                     f"  new, one call alone                                {f(stat(res['new alone']))}",
                     f"  parent: loudness_rows + gain_rows, {reps} back to back  {f(stat(res['parent']))}",
                     f"  parent, one call alone                             {f(stat(res['parent alone']))}",
                     *[f"  {k + ', back to back':<50s} {f(stat(res[k]))}" for k in parts],
                     f"  host float64 (numpy, limit_ref.limit), all rows     {f(stat(res['host']))}"):
            lines.append(line)
            print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
