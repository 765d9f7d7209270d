#!/usr/bin/env python3
"""Tempo on the device against the host and against the vocoder call that produces the same rows (GPU box):
    python tools/tempo_time.py [--pairs 5] [--out FILE]

`DeviceAudio.tempo_rows` (two launches; the rows are on the device before and after, as they are behind the vocoder) for 1, 8
and 32 rows of 3 s at 16 kHz, at tempo 1.25 (about one frame in four is searched) and at 2.0 (every frame is searched), against
  - tests/tempo_ref.py on the host, row by row, with the copy of the rows to the host and of the results back to the device that
    a pipeline doing the stage there would need;
  - `BiCodecVocoder.detokenize` of the full-size vocoder (synthetic weights) for the same number of rows of 150 frames = 3 s.
The device figure is a host clock around `reps` back-to-back calls that end in one synchronise, divided by `reps`; `alone` is one
call from a drained device to a drained device.  The three alternate pair by pair in one process; each figure is the median over
the pairs with min .. max beside it.  The device's places and samples are checked against the host's, bit for bit, before
anything is timed.  The rows are a gliding 7-harmonic tone with noise, each row its own."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000
SECONDS = 3.0
FRAMES = 150                                 # vocoder frames of 3 s
SHAPES = ((1, 50), (8, 50), (32, 30))        # rows, calls a timed window
TEMPOS = (1.25, 2.0)


def stat(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import tempo_ref as R
    from bench import build_hash
    from sparkmi import audio, config as C, weights as W
    from sparkmi.bicodec import BiCodecVocoder
    sync = torch.cuda.synchronize
    dev = "cuda:0"
    da = audio.DeviceAudio(dev)
    N, D = audio.tempo_frame(SR)
    f = lambda s: f"{s[0]:9.4f} ({s[1]:.4f} .. {s[2]:.4f})"   # noqa: E731
    head = (f"tools/tempo_time.py, build {build_hash()}; ms per call at {SR} Hz, N = {N}, D = {D}, rows of {SECONDS:g} s, "
            f"median of {a.pairs} alternating pairs (min .. max)")
    lines = [head]
    print(head, flush=True)
    cfg = C.spark_0p5b_bicodec()
    voc = BiCodecVocoder(cfg, W.bicodec_detok_state(cfg), dev, max_batch=max(b for b, _ in SHAPES), max_frames=FRAMES + 10)
    rng = np.random.default_rng(11)
    n = int(SECONDS * SR)
    t = np.arange(n) / SR
    for B, reps in SHAPES:
        rows = []
        for i in range(B):
            f0 = (100.0 + 7 * i) * (1.0 + 0.15 * np.sin(2 * np.pi * 0.4 * t + i))
            ph = 2 * np.pi * np.cumsum(f0) / SR
            v = sum(np.sin(h * ph) / h for h in range(1, 8))
            rows.append((0.5 * v / np.max(np.abs(v)) + 0.02 * rng.standard_normal(n)).astype(np.float32))
        x = torch.from_numpy(np.stack(rows)).to(dev)
        sem = torch.from_numpy(rng.integers(0, cfg.codebook_size, size=(B, FRAMES)))
        glob = torch.from_numpy(rng.integers(0, 4096, size=(B, 1, cfg.spk_token_num)))
        for _ in range(2):
            voc.detokenize(sem, glob)
        sync()
        for tempo in TEMPOS:
            p, q = audio.tempo_ratio(tempo)
            lens, tempos = [n] * B, [tempo] * B

            def host_stage():
                h = x.cpu().numpy()
                outs = [R.tempo(h[b], p, q, N, D) for b in range(B)]
                return torch.from_numpy(np.stack([o for o, _ in outs])).to(dev), outs

            for _ in range(2):
                y, m, pos = da.tempo_rows(x, lens, tempos, sr=SR)
                sync()
            _, outs = host_stage()
            yh, ph_ = y.cpu().numpy(), pos.cpu().numpy()
            same = sum(int(np.array_equal(yh[b, : m[b]].view(np.uint32), outs[b][0].view(np.uint32))
                           and np.array_equal(ph_[b, : outs[b][1].size], outs[b][1].astype(np.int32))) for b in range(B))
            assert same == B, (same, B)
            searched = []
            R.positions(rows[0], p, q, N, D, searched)
            devt, alone, host, vocd = [], [], [], []
            for _ in range(a.pairs):
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    da.tempo_rows(x, lens, tempos, sr=SR)
                sync()
                t1 = time.perf_counter()
                da.tempo_rows(x, lens, tempos, sr=SR)
                sync()
                t2 = time.perf_counter()
                host_stage()
                sync()
                t3 = time.perf_counter()
                for _ in range(reps):
                    voc.detokenize(sem, glob)
                sync()
                t4 = time.perf_counter()
                devt.append((t1 - t0) * 1e3 / reps); alone.append((t2 - t1) * 1e3); host.append((t3 - t2) * 1e3)
                vocd.append((t4 - t3) * 1e3 / reps)
            for line in (f"{B} x {SECONDS:g} s at tempo {tempo:g} = {p}/{q} ({m[0]} samples out, {len(searched)} of {outs[0][1].size} frames of row 0 "
                         f"searched; {same} of {B} rows bit-equal to the host's, places and samples):",
                         f"  device tempo_rows, {reps} calls back to back   {f(stat(devt))}",
                         f"  device tempo_rows, one call alone          {f(stat(alone))}",
                         f"  host tempo_ref + the two copies            {f(stat(host))}",
                         f"  vocoder detokenize, {reps} calls back to back  {f(stat(vocd))}"):
                lines.append(line)
                print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
