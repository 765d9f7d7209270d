#!/usr/bin/env python3
"""The pitch stage on the device against the two existing calls it fuses, and against the vocoder call that produces the same
rows (GPU box):
    python tools/pitch_time.py [--pairs 5] [--out FILE]

`DeviceAudio.pitch_rows` (two launches: k_tempo_search, k_pitch_ola; the stretched signal stays in LDS) for 1, 8 and 32 rows of
3 s at 16 kHz, at +2 semitones (28/25) and +7 (3/2), alone and with tempo 1.25, against
  - `DeviceAudio.tempo_rows` at the same stretch P/Q followed by `DeviceAudio.resample_rows` at up/down and the cut (a view):
    three launches, the stretched rows written to memory and read back;
  - `BiCodecVocoder.detokenize` of the full-size vocoder (synthetic weights) for the same number of rows of 150 frames = 3 s.
Every figure is a host clock around `reps` back-to-back calls that end in one synchronise, divided by `reps`; `alone` is one call
from a drained device to a drained device.  The three alternate pair by pair in one process; each figure is the median over the
pairs with min .. max beside it.  The fused call's samples and places are checked against the two calls', bit for bit, before
anything is timed.  The rows are those of tools/tempo_time.py: a gliding 7-harmonic tone with noise, each row its own.
Not measured: real speech and a real checkpoint."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))

SR = 16000
SECONDS = 3.0
FRAMES = 150                                 # vocoder frames of 3 s
SHAPES = ((1, 50), (8, 50), (32, 30))        # rows, calls a timed window
SHIFTS = (2, 7)                              # semitones
TEMPOS = (None, 1.25)


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
    from bench import build_hash
    from sparkmi import _lib, audio, config as C, weights as W
    from sparkmi.bicodec import BiCodecVocoder
    sync = torch.cuda.synchronize
    dev = "cuda:0"
    da = audio.DeviceAudio(dev)
    N, D = audio.tempo_frame(SR)
    f = lambda s: f"{s[0]:9.4f} ({s[1]:.4f} .. {s[2]:.4f})"   # noqa: E731
    head = (f"tools/pitch_time.py, build {build_hash()}; ms per call at {SR} Hz, N = {N}, D = {D}, rows of {SECONDS:g} s, "
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
        for shift in SHIFTS:
            for tempo in TEMPOS:
                tq = (1, 1) if tempo is None else audio.tempo_ratio(tempo)
                rq = audio.pitch_ratio(shift)
                P, Q, up, down = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
                M = ctypes.c_longlong()
                n_out = _lib.lib().smi_pitch_layout(n, tq[0], tq[1], rq[0], rq[1], N, ctypes.byref(P), ctypes.byref(Q), ctypes.byref(M), None,
                                                    ctypes.byref(up), ctypes.byref(down))
                lens, tempos, shifts = [n] * B, [tq] * B, [rq] * B
                stretch, ups, downs = [(P.value, Q.value)] * B, [up.value] * B, [down.value] * B

                def two_calls():
                    z, zm, zpos = da.tempo_rows(x, lens, stretch, sr=SR)
                    w, _ = da.resample_rows(z, zm, ups, downs)
                    return w[:, :n_out], zpos

                for _ in range(2):
                    y, m, pos = da.pitch_rows(x, lens, tempos, shifts, sr=SR)
                    w, zpos = two_calls()
                    sync()
                assert m == [n_out] * B, (m, n_out)
                same = sum(int(torch.equal(y[b, :n_out].view(torch.int32), w[b].contiguous().view(torch.int32)) and torch.equal(pos[b], zpos[b]))
                           for b in range(B))
                assert same == B, (same, B)
                fused, alone, two, two_alone, vocd = [], [], [], [], []
                for _ in range(a.pairs):
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        da.pitch_rows(x, lens, tempos, shifts, sr=SR)
                    sync()
                    t1 = time.perf_counter()
                    da.pitch_rows(x, lens, tempos, shifts, sr=SR)
                    sync()
                    t2 = time.perf_counter()
                    for _ in range(reps):
                        two_calls()
                    sync()
                    t3 = time.perf_counter()
                    two_calls()
                    sync()
                    t4 = time.perf_counter()
                    for _ in range(reps):
                        voc.detokenize(sem, glob)
                    sync()
                    t5 = time.perf_counter()
                    fused.append((t1 - t0) * 1e3 / reps); alone.append((t2 - t1) * 1e3); two.append((t3 - t2) * 1e3 / reps)
                    two_alone.append((t4 - t3) * 1e3); vocd.append((t5 - t4) * 1e3 / reps)
                for line in (f"{B} x {SECONDS:g} s at {shift:+d} semitones = {rq[0]}/{rq[1]}, tempo {tq[0]}/{tq[1]}: stretch {P.value}/{Q.value} to "
                             f"{M.value} samples, resampled {up.value}/{down.value}, {n_out} samples out; {same} of {B} rows bit-equal to the "
                             f"two calls', places and samples:",
                             f"  device pitch_rows, {reps} calls back to back                 {f(stat(fused))}",
                             f"  device pitch_rows, one call alone                        {f(stat(alone))}",
                             f"  tempo_rows + resample_rows + cut, {reps} back to back        {f(stat(two))}",
                             f"  tempo_rows + resample_rows + cut, once alone             {f(stat(two_alone))}",
                             f"  vocoder detokenize, {reps} calls back to back                {f(stat(vocd))}"):
                    lines.append(line)
                    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
