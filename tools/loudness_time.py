#!/usr/bin/env python3
"""Output loudness on the device against the host, and what it adds to a long-form call (GPU box):
    python tools/loudness_time.py [--pairs 9] [--out FILE]

1.  `DeviceAudio.loudness_rows` + `gain_rows` (five launches; the rows are on the device before and after, as they are behind the
    vocoder) for 1 x 3 s, 32 x 3 s and 1 x 60 s at 16 kHz, against a host float64 implementation of the same measurement and gain
    on rows that are already in host memory: `scipy.signal.lfilter` for the two biquads, numpy for hops, blocks, gates and the
    scaling.  The device figure is a host clock around `reps` back-to-back call pairs that end in one synchronise, divided by
    `reps`; `alone` is one call pair from a drained device to a drained device (what a caller that waits for it sees).  The host's
    figure does not include the copy of the rows to the host and back that a pipeline would need.  The two alternate pair by
    pair in one process; each figure is the median over the pairs with min .. max beside it.  The device's loudness is checked
    against the host's (1e-9 LU) before anything is timed.
2.  `SparkTTS.inference_long` on the synthetic model directory of the tests (max_batch=2, greedy, 40 tokens a sentence, five
    sentences) with `loudness=None` and with `loudness=-23`, alternating."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))

SR = 16000
SHAPES = ((1, 3.0, 200), (32, 3.0, 100), (1, 60.0, 50))   # rows, seconds, call pairs a timed window
TEXT = ("The first sentence of the paragraph is this one. Then a second one follows it, a little longer than the first! "
        "Is the third one a question? The fourth sentence; short. And the fifth sentence closes the paragraph.")


def stat(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def host_normalize(rows, coef, block, target, max_gain_db, ceiling):
    """float64 on the host: (loudness per row, the scaled rows)"""
    import numpy as np
    from scipy.signal import lfilter
    hop = block // 4
    gate = 10.0 ** ((-70.0 + 0.691) / 10.0)
    louds, outs = [], []
    for x in rows:
        y = lfilter(coef[5:8], [1.0, coef[8], coef[9]], lfilter(coef[0:3], [1.0, coef[3], coef[4]], x.astype(np.float64)))
        e = y * y
        nh = e.size // hop
        H = e[: nh * hop].reshape(nh, hop).sum(axis=1)
        z = (H[:-3] + H[1:-2] + H[2:-1] + H[3:]) / block
        z = z[z > gate]
        z = z[z > 0.1 * z.mean()] if z.size else z
        loud = -0.691 + 10.0 * np.log10(z.mean()) if z.size else -np.inf
        g = 1.0
        if z.size:
            g = min(10.0 ** ((target - loud) / 20.0), 10.0 ** (max_gain_db / 20.0))
            peak = float(np.max(np.abs(x)))
            if g * peak > ceiling:
                g = ceiling / peak
        louds.append(loud)
        outs.append((x.astype(np.float64) * g).astype(np.float32))
    return louds, outs


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_hash
    from sparkmi import audio, synthetic
    from sparkmi.pipeline import SparkTTS
    sync = torch.cuda.synchronize
    da = audio.DeviceAudio("cuda:0")
    coef, block = audio.k_weighting(SR), audio.loudness_block(SR)
    f = lambda s: f"{s[0]:9.4f} ({s[1]:.4f} .. {s[2]:.4f})"   # noqa: E731
    head = (f"tools/loudness_time.py, build {build_hash()}; ms per call pair (loudness_rows + gain_rows, target -23 LUFS) at {SR} Hz, "
            f"median of {a.pairs} alternating pairs (min .. max)")
    lines = [head]
    print(head, flush=True)
    rng = np.random.default_rng(5)
    for B, seconds, reps in SHAPES:
        n = int(seconds * SR)
        t = np.arange(n) / SR
        rows = [((0.05 + 0.25 * (np.sin(2 * np.pi * (0.3 + 0.1 * i) * t) > 0)) * np.sin(2 * np.pi * (140.0 + 9 * i) * t)
                 + 0.01 * rng.standard_normal(n)).astype(np.float32) for i in range(B)]
        x = torch.from_numpy(np.stack(rows)).to("cuda:0")
        lens, targets = [n] * B, [-23.0] * B

        def device_pair():
            stats = da.loudness_rows(x, lens, targets=targets, sr=SR)
            return stats, da.gain_rows(x, lens, stats)

        for _ in range(3):
            stats, y = device_pair()
            sync()
        want, outs = host_normalize(rows, coef, block, -23.0, 20.0, audio.PEAK_CEILING)
        got = stats.cpu().numpy()
        err = max(abs(g - w) for g, w in zip(got[:, 0], want))
        assert err < 1e-9, err
        same = sum(int(np.array_equal(y[b].cpu().numpy(), outs[b])) for b in range(B))
        dev, alone, host = [], [], []
        for _ in range(a.pairs):
            sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                device_pair()
            sync()
            t1 = time.perf_counter()
            device_pair()
            sync()
            t2 = time.perf_counter()
            host_normalize(rows, coef, block, -23.0, 20.0, audio.PEAK_CEILING)
            t3 = time.perf_counter()
            dev.append((t1 - t0) * 1e3 / reps); alone.append((t2 - t1) * 1e3); host.append((t3 - t2) * 1e3)
        for line in (f"{B} x {seconds:g} s ({n} samples a row; device - host loudness at most {err:.1e} LU; {same} of {B} scaled rows bit-equal):",
                     f"  device, {reps} pairs back to back  {f(stat(dev))}",
                     f"  device, one pair alone          {f(stat(alone))}",
                     f"  host float64 (lfilter + numpy)  {f(stat(host))}"):
            lines.append(line)
            print(line, flush=True)
    # ---- inference_long with and without loudness
    with tempfile.TemporaryDirectory() as d:
        lcfg, vcfg = synthetic.make_model_dir(d)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
        glob = torch.from_numpy(np.random.Generator(np.random.PCG64(23)).integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        kw = dict(prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)), allowed_token_ids=sorted(tts._map.sem) + list(tts._eos),
                  min_new_tokens=14, do_sample=False, max_new_tokens=40, trim=False)
        for _ in range(2):
            tts.inference_long(TEXT, **kw)
            tts.inference_long(TEXT, loudness=-23.0, **kw)
        off, on = [], []
        for _ in range(a.pairs):
            sync()
            t0 = time.perf_counter()
            tts.inference_long(TEXT, **kw)
            t1 = time.perf_counter()
            tts.inference_long(TEXT, loudness=-23.0, **kw)
            t2 = time.perf_counter()
            off.append((t1 - t0) * 1e3); on.append((t2 - t1) * 1e3)
        diff = [b - c for b, c in zip(on, off)]
        for line in ("inference_long, synthetic model directory, five sentences, greedy, max_batch=2 (ms per call; the result is on the host):",
                     f"  loudness=None   {f(stat(off))}",
                     f"  loudness=-23    {f(stat(on))}",
                     f"  difference, pair by pair {f(stat(diff))}"):
            lines.append(line)
            print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
