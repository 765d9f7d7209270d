#!/usr/bin/env python3
"""One ragged rows call against eight streams for a batch of voice prompts (GPU box):
    python tools/enc_rows_time.py [--pairs 9] [--out FILE]

xlsr-53 + the 0.5B BiCodec tokenizer, synthetic weights.  Two inputs: (a) 8 x 6 s prompts, (b) 8 ragged prompts of 2 .. 6 s; the
reference clip is the pipeline's 6 s clip (short prompts tiled).  `BiCodecEncoder.tokenize_rows` (one handle, one launch sequence
per run of equal plans, eager) is timed against `tokenize_many(lanes=8)` (eight handles on eight HIP streams, warmed, so every
lane replays its captured hipGraph).  Both are timed through their Python entry, host upload of the prompts included, from a
drained device to a drained device; the two alternate pair by pair inside one process, and the ids of the two paths are compared
on every pair.  Each figure is the median over the pairs with min .. max beside it.  `enqueue` is the host time the rows call
takes to return (all launches issued): where it is close to the whole time, the call is bound by issuing its launches, not by
the kernels."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))

INPUTS = {"8 x 6 s": (6.0,) * 8, "8 ragged 2..6 s": (2.0, 2.5, 3.1, 3.7, 4.2, 4.8, 5.4, 6.0)}


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
    from bench import build_hash
    from sparkmi import config as C, config_tok as T, weights as W
    from sparkmi.encoder import BiCodecEncoder, get_ref_clip
    wcfg, tcfg, vcfg = T.xlsr53(), T.spark_0p5b_tok(), C.spark_0p5b_bicodec()
    wsd = W.wav2vec2_state(wcfg)
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", max_seconds=6.0, ref_seconds=6.0, diag=True)
    sync = torch.cuda.synchronize
    head = (f"tools/enc_rows_time.py, build {build_hash()}, xlsr-53 + 0.5B BiCodec tokenizer, synthetic weights; ms per batch of 8 "
            f"prompts, median of {a.pairs} alternating pairs (min .. max)")
    lines = [head]
    print(head, flush=True)
    rng = np.random.default_rng(11)
    for name, secs in INPUTS.items():
        wavs = [(0.1 * rng.standard_normal(int(16000 * s))).astype(np.float32) for s in secs]
        refs = [get_ref_clip(w.astype(np.float64), 16000, 6.0, tcfg.hop_length).astype(np.float32) for w in wavs]
        for _ in range(3):                       # streams: eager, capture, replay; rows: reservation, signature cache
            enc.tokenize_many(wavs, refs, lanes=8)
            enc.tokenize_rows(wavs, refs)
            sync()
        starts, launches = enc.rows_debug_runs()
        solo_launches = []
        for lane, _ in enc._lanes[:8]:
            solo_launches.append(lane.launches())
        rows_ms, enq_ms, many_ms, equal = [], [], [], True
        for _ in range(a.pairs):
            sync()
            t0 = time.perf_counter()
            r = enc.tokenize_rows(wavs, refs)
            t1 = time.perf_counter()
            sync()
            t2 = time.perf_counter()
            m = enc.tokenize_many(wavs, refs, lanes=8)
            sync()
            t3 = time.perf_counter()
            rows_ms.append((t2 - t0) * 1e3); enq_ms.append((t1 - t0) * 1e3); many_ms.append((t3 - t2) * 1e3)
            equal = equal and all(torch.equal(g1, g2) and torch.equal(s1, s2) for (g1, s1), (g2, s2) in zip(r, m))
        diff = [x - y for x, y in zip(rows_ms, many_ms)]
        f = lambda s: f"{s[0]:8.3f} ({s[1]:.3f} .. {s[2]:.3f})"   # noqa: E731
        for line in (f"{name}: frames {[wcfg.frames(len(w)) for w in wavs]}",
                     f"  rows    {f(stat(rows_ms))}   enqueue {f(stat(enq_ms))}   runs {len(starts)} (start rows {starts}), {launches} launches",
                     f"  streams {f(stat(many_ms))}   8 graph replays of {solo_launches[0]} launches each ({sum(solo_launches)} kernel nodes)",
                     f"  rows - streams, pair by pair {f(stat(diff))}   ids equal on every pair: {equal}"):
            lines.append(line)
            print(line, flush=True)
        if not equal:
            raise SystemExit("the two paths returned different ids")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
