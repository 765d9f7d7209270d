#!/usr/bin/env python3
"""Voice-prompt preparation on the host against the device, for a batch of 8 prompts (GPU box):
    python tools/audio_prep_time.py [--pairs 9] [--out FILE]

xlsr-53 + the 0.5B BiCodec tokenizer, synthetic weights.  Two inputs: 8 x 6 s prompts at 48 kHz, and at 44.1 kHz, as mono float64
arrays in memory (what `read_audio` hands back for a file).  Both sides run from those arrays to ids on the device, from a drained
device to a drained device:
    host    per prompt `resample_poly` (float64), `audio_volume_normalize`, `get_ref_clip` -- `load_audio`'s steps, the default
            path of `BiCodecTokenizer.tokenize_rows` -- then `BiCodecEncoder.tokenize_rows` (pack, upload, one rows call)
    device  `BiCodecEncoder.tokenize_rows_device`: one upload of the raw rows, `smi_rs_prompt_rows`, the same rows call
The two alternate pair by pair inside one process.  Each figure is the median over the pairs with min .. max beside it; `prep`
is the part before the encoder's rows call (host: the numpy / scipy steps; device: upload + `smi_rs_prompt_rows`, synchronised).
The two paths' ids are NOT compared: the device rows differ from the host's by fp32 rounding."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))

RATES = (48000, 44100)
SECONDS, PROMPTS = 6.0, 8


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
    from scipy.signal import resample_poly
    from bench import build_hash
    from sparkmi import audio, config as C, config_tok as T, weights as W
    from sparkmi.encoder import BiCodecEncoder, audio_volume_normalize, get_ref_clip
    wcfg, tcfg, vcfg = T.xlsr53(), T.spark_0p5b_tok(), C.spark_0p5b_bicodec()
    wsd = W.wav2vec2_state(wcfg)
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    enc = BiCodecEncoder(wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, "cuda:0", max_seconds=SECONDS, ref_seconds=6.0)
    sync = torch.cuda.synchronize
    hop = tcfg.hop_length
    ref_len = int(16000 * 6.0) // hop * hop

    def host_prepare(raws, sr):
        up, down = audio.ratio(sr, 16000)
        wavs = [audio_volume_normalize(resample_poly(x, up, down)) for x in raws]
        return wavs, [get_ref_clip(w, 16000, 6.0, hop) for w in wavs]

    head = (f"tools/audio_prep_time.py, build {build_hash()}, xlsr-53 + 0.5B BiCodec tokenizer, synthetic weights; ms per batch of "
            f"{PROMPTS} prompts of {SECONDS:g} s, median of {a.pairs} alternating pairs (min .. max)")
    lines = [head]
    print(head, flush=True)
    rng = np.random.default_rng(11)
    for sr in RATES:
        t = np.arange(int(sr * SECONDS)) / sr
        raws = [0.3 * np.sin(2 * np.pi * (120.0 + 15 * i) * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.0 * t)) + 0.02 * rng.standard_normal(t.size)
                for i in range(PROMPTS)]
        rates = [sr] * PROMPTS
        for _ in range(3):          # reservations, filter registration, code objects
            enc.tokenize_rows(*host_prepare(raws, sr))
            enc.tokenize_rows_device(raws, rates, ref_len)
            sync()
        host_ms, host_prep, dev_ms, dev_prep = [], [], [], []
        for _ in range(a.pairs):
            sync()
            t0 = time.perf_counter()
            wavs, refs = host_prepare(raws, sr)
            t1 = time.perf_counter()
            enc.tokenize_rows(wavs, refs)
            sync()
            t2 = time.perf_counter()
            enc.tokenize_rows_device(raws, rates, ref_len)
            sync()
            t3 = time.perf_counter()
            enc.prepare_rows_device(raws, rates, ref_len)
            sync()
            t4 = time.perf_counter()
            host_ms.append((t2 - t0) * 1e3); host_prep.append((t1 - t0) * 1e3); dev_ms.append((t3 - t2) * 1e3); dev_prep.append((t4 - t3) * 1e3)
        diff = [d - h for d, h in zip(dev_ms, host_ms)]
        f = lambda s: f"{s[0]:8.3f} ({s[1]:.3f} .. {s[2]:.3f})"   # noqa: E731
        for line in (f"{PROMPTS} x {SECONDS:g} s at {sr} Hz -> 16 kHz (up/down = {'/'.join(map(str, audio.ratio(sr, 16000)))}):",
                     f"  host    {f(stat(host_ms))}   prep {f(stat(host_prep))}   = {stat(host_prep)[0] / PROMPTS:.3f} ms a prompt",
                     f"  device  {f(stat(dev_ms))}   prep {f(stat(dev_prep))}   = {stat(dev_prep)[0] / PROMPTS:.3f} ms a prompt",
                     f"  device - host, pair by pair {f(stat(diff))}"):
            lines.append(line)
            print(line, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
