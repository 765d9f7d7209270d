#!/usr/bin/env python3
"""What inference_long buys (GPU box):  python tools/longform_time.py [--pairs 2] [--reps 3] [--out FILE]

Synthetic weights at the 0.5B shape in a synthetic model directory; every generated id is read as a semantic token (id mod
codebook size, as tools/stream_join_time.py does), so both sides see the same token streams.  One paragraph of 12 sentences,
greedy, up to 100 tokens a sentence, voice cloning with given prompt tokens.
  (a) the loop a user writes today -- ``inference()`` per sentence on a ``max_batch=1`` model, then numpy on the host: the
      reference's ``detect_speech_boundaries``, a linear fade at both edges, concatenation with pauses -- against
      ``inference_long`` on models with ``max_batch`` 1, 8 and 32.  Every side is a fresh process per run and the sides alternate,
      --pairs times; per side the wall time of a call, median (min .. max) over --reps calls after one untimed call.
  (b) the two device calls of the audio edge alone, timed with HIP events on 12 rows of 100 frames: smi_trim_rows (two launches)
      and smi_concat_rows (one launch), median (min .. max) over 50 calls."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENS = 100
PARAGRAPH = " ".join(f"This is sentence number {i + 1} of the paragraph, and it says a few words about item {i * 7 + 3}." for i in range(12))
SIDES = [("loop", 1), ("long", 1), ("long", 8), ("long", 32)]


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:9.2f} {unit} ({s['min']:.2f} .. {s['max']:.2f})"


def host_edge(rows, sr, thr, pause, fade):
    """what the loop does with its waveforms, in numpy: trim as the reference does, fade, join with pauses"""
    import numpy as np
    from numpy.lib.stride_tricks import sliding_window_view
    W = int(0.1 * sr)
    out, gap, f = [], np.zeros(int(round(pause * sr)), np.float32), int(round(fade * sr))
    for x in rows:
        if x.size >= W:
            mask = np.sqrt(np.mean(sliding_window_view(x, W)[:: W // 10] ** 2, axis=1)) >= thr
            if not mask.any():
                continue
            a = max(0, int(np.argmax(mask)) * (W // 10) - 2 * W)
            b = min(x.size, (len(mask) - 1 - int(np.argmax(mask[::-1]))) * (W // 10) + 2 * W)
            x = x[a:b].copy()
        k = min(f, x.size // 2)
        if k:
            w = (np.arange(1, k + 1) / (k + 1)).astype(np.float32)
            x[:k] *= w
            x[x.size - k:] *= w[::-1]
        out += ([gap] if out else []) + [x]
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def worker(mode, max_batch, reps):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import _lib, config as Cf, longform, synthetic
    if mode == "kernels":
        l = _lib.lib()
        rng = np.random.default_rng(0)
        B, n = 12, TOKENS * 320
        x = torch.from_numpy((0.05 * rng.standard_normal((B, n))).astype(np.float32)).cuda()
        W, s, m = longform.trim_params(16000)
        i32 = lambda v: (C.c_int32 * B)(*v)   # noqa: E731
        work = torch.empty((l.smi_trim_work_len(n, W, s, B),), dtype=torch.int32, device="cuda")
        bounds = torch.empty((B, 2), dtype=torch.int32, device="cuda")
        out = torch.empty((B * (n + 4000),), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = {"smi_trim_rows (2 launches)": lambda: l.smi_trim_rows(C.c_void_p(x.data_ptr()), n, i32([n] * B), B, W, s, 0.01, m,
                                                                       C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(bounds.data_ptr()), stream),
                 "smi_concat_rows (1 launch)": lambda: l.smi_concat_rows(C.c_void_p(x.data_ptr()), n, i32([n] * B), i32([800] * B), i32([n - 800] * B),
                                                                        i32([0] + [4000] * (B - 1)), B, 80, C.c_void_p(out.data_ptr()),
                                                                        B * (n - 1600) + 4000 * (B - 1), None, None, stream)}
        res = {}
        for name, call in calls.items():
            us = []
            for it in range(55):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                assert call() == 0, l.smi_last_error()
                b.record()
                b.synchronize()
                if it >= 5:
                    us.append(a.elapsed_time(b) * 1e3)
            res[name] = us
        print("RESULT " + json.dumps(res), flush=True)
        return
    from sparkmi.pipeline import SparkTTS
    lcfg, vcfg = Cf.spark_0p5b_llm(), Cf.spark_0p5b_bicodec()
    with tempfile.TemporaryDirectory() as d:
        synthetic.make_model_dir(d, llm_cfg=lcfg, voc_cfg=vcfg, with_prompt_encoder=False)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=max_batch, max_positions=1024, max_frames=400)
    tts._map.usable = False
    tts._parse = lambda ids: ([int(t) % vcfg.codebook_size for t in ids], [])
    rng = np.random.Generator(np.random.PCG64(3))
    voice = dict(prompt_tokens=(torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num))),
                                torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 100)))), prompt_text="a transcript")
    sentences = longform.split_text(PARAGRAPH)
    assert len(sentences) == 12

    def loop():
        rows = [tts.inference(s, do_sample=False, max_new_tokens=TOKENS, **voice) for s in sentences]
        return host_edge(rows, tts.sample_rate, 0.01, 0.25, 0.005)

    def long():
        return tts.inference_long(PARAGRAPH, do_sample=False, max_new_tokens=TOKENS, **voice)

    run = loop if mode == "loop" else long
    ms, samples = [], 0
    for it in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samples = run().size
        torch.cuda.synchronize()
        if it:
            ms.append((time.perf_counter() - t0) * 1e3)
    print("RESULT " + json.dumps({"ms": ms, "samples": samples}), flush=True)


def child(mode, max_batch, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--max-batch", str(max_batch), "--reps", str(reps)],
                         check=True, capture_output=True, text=True, timeout=600).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--max-batch", type=int, default=1)
    a = ap.parse_args()
    if a.worker:
        worker(a.worker, a.max_batch, a.reps)
        return
    sys.path.insert(0, HERE)
    from bench import build_hash
    head = (f"tools/longform_time.py, build {build_hash()}, 0.5B shape, synthetic weights, a paragraph of 12 sentences, greedy, "
            f"up to {TOKENS} tokens a sentence")
    lines, raw = [head], {"build": build_hash(), "sides": {}}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    print(head, flush=True)
    name = lambda mode, mb: "inference() loop + numpy, max_batch=1" if mode == "loop" else f"inference_long, max_batch={mb}"   # noqa: E731
    for p in range(a.pairs):
        for mode, mb in SIDES:
            r = child(mode, mb, a.reps)
            raw["sides"].setdefault(name(mode, mb), []).append(r)
            say(f"(a) round {p}: {name(mode, mb):40s} {fmt(stat(r['ms']))}   {r['samples']} samples")
    med = {k: stat([stat(r["ms"])["median"] for r in v]) for k, v in raw["sides"].items()}
    base = med[name("loop", 1)]["median"]
    for k, s in med.items():
        say(f"(a) medians of the {a.pairs} rounds: {k:40s} {fmt(s)}   {base / s['median']:.2f} x the loop's speed")
    k = child("kernels", 1, 0)
    raw["kernels"] = k
    for kname, us in k.items():
        say(f"(b) {kname:30s} {fmt(stat(us), 'us')}   12 rows of {TOKENS * 320} samples")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
