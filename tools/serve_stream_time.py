#!/usr/bin/env python3
"""What SparkTTS.serve_stream costs and buys at the 0.5B shape (GPU box):  python tools/serve_stream_time.py [--reps 5] [--out FILE]

Synthetic weights in a synthetic model directory; every generated id is read as a semantic token (id mod codebook size, as
bench.py's streaming probe does), so every path sees the same token streams whatever the random weights emit.  At 1, 8 and 32
live requests of 150 tokens (chunks: 50 frames, then the remainder):
  (a) time from the call to the first yielded chunk: serve_stream against inference_stream (one request) on this build;
  (b) host time of one poll of the live slots: SparkLLM.poll (cap = 8) against SparkLLM.slots_tokens at cap = 3000;
  (c) tokens/s over all rows: serve_stream against serve of the same requests (serve yields whole utterances);
  (d) one detokenize_rows call of 8 / 32 chunks of 50 frames against the same chunks through detokenize one by one, and as one
      detokenize batch (whose rows do not carry their solo bits).
Every shape is warmed up once untimed; the two (three) sides of a comparison alternate inside one run; each figure is the median
of --reps with its min .. max beside it."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
LIVE = (1, 8, 32)
TOKENS = 150
MAX_POS = 3072     # the history smi_llm_slots_tokens copies at cap = 3000: 3000 x 64 x 8 bytes


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.2f} {unit} ({s['min']:.2f} .. {s['max']:.2f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_hash
    from sparkmi import config as Cf, synthetic
    from sparkmi.pipeline import SparkTTS
    lcfg, vcfg = Cf.spark_0p5b_llm(), Cf.spark_0p5b_bicodec()
    with tempfile.TemporaryDirectory() as d:
        synthetic.make_model_dir(d, llm_cfg=lcfg, voc_cfg=vcfg, with_prompt_encoder=False)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=max(LIVE), max_positions=MAX_POS, max_frames=400)
    tts._map.usable = False                                             # every id is a semantic token, for every path alike
    tts._parse = lambda ids: ([int(t) % vcfg.codebook_size for t in ids], [])
    rng = np.random.Generator(np.random.PCG64(3))

    def request(i):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 100)))
        return dict(text=f"a sentence to be spoken, number {i}", prompt_tokens=(glob, sem))

    reqs = [request(i) for i in range(max(LIVE))]
    kw = dict(do_sample=False, max_new_tokens=TOKENS)
    sync = torch.cuda.synchronize
    head = f"tools/serve_stream_time.py, build {build_hash()}, 0.5B shape, synthetic weights, {TOKENS} tokens per request, median of {a.reps} (min .. max)"
    lines, raw = [head], {"build": build_hash(), "reps": a.reps}
    print(head, flush=True)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def first_chunk_stream(n):
        sync(); t0 = time.perf_counter()
        it = tts.serve_stream(reqs[:n], decode_stride=8, **kw)
        next(it)
        t = (time.perf_counter() - t0) * 1e3
        for _ in it:
            pass
        return t

    def first_chunk_single():
        r = reqs[0]
        sync(); t0 = time.perf_counter()
        it = tts.inference_stream(r["text"], prompt_tokens=r["prompt_tokens"], decode_stride=8, **kw)
        next(it)
        t = (time.perf_counter() - t0) * 1e3
        for _ in it:
            pass
        return t

    # (a)
    raw["first_chunk_ms"] = {}
    first_chunk_single()
    for n in LIVE:
        first_chunk_stream(n)
        s, o = [], []
        for _ in range(a.reps):
            s.append(first_chunk_stream(n))
            o.append(first_chunk_single())
        raw["first_chunk_ms"][n] = {"serve_stream": stat(s), "inference_stream_1": stat(o)}
        say(f"(a) first chunk, {n:2d} live: serve_stream {fmt(stat(s))}   inference_stream (1 request) {fmt(stat(o))}")

    # (b)
    raw["poll_us"] = {}
    llm = tts.model
    for n in LIVE:
        llm.session_begin(tts._eos)
        ids = [tts.tokenizer([tts.process_prompt(r["text"], None, None, r["prompt_tokens"])[0]], return_tensors="pt").input_ids[0].tolist()
               for r in reqs[:n]]
        slots = llm.admit(ids)
        llm.decode(40)
        frm = [c - 8 for c, _, _ in [(x[1], 0, 0) for x in llm.poll(slots, [0] * n, 1)]]
        llm.slots_tokens(slots, 3000)
        p, f = [], []
        for _ in range(max(a.reps, 5) * 4):
            sync(); t0 = time.perf_counter(); llm.poll(slots, frm, 8); p.append((time.perf_counter() - t0) * 1e6)
            sync(); t0 = time.perf_counter(); llm.slots_tokens(slots, 3000); f.append((time.perf_counter() - t0) * 1e6)
        llm.retire_many(slots)
        raw["poll_us"][n] = {"poll_cap8": stat(p), "slots_tokens_cap3000": stat(f)}
        say(f"(b) one poll, {n:2d} live: poll(cap 8) {fmt(stat(p), 'us')}   slots_tokens(cap 3000) {fmt(stat(f), 'us')}")

    # (c)
    raw["tokens_per_s"] = {}
    for n in LIVE:
        def run(fn):
            sync(); t0 = time.perf_counter()
            for _ in fn(reqs[:n], decode_stride=8, **kw):
                pass
            sync()
            return n * TOKENS / (time.perf_counter() - t0)
        run(tts.serve_stream); run(tts.serve)
        s, o = [], []
        for _ in range(a.reps):
            s.append(run(tts.serve_stream))
            o.append(run(tts.serve))
        raw["tokens_per_s"][n] = {"serve_stream": stat(s), "serve": stat(o)}
        say(f"(c) throughput, {n:2d} live: serve_stream {fmt(stat(s), 'tok/s')}   serve {fmt(stat(o), 'tok/s')}")

    # (d)
    raw["vocode_ms"] = {}
    voc = tts.audio_tokenizer.model
    for n in (8, 32):
        sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(n, 50))).to("cuda:0")
        glob = torch.from_numpy(rng.integers(0, 4096, size=(n, 1, vcfg.spk_token_num))).to("cuda:0")
        sides = {"detokenize_rows": lambda: voc.detokenize_rows(sem, glob, lengths=[50] * n),
                 "one_by_one": lambda: [voc.detokenize(sem[b:b + 1], glob[b:b + 1]) for b in range(n)],
                 "detokenize_batch": lambda: voc.detokenize(sem, glob, lengths=[50] * n)}
        t = {k: [] for k in sides}
        for fn in sides.values():
            fn()
        for _ in range(max(a.reps, 5) * 2):
            for k, fn in sides.items():
                sync(); t0 = time.perf_counter(); fn(); sync(); t[k].append((time.perf_counter() - t0) * 1e3)
        raw["vocode_ms"][n] = {k: stat(v) for k, v in t.items()}
        say(f"(d) {n:2d} chunks of 50 frames: detokenize_rows {fmt(stat(t['detokenize_rows']))}   one by one {fmt(stat(t['one_by_one']))}"
            f"   one detokenize batch {fmt(stat(t['detokenize_batch']))}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
