#!/usr/bin/env python3
"""What a tempo costs in joined streaming (GPU box):  python tools/stream_tempo_time.py [--parent DIR] [--pairs 3] [--reps 5] [--out FILE]

Synthetic weights at the 0.5B shape in a synthetic model directory; every generated id is read as a semantic token (id mod
codebook size, as tools/stream_join_time.py does), so every side sees the same token streams.  One session of 32 rows; 1, 8 and
32 open requests of 150 tokens, first chunk 25 frames, overlap 5 (chunks of 25 and 130 frames).
  (a) serve_stream(joined=True) without tempo on this build against the same call on a built checkout of the parent commit
      (--parent DIR; left out without it): the path runs no new code.  Each side is a fresh process per run and the two
      alternate, --pairs times; a difference beyond the spread of the pairs is a regression to explain.
  (b) on this build, alternating inside one process, --reps times: joined=True without tempo and with tempo=1.25.  Per case and
      number of open requests: the time from the call to a request's first yielded audio and the call's wall time (median over
      the requests, then median (min .. max) over the runs); with the tempo also what the added launches cost per poll that had
      chunks ready -- on the device (events around StreamTempo.push on the vocoder's stream) and on the host (the call itself)
      -- and the input samples a request's first piece holds back: what it was fed less what the piece covers (its length times
      the tempo), the audio by which the first piece is shorter than without tempo.
Every case is warmed up once untimed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, TOKENS = 32, 150
OPEN = (1, 8, 32)
STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
CASES = {"no tempo": dict(), "tempo 1.25": dict(tempo=1.25)}


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.3f} {unit} ({s['min']:.3f} .. {s['max']:.3f})"


def worker(root, mode, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import audio, config as Cf, synthetic
    from sparkmi.pipeline import SparkTTS
    lcfg, vcfg = Cf.spark_0p5b_llm(), Cf.spark_0p5b_bicodec()
    with tempfile.TemporaryDirectory() as d:
        synthetic.make_model_dir(d, llm_cfg=lcfg, voc_cfg=vcfg, with_prompt_encoder=False)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=ROWS, max_positions=1024, max_frames=400)
    tts._map.usable = False
    tts._parse = lambda ids: ([int(t) % vcfg.codebook_size for t in ids], [])
    rng = np.random.Generator(np.random.PCG64(3))
    reqs = []
    for i in range(ROWS):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 100)))
        reqs.append(dict(text=f"a sentence to be spoken, number {i}", prompt_tokens=(glob, sem)))
    polls = []           # per StreamTempo.push: (start event, end event, host ms)
    fed = {}             # request -> input samples pushed into the tempo stage before its first piece left

    if hasattr(audio, "StreamTempo"):
        push = audio.StreamTempo.push

        def push_spy(self, x, rows, *a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            out = push(self, x, rows, *a, **k)
            host = (time.perf_counter() - t0) * 1e3
            e1.record()
            polls.append((e0, e1, host))
            for (key, length, _), piece in zip(rows, out[1]):
                if fed.get(key, (0, 0))[1] == 0:
                    fed[key] = (fed.get(key, (0, 0))[0] + length, piece)
            return out

        audio.StreamTempo.push = push_spy

    def run(n_open, **extra):
        polls.clear()
        fed.clear()
        first = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, w, last in tts.serve_stream(reqs[:n_open], do_sample=False, max_new_tokens=TOKENS, decode_stride=8, joined=True, **STREAM, **extra):
            if i not in first and w.size:
                first[i] = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        res = dict(first_ms=sorted(first.values())[len(first) // 2], wall_ms=wall)
        if polls:
            res.update(tempo_dev_ms=sorted(a.elapsed_time(b) for a, b, _ in polls)[len(polls) // 2],
                       tempo_host_ms=sorted(h for _, _, h in polls)[len(polls) // 2], polls=len(polls),
                       held_at_first=sorted(v[0] - v[1] * extra["tempo"] for v in fed.values())[len(fed) // 2])
        return res

    cases = CASES if mode == "cases" else {"no tempo": dict()}
    res = {f"{k} / {n}": [] for k in cases for n in OPEN}
    for n in OPEN:
        for k, extra in cases.items():
            run(n, **extra)
    for _ in range(reps):
        for n in OPEN:
            for k, extra in cases.items():
                res[f"{k} / {n}"].append(run(n, **extra))
    print("RESULT " + json.dumps(res), flush=True)


def child(root, mode, reps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", mode, "--root", root, "--reps", str(reps)],
                         check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.worker:
        worker(a.root, a.worker, a.reps)
        return
    sys.path.insert(0, HERE)
    from bench import build_hash
    head = (f"tools/stream_tempo_time.py, build {build_hash()}, 0.5B shape, synthetic weights, 1 / 8 / 32 open requests of {TOKENS} tokens on "
            f"{ROWS} rows, chunks of 25 and 130 frames, overlap 5, serve_stream(joined=True)")
    lines, raw = [head], {"build": build_hash()}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    print(head, flush=True)
    if a.parent:
        pairs = []
        for p in range(a.pairs):
            new = child(HERE, "default", a.reps)
            old = child(os.path.abspath(a.parent), "default", a.reps)
            pairs.append((new, old))
            for k in new:
                say(f"(a) pair {p}: {k:16s} first audio: this build {fmt(stat([r['first_ms'] for r in new[k]]))}   "
                    f"parent {fmt(stat([r['first_ms'] for r in old[k]]))}   wall: this build {fmt(stat([r['wall_ms'] for r in new[k]]))}   "
                    f"parent {fmt(stat([r['wall_ms'] for r in old[k]]))}")
        raw["vs_parent"] = pairs
    res = child(HERE, "cases", a.reps)
    raw["cases"] = res
    say(f"(b) {'case / open':18s} {'first audio':>36s} {'wall':>36s} {'tempo launches / poll, device':>30s} {'host':>10s} {'input held back at the first piece':>35s}")
    for k, runs in res.items():
        tail = ""
        if "tempo_dev_ms" in runs[0]:
            tail = (f" {stat([r['tempo_dev_ms'] for r in runs])['median']:27.3f} ms {stat([r['tempo_host_ms'] for r in runs])['median']:7.3f} ms"
                    f" {runs[0]['held_at_first']:27.0f} samples")
        say(f"(b) {k:18s} {fmt(stat([r['first_ms'] for r in runs])):>36s} {fmt(stat([r['wall_ms'] for r in runs])):>36s}{tail}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
