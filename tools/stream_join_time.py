#!/usr/bin/env python3
"""What joined streaming costs (GPU box):  python tools/stream_join_time.py [--parent DIR] [--pairs 3] [--reps 5] [--out FILE]

Synthetic weights at the 0.5B shape in a synthetic model directory; every generated id is read as a semantic token (id mod
codebook size, as tools/serve_stream_time.py does), so every side sees the same token streams.  One request set: 8 requests of
150 tokens through 8 rows, first chunk 25 frames, overlap 5 (chunks of 25 and 130 frames).
  (a) serve_stream with its defaults on this build against the same call on a built checkout of the parent commit (--parent DIR;
      left out without it): the path runs no new code.  Each side is a fresh process per run and the two alternate, --pairs times;
      a difference beyond the spread of the pairs is a regression to explain.
  (b) on this build, alternating inside one process, --reps times: joined=True at 16 kHz, joined=True at 24 kHz and joined=False.
      Per case: the time from the call to a request's first yielded audio and the call's wall time (median over the requests,
      then median (min .. max) over the runs), the bytes copied to the host per request and the join's launches per poll that had
      chunks ready.
Every case is warmed up once untimed."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE, TOKENS = 8, 150
STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
CASES = {"joined 16 kHz": dict(joined=True), "joined 24 kHz": dict(joined=True, output_sample_rate=24000), "joined=False": dict()}


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.2f} {unit} ({s['min']:.2f} .. {s['max']:.2f})"


def worker(root, mode, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import config as Cf, synthetic
    from sparkmi.pipeline import SparkTTS
    lcfg, vcfg = Cf.spark_0p5b_llm(), Cf.spark_0p5b_bicodec()
    with tempfile.TemporaryDirectory() as d:
        synthetic.make_model_dir(d, llm_cfg=lcfg, voc_cfg=vcfg, with_prompt_encoder=False)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=LIVE, max_positions=1024, max_frames=400)
    tts._map.usable = False
    tts._parse = lambda ids: ([int(t) % vcfg.codebook_size for t in ids], [])
    rng = np.random.Generator(np.random.PCG64(3))
    reqs = []
    for i in range(LIVE):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 100)))
        reqs.append(dict(text=f"a sentence to be spoken, number {i}", prompt_tokens=(glob, sem)))
    voc = tts.audio_tokenizer.model
    copied, jobs = [0], [0]
    detok = voc.detokenize_rows

    def spy(*a, **k):             # joined=False copies the vocoder's rows to the host as they are
        w = detok(*a, **k)
        copied[0] += w.numel() * 4
        jobs[0] += 1
        return w

    voc.detokenize_rows = spy

    def run(**extra):
        copied[0] = jobs[0] = 0
        joiner_calls = 0
        first = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, w, last in tts.serve_stream(reqs, do_sample=False, max_new_tokens=TOKENS, decode_stride=8, **STREAM, **extra):
            if i not in first and w.size:
                first[i] = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        nbytes = copied[0]
        if extra.get("joined"):
            key = [k for k in tts._joiners if (k[3], k[4]) == ((3, 2) if extra.get("output_sample_rate") else (1, 1))][0]
            j = tts._joiners[key]
            joiner_calls, nbytes = j.calls - run.seen.get(key, 0), run.pushed[0] * 4
            run.seen[key] = j.calls
        run.pushed[0] = 0
        return dict(first_ms=sorted(first.values())[len(first) // 2], wall_ms=wall, bytes_per_request=nbytes / LIVE,
                    join_launches_per_poll=joiner_calls / max(1, jobs[0]))

    run.seen, run.pushed = {}, [0]
    if mode == "cases":
        from sparkmi import audio
        push = audio.StreamJoiner.push

        def push_spy(self, x, rows):   # joined=True copies the pieces' rows
            out, lens = push(self, x, rows)
            run.pushed[0] += out.numel()
            return out, lens

        audio.StreamJoiner.push = push_spy
        res = {k: [] for k in CASES}
        for k, extra in CASES.items():
            run(**extra)
        for _ in range(reps):
            for k, extra in CASES.items():
                res[k].append(run(**extra))
    else:
        run()
        res = {"default": [run() for _ in range(reps)]}
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
    head = (f"tools/stream_join_time.py, build {build_hash()}, 0.5B shape, synthetic weights, {LIVE} requests of {TOKENS} tokens on {LIVE} rows, "
            f"chunks of 25 and 130 frames, overlap 5")
    lines, raw = [head], {"build": build_hash()}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    print(head, flush=True)
    if a.parent:
        pairs = []
        for p in range(a.pairs):
            new = child(HERE, "default", a.reps)["default"]
            old = child(os.path.abspath(a.parent), "default", a.reps)["default"]
            pairs.append((new, old))
            say(f"(a) pair {p}: serve_stream defaults, wall: this build {fmt(stat([r['wall_ms'] for r in new]))}   "
                f"parent {fmt(stat([r['wall_ms'] for r in old]))}")
            say(f"(a) pair {p}: first audio:                 this build {fmt(stat([r['first_ms'] for r in new]))}   "
                f"parent {fmt(stat([r['first_ms'] for r in old]))}")
        raw["vs_parent"] = pairs
        med = lambda side, key: [stat([r[key] for r in pr[side]])["median"] for pr in pairs]   # noqa: E731
        say(f"(a) medians of the {a.pairs} pairs, wall: this build {fmt(stat(med(0, 'wall_ms')))}   parent {fmt(stat(med(1, 'wall_ms')))}")
    res = child(HERE, "cases", a.reps)
    raw["cases"] = res
    say(f"(b) {'case':14s} {'first audio':>34s} {'wall':>34s} {'bytes to host / request':>24s} {'join launches / poll':>21s}")
    for k, runs in res.items():
        say(f"(b) {k:14s} {fmt(stat([r['first_ms'] for r in runs])):>34s} {fmt(stat([r['wall_ms'] for r in runs])):>34s} "
            f"{runs[0]['bytes_per_request']:24.0f} {runs[0]['join_launches_per_poll']:21.2f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
