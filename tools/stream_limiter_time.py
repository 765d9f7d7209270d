#!/usr/bin/env python3
"""What the limiter costs in joined streaming (GPU box):  python tools/stream_limiter_time.py [--parent DIR] [--pairs 2] [--reps 5] [--out FILE]

Synthetic weights at the 0.5B shape; every side is a fresh process per run.
  (a) one push.  StreamLimiter.push of a 1 s chunk (seeded noise bursts at the model's rate, hot enough that the limiter works)
      at 1, 8 and 32 rows, device time between two events, against vocoding the same rows (detokenize_rows of 1 s of frames):
      on streams that have just begun and on streams that hold their full history (the third push).  Median (min .. max) over
      --reps pushes per process and --pairs processes.
  (b) first piece.  The time from the call to the first piece of inference_stream(joined=True) without and with
      stream_limiter="true", alternating inside one process, and the samples of that first piece: the stage holds back
      A + R + 10 = 450 samples and never waits for another chunk.  A request of 150 tokens, first chunk 25 frames, overlap 5;
      with the default scale factor the second chunk (130 frames) is the last, so both schedules are run: that one and chunks
      of 25 frames throughout.
  (c) bench.py --gpus 1 on this build against a built checkout of the parent commit (--parent DIR; left out without it),
      alternating, --pairs times: the benchmark runs no new code, so a difference is noise."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (1, 8, 32)
STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.3f} {unit} ({s['min']:.3f} .. {s['max']:.3f})"


def _timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def worker_push(root, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import audio, config as Cf, weights as W
    from sparkmi.bicodec import BiCodecVocoder
    vcfg = Cf.spark_0p5b_bicodec()
    voc = BiCodecVocoder(vcfg, W.bicodec_detok_state(vcfg), "cuda:0", max_batch=max(ROWS), max_frames=64)
    sr = 16000
    frames = sr // voc.hop
    rng = np.random.default_rng(5)
    res = {}
    for B in ROWS:
        env = np.repeat(rng.uniform(0.01, 0.6, size=(B, 3 * 10)), sr // 10, axis=1)
        x = torch.from_numpy((env * rng.standard_normal((B, 3 * sr))).astype(np.float32)).cuda()
        sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(B, frames)))
        glob = torch.from_numpy(rng.integers(0, 4096, size=(B, 1, vcfg.spk_token_num)))
        sl = audio.StreamLimiter(B, sr, sr=sr, device="cuda:0")
        fresh, late, vocode = [], [], []
        for rep in range(reps + 1):           # (the first is the warm-up)
            sl.reset()
            for b in range(B):
                sl.open(b, "true", audio.PEAK_CEILING)
            head = x[:, :sr].contiguous()
            t_first = _timed(lambda: sl.push(head, [(b, sr, False) for b in range(B)]))
            sl.push(x[:, sr: 2 * sr].contiguous(), [(b, sr, False) for b in range(B)])
            chunk = x[:, 2 * sr: 3 * sr].contiguous()
            t_late = _timed(lambda: sl.push(chunk, [(b, sr, False) for b in range(B)]))
            t_voc = _timed(lambda: voc.detokenize_rows(sem, glob, lengths=[frames] * B))
            if rep:
                fresh.append(t_first)
                late.append(t_late)
                vocode.append(t_voc)
        sl.close()
        res[str(B)] = dict(fresh=fresh, late=late, vocode=vocode)
    print("RESULT " + json.dumps(res), flush=True)


def worker_first(root, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import config as Cf, synthetic
    from sparkmi.pipeline import SparkTTS
    lcfg, vcfg = Cf.spark_0p5b_llm(), Cf.spark_0p5b_bicodec()
    with tempfile.TemporaryDirectory() as d:
        synthetic.make_model_dir(d, llm_cfg=lcfg, voc_cfg=vcfg, with_prompt_encoder=False)
        tts = SparkTTS(d, torch.device("cuda:0"), max_batch=1, max_positions=1024, max_frames=400)
    tts._map.usable = False
    tts._parse, tts._eos = (lambda ids: ([int(t) % vcfg.codebook_size for t in ids], [])), None
    rng = np.random.Generator(np.random.PCG64(3))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    sem = torch.from_numpy(rng.integers(0, vcfg.codebook_size, size=(1, 100)))

    def run(**extra):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = size = None
        pieces = 0
        for w in tts.inference_stream("a sentence to be spoken", prompt_tokens=(glob, sem), do_sample=False, max_new_tokens=150,
                                      joined=True, **dict(STREAM, **extra)):
            pieces += 1
            if first is None:
                first, size = (time.perf_counter() - t0) * 1e3, int(w.size)
        torch.cuda.synchronize()
        return dict(first_ms=first, first_samples=size, pieces=pieces, wall_ms=(time.perf_counter() - t0) * 1e3)

    even = dict(audio_chunk_size_scale_factor=1.0)     # chunks of 25 frames throughout, not 25 and then 130
    cases = {"no limiter, chunks 25 + 130": dict(), "stream_limiter, chunks 25 + 130": dict(stream_limiter="true"),
             "no limiter, chunks of 25": dict(even), "stream_limiter, chunks of 25": dict(even, stream_limiter="true")}
    res = {k: [] for k in cases}
    for k, extra in cases.items():
        run(**extra)
    for _ in range(reps):
        for k, extra in cases.items():
            res[k].append(run(**extra))
    print("RESULT " + json.dumps(res), flush=True)


def child(args, cwd=None, timeout=900):
    out = subprocess.run([sys.executable] + args, check=True, capture_output=True, text=True, timeout=timeout, cwd=cwd).stdout
    return out


def result(out):
    return json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None)
    ap.add_argument("--root", default=HERE)
    a = ap.parse_args()
    if a.worker == "push":
        return worker_push(a.root, a.reps)
    if a.worker == "first":
        return worker_first(a.root, a.reps)
    sys.path.insert(0, HERE)
    from bench import build_hash
    head = f"tools/stream_limiter_time.py, build {build_hash()}, 0.5B shape, synthetic weights, 16 kHz, A = 40, R = 400, true-peak mode"
    lines, raw = [head], {"build": build_hash()}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    print(head, flush=True)
    me = os.path.abspath(__file__)
    runs = [result(child([me, "--worker", "push", "--root", HERE, "--reps", str(a.reps)])) for _ in range(a.pairs)]
    raw["push"] = runs
    say(f"(a) {'rows':>4s} {'push of 1 s, stream begins':>36s} {'push of 1 s, full history held':>36s} {'vocoding the same rows':>36s}")
    for B in ROWS:
        col = lambda k: fmt(stat([v for r in runs for v in r[str(B)][k]]))   # noqa: E731
        say(f"(a) {B:4d} {col('fresh'):>36s} {col('late'):>36s} {col('vocode'):>36s}")
    first = result(child([me, "--worker", "first", "--root", HERE, "--reps", str(a.reps)]))
    raw["first"] = first
    for k, rs in first.items():
        say(f"(b) {k:32s} first piece after {fmt(stat([r['first_ms'] for r in rs]))}, {rs[0]['first_samples']} samples, "
            f"{rs[0]['pieces']} pieces;  the call {fmt(stat([r['wall_ms'] for r in rs]))}")
    if a.parent:
        cmd = ["bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", "1"]
        pairs = []
        for p in range(a.pairs):
            one = []
            for root in (HERE, os.path.abspath(a.parent)):
                out = child(cmd, cwd=root, timeout=1500)
                one.append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
            pairs.append(one)
            say(f"(c) pair {p}: this build {json.dumps(one[0])}")
            say(f"(c) pair {p}: parent     {json.dumps(one[1])}")
        raw["bench"] = pairs
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
