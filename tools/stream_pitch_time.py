#!/usr/bin/env python3
"""What a pitch shift costs in joined streaming (GPU box):  python tools/stream_pitch_time.py [--parent DIR] [--pairs 3] [--reps 5] [--out FILE]

Synthetic weights at the 0.5B shape in a synthetic model directory; every generated id is read as a semantic token (id mod
codebook size, as tools/stream_tempo_time.py does), so every side sees the same token streams.  One session of 32 rows; 1, 8 and
32 open requests of 150 tokens, first chunk 25 frames, overlap 5 (chunks of 25 and 130 frames).
  (a) serve_stream(joined=True) without the keyword on this build against the same call on a built checkout of the parent commit
      (--parent DIR; left out without it): the path runs no new code.  Each side is a fresh process per run and the two
      alternate, --pairs times; a difference beyond the spread of the pairs is a regression to explain.
  (b) on this build, alternating inside one process, --reps times: joined=True without the keyword and with
      stream_pitch_shift=2.  Per case and number of open requests: the time from the call to a request's first yielded audio
      and the call's wall time (median over the requests, then median (min .. max) over the runs); with the shift also what the
      stage's launches cost per poll that had chunks ready -- on the device (events around StreamPitch.push on the vocoder's
      stream) and on the host (the call itself) -- and the input samples a request's first piece holds back: what it was fed
      less what the piece covers.
  (c) the stage alone, one poll of 1 / 8 / 32 streams that each push a chunk of 130 frames into a stream that is under way, at
      +2 (28/25) and +7 (3/2) semitones: StreamPitch.push (two launches) against the composition it replaces -- StreamTempo.push
      at P / Q, then StreamJoiner(overlap 0, up, down).push of its pieces (three launches; the cut is a slice) -- device time
      between events and host time of the calls, alternating, --reps times seven polls.
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
CASES = {"no shift": dict(), "shift +2": dict(stream_pitch_shift=2)}
SHIFTS = {"+2 (28/25)": (28, 25), "+7 (3/2)": (3, 2)}
CHUNK = 130 * 320


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.3f} {unit} ({s['min']:.3f} .. {s['max']:.3f})"


def stage_alone(reps):
    """(c): {"<shift> / <B>": {"fused_dev", "two_dev", "fused_host", "two_host": [ms per poll]}}"""
    import numpy as np
    import torch
    from sparkmi import audio
    from sparkmi.streaming import pitch_plan
    frame = audio.tempo_frame(16000)
    rng = np.random.Generator(np.random.PCG64(5))
    res = {}
    for name, (rp, rq) in SHIFTS.items():
        P, Q, up, down = pitch_plan(1, 1, rp, rq)
        for B in OPEN:
            x = torch.from_numpy(rng.uniform(-0.5, 0.5, size=(B, CHUNK)).astype(np.float32)).cuda()
            sp = audio.StreamPitch(B, CHUNK, frame)
            st = audio.StreamTempo(B, CHUNK, frame)
            sj = audio.StreamJoiner(B, 4 * (st.history + CHUNK) + frame[0], 0, up, down)
            for b in range(B):
                sp.open(b, (1, 1), (rp, rq))
                st.open(b, P, Q)
            rows = [(b, CHUNK, False) for b in range(B)]

            def fused():
                sp.push(x, rows)

            def two():
                z, m = st.push(x, rows)
                sj.push(z, [(b, m[b], False) for b in range(B)])

            out = {"fused_dev": [], "two_dev": [], "fused_host": [], "two_host": []}
            for poll in range(1 + 7 * reps):          # (the first poll opens the streams' state and is not timed)
                for key, fn in (("fused", fused), ("two", two)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    t0 = time.perf_counter()
                    fn()
                    host = (time.perf_counter() - t0) * 1e3
                    e1.record()
                    torch.cuda.synchronize()
                    if poll:
                        out[key + "_dev"].append(e0.elapsed_time(e1))
                        out[key + "_host"].append(host)
            res[f"{name} / {B}"] = out
            sp.close()
            st.close()
            sj.close()
    return res


def worker(root, mode, reps):
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "spark-tts_amd"))
    import numpy as np
    import torch
    from sparkmi import audio, config as Cf, synthetic
    from sparkmi.pipeline import SparkTTS
    if mode == "stage":
        print("RESULT " + json.dumps(stage_alone(reps)), flush=True)
        return
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
    polls = []           # per StreamPitch.push: (start event, end event, host ms)
    fed = {}             # request -> input samples pushed into the pitch stage before its first piece left

    if hasattr(audio, "StreamPitch"):
        push = audio.StreamPitch.push

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

        audio.StreamPitch.push = push_spy

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
            res.update(pitch_dev_ms=sorted(a.elapsed_time(b) for a, b, _ in polls)[len(polls) // 2],
                       pitch_host_ms=sorted(h for _, _, h in polls)[len(polls) // 2], polls=len(polls),
                       held_at_first=sorted(v[0] - v[1] for v in fed.values())[len(fed) // 2])
        return res

    cases = CASES if mode == "cases" else {"no shift": dict()}
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
    head = (f"tools/stream_pitch_time.py, build {build_hash()}, 0.5B shape, synthetic weights, 1 / 8 / 32 open requests of {TOKENS} tokens on "
            f"{ROWS} rows, chunks of 25 and 130 frames, overlap 5, serve_stream(joined=True)")
    lines, raw = [head], {"build": build_hash()}

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def flush():
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")

    print(head, flush=True)
    stage = child(HERE, "stage", a.reps)
    raw["stage"] = stage
    say(f"(c) {'shift / streams':18s} {'StreamPitch.push, device':>36s} {'StreamTempo + StreamJoiner, device':>36s} {'host, fused':>36s} {'host, two':>36s}")
    for k, r in stage.items():
        say(f"(c) {k:18s} {fmt(stat(r['fused_dev'])):>36s} {fmt(stat(r['two_dev'])):>36s} {fmt(stat(r['fused_host'])):>36s} {fmt(stat(r['two_host'])):>36s}")
    flush()
    res = child(HERE, "cases", a.reps)
    raw["cases"] = res
    say(f"(b) {'case / open':18s} {'first audio':>36s} {'wall':>36s} {'pitch launches / poll, device':>30s} {'host':>10s} {'input held back at the first piece':>35s}")
    for k, runs in res.items():
        tail = ""
        if "pitch_dev_ms" in runs[0]:
            tail = (f" {stat([r['pitch_dev_ms'] for r in runs])['median']:27.3f} ms {stat([r['pitch_host_ms'] for r in runs])['median']:7.3f} ms"
                    f" {runs[0]['held_at_first']:27.0f} samples")
        say(f"(b) {k:18s} {fmt(stat([r['first_ms'] for r in runs])):>36s} {fmt(stat([r['wall_ms'] for r in runs])):>36s}{tail}")
    flush()
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
            flush()


if __name__ == "__main__":
    main()
