#!/usr/bin/env python3
"""What parking a sequence costs at the 0.5B shape (GPU box):  python tools/park_time.py [--reps 5] [--out FILE]

Synthetic weights, greedy decoding.  One and eight sequences at 200, 500 and 1500 cache positions, with a contiguous and with a
paged (64-token pages) bf16 KV cache, unflagged and with a penalty plus no_repeat_ngram_size record (the two parts of a blob that
only flagged sequences pay: the penalty history row and the prompt ids):
  (a) park and resume: SparkLLM.save_slots, retire_many and restore_slots of all the sequences in one call each, every call
      timed from a drained stream to a drained stream; beside them the blob bytes, and the time a plain device copy of those
      bytes would take at the HBM copy rate measured for this part (6.29 TB/s of float4 copy traffic, read plus write: a
      save or a restore reads the bytes once and writes them once);
  (b) the only alternative without parking: retire the sequences and admit prompts of the same length again (prefill);
  (c) the admission alone at 128, 256 and 460 tokens, one sequence, the lengths of DESIGN.md section 7, measured in this run.
Every shape is warmed up once untimed; (a) and (b) alternate inside one run, rep by rep; each figure is the median of --reps
with its min .. max beside it."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "spark-tts_amd"))
COUNTS = (1, 8)
POSITIONS = (200, 500, 1500)
PREFILL_LENS = (128, 256, 460)
MAX_POS = 1536
PAGE = 64
WARM_STEPS = 8           # decode steps between the admission and the first park, so the history is not a single token
HBM_COPY_BYTES_PER_S = 6.29e12
FLAGGED = dict(repetition_penalty=1.1, no_repeat_ngram_size=4)


def stat(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def fmt(s, unit="ms"):
    return f"{s['median']:8.3f} {unit} ({s['min']:.3f} .. {s['max']:.3f})"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import build_hash
    from sparkmi import config as Cf, weights as W
    from sparkmi.llm import SparkLLM
    cfg = Cf.spark_0p5b_llm()
    syn = W.SyntheticLLM(cfg)
    rng = np.random.Generator(np.random.PCG64(5))
    sync = torch.cuda.synchronize
    head = (f"tools/park_time.py, build {build_hash()}, 0.5B shape, synthetic weights, bf16 KV, median of {a.reps} (min .. max); "
            f"copy floor = 2 x blob bytes / {HBM_COPY_BYTES_PER_S / 1e12:.2f} TB/s")
    lines, raw = [head], {"build": build_hash(), "reps": a.reps, "park": [], "admit_ms": {}}
    print(head, flush=True)

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def timed(fn):
        sync(); t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    for paged in (False, True):
        kw = dict(kv_page_tokens=PAGE, kv_pages=max(COUNTS) * MAX_POS // PAGE) if paged else {}
        llm = SparkLLM(cfg, syn, "cuda:0", max_slots=max(COUNTS), max_positions=MAX_POS, kv_dtype="bf16", **kw)
        llm.set_sampling(False)
        cache = "paged" if paged else "contiguous"
        for flagged in (False, True):
            for n in COUNTS:
                for pos in POSITIONS:
                    samp = [dict(FLAGGED) if flagged else None] * n
                    first = [rng.integers(0, cfg.vocab_size, size=pos - 1 - WARM_STEPS).tolist() for _ in range(n)]
                    again = [rng.integers(0, cfg.vocab_size, size=pos - 1).tolist() for _ in range(n)]   # the same cache length by prefill
                    llm.session_begin(None)
                    slots = llm.admit(first, samp)
                    llm.decode(WARM_STEPS)

                    def park_side(slots):
                        t_save, blobs = timed(lambda: llm.save_slots(slots))
                        t_ret, _ = timed(lambda: llm.retire_many(slots))
                        t_back, back = timed(lambda: llm.restore_slots(blobs))
                        return (t_save, t_ret, t_back), back, sum(b.numel() for b in blobs)

                    def admit_side(slots):
                        llm.retire_many(slots)
                        return timed(lambda: llm.admit(again, samp))

                    _, slots, nbytes = park_side(slots)     # warm-up, untimed
                    _, slots = admit_side(slots)
                    t = {k: [] for k in ("save", "retire", "restore", "park_total", "readmit")}
                    for _ in range(a.reps):
                        (s, r, b), slots, nbytes = park_side(slots)
                        t["save"].append(s); t["retire"].append(r); t["restore"].append(b); t["park_total"].append(s + r + b)
                        ta, slots = admit_side(slots)
                        t["readmit"].append(ta)
                    llm.retire_many(slots)
                    floor = 2 * nbytes / HBM_COPY_BYTES_PER_S * 1e3
                    st = {k: stat(v) for k, v in t.items()}
                    raw["park"].append(dict(cache=cache, flagged=flagged, n=n, positions=pos, blob_bytes=nbytes, copy_floor_ms=floor, **st))
                    say(f"(a,b) {cache:10s} {'penalty+ngram' if flagged else 'unflagged':13s} {n} x {pos:4d} positions, {nbytes / 1e6:7.2f} MB: "
                        f"save {fmt(st['save'])}  retire {fmt(st['retire'])}  restore {fmt(st['restore'])}  "
                        f"copy floor (each way) {floor:.3f} ms  |  re-admit by prefill {fmt(st['readmit'])}")
        if not paged:   # (c)
            for plen in PREFILL_LENS:
                prompt = [rng.integers(0, cfg.vocab_size, size=plen).tolist()]
                llm.session_begin(None)
                llm.retire_many(llm.admit(prompt))
                ts = []
                for _ in range(a.reps):
                    ta, s = timed(lambda: llm.admit(prompt))
                    llm.retire_many(s)
                    ts.append(ta)
                raw["admit_ms"][plen] = stat(ts)
                say(f"(c) admission of one {plen}-token prompt (contiguous): {fmt(stat(ts))}")
        llm.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n\n" + json.dumps(raw) + "\n")


if __name__ == "__main__":
    main()
