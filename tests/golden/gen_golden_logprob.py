#!/usr/bin/env python3
"""Generates ``tests/golden/logprob.npz``: what transformers' OWN logits processors make of committed logits rows, for the
per-token log-probabilities of ``smi_llm_admit_logprobs`` (include/sparkmi.h).

Each case runs ``RepetitionPenaltyLogitsProcessor`` (when r != 1) in float32, as generation does, then
``TemperatureLogitsWarper`` (when the row samples) and ``torch.log_softmax`` in float64 on those scores -- all imported, not
restated -- and keeps the log-probability of a few ids, the emitted one first (float64: the reference value, free of the
float32 rounding a log_softmax over 166 000 entries would add).
A row may carry ``-inf`` entries (``min_new_tokens``' eos mask) before the processors run.  The scores z the kernel sees (the
processed logits, before the temperature) are stored too, so the GPU test feeds the kernel exactly what a step leaves in the
logits buffer.  ``tests/logprob_ref.py`` is the float64 restatement the GPU tests use; ``tests/test_logprob_cpu.py`` requires it
to reproduce this file.  Data only.

    python tests/golden/gen_golden_logprob.py

Case ``<name>``: ``V``, ``seed`` (the raw row: ``base_row(V, seed)``), ``prompt`` / ``gen`` (the ids the repetition penalty
sees), ``neg_inf`` (ids set to -inf first), ``params`` = (r, T; T = 0: the row does not sample), ``ids`` (the emitted id first),
``z`` (the processed row before the temperature, float32; stored whole for V = 1003, as the entries that differ from the raw
row for V = 166 000: ``z_ids`` / ``z_vals``) and ``lp`` (float64 log_softmax at ``ids``).
"""
from __future__ import annotations

import os

import numpy as np
import torch
from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper

HERE = os.path.dirname(os.path.abspath(__file__))
BIG_V = 166000


def base_row(v: int, seed: int) -> np.ndarray:
    return (np.random.Generator(np.random.PCG64(seed)).standard_normal(v) * 3.0).astype(np.float32)


def hf_logprobs(x: np.ndarray, prompt, gen, neg_inf, r: float, T: float):
    """-> (z: the processed float32 row before the temperature, float64 log_softmax row of the warped scores)"""
    scores = torch.from_numpy(x.copy())[None]
    if len(neg_inf):
        scores[0, torch.tensor(list(neg_inf), dtype=torch.long)] = -float("inf")
    ids = torch.tensor([list(prompt) + list(gen)], dtype=torch.long)
    if r != 1.0:
        scores = RepetitionPenaltyLogitsProcessor(r)(ids, scores)
    z = scores[0].clone()
    scores = scores.to(torch.float64)
    if T > 0:
        scores = TemperatureLogitsWarper(T)(ids, scores)
    return z.numpy(), torch.log_softmax(scores, dim=-1)[0].numpy()


def cases():
    """(name, V, seed, prompt, gen, neg_inf, (r, T), emitted id or None = the arg-max)"""
    pr = [3, 5, 5, 11, 42, 42, 600, 7, 0]
    gn = [5, 12, 12, 600, 33, 998]
    eos = [7, 900]
    out = [
        ("greedy", 1003, 31, [], [], [], (1.0, 0.0), None),
        ("rep_greedy", 1003, 32, pr, gn, [], (1.3, 0.0), None),
        ("t03", 1003, 33, [], [], [], (1.0, 0.3), 17),
        ("t08_rep", 1003, 34, pr, gn, [], (1.2, 0.8), 5),
        ("t17_eos_masked", 1003, 35, pr, gn, eos, (1.0, 1.7), 600),
        ("eos_masked_greedy", 1003, 36, [], [], eos, (1.0, 0.0), None),
    ]
    bp = [int(i) for i in np.random.Generator(np.random.PCG64(7)).integers(0, BIG_V, 200)]
    big_eos = [165998, 151643]
    out += [
        ("big_greedy", BIG_V, 41, [], [], [], (1.0, 0.0), None),
        ("big_t03", BIG_V, 42, [], [], [], (1.0, 0.3), 123456),
        ("big_t08_rep", BIG_V, 43, bp, [bp[0], bp[1]], [], (1.3, 0.8), bp[0]),
        ("big_t17_eos_masked", BIG_V, 44, bp, [], big_eos, (1.1, 1.7), 165999),
    ]
    return out


def main() -> None:
    data = {}
    names = []
    for name, v, seed, prompt, gen, neg_inf, (r, T), tok in cases():
        x = base_row(v, seed)
        z, lp = hf_logprobs(x, prompt, gen, neg_inf, r, T)
        tok = int(np.argmax(z)) if tok is None else tok
        ids = [tok] + [int(i) for i in np.random.Generator(np.random.PCG64(seed + 1000)).integers(0, v, 7)]
        ids += [int(i) for i in neg_inf]
        names.append(name)
        data[f"{name}.V"] = np.int64(v)
        data[f"{name}.seed"] = np.int64(seed)
        data[f"{name}.prompt"] = np.asarray(prompt, dtype=np.int64)
        data[f"{name}.gen"] = np.asarray(gen, dtype=np.int64)
        data[f"{name}.neg_inf"] = np.asarray(neg_inf, dtype=np.int64)
        data[f"{name}.params"] = np.asarray([r, T], dtype=np.float64)
        data[f"{name}.ids"] = np.asarray(ids, dtype=np.int64)
        data[f"{name}.lp"] = lp[ids].astype(np.float64)
        if v == BIG_V:
            d = np.nonzero(x.view(np.uint32) != z.view(np.uint32))[0]
            data[f"{name}.z_ids"] = d.astype(np.int64)
            data[f"{name}.z_vals"] = z[d]
        else:
            data[f"{name}.z"] = z
        print(f"{name}: V {v}, r {r}, T {T}, token {tok}: lp {lp[tok]:.6f}")
    data["names"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "logprob.npz"), **data)


if __name__ == "__main__":
    main()
