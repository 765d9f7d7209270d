#!/usr/bin/env python3
"""Generates ``tests/golden/penalty.npz``: what transformers' OWN logits processors make of committed logits rows, for the
per-request penalties of ``smi_llm_admit_penalized`` (include/sparkmi.h).

Stage 1 runs ``RepetitionPenaltyLogitsProcessor`` (with ``prompt_ignore_length = len(prompt)`` for penalize_prompt = 0),
stage 3 ``MinNewTokensLengthLogitsProcessor`` -- both imported, not restated.  Stage 2 (presence / frequency) has no class in
transformers; it is the additive form the header defines, ``x - (f * c + p * (c > 0))`` in fp32, c = the id's count among the
generated tokens.  ``tests/penalty_ref.py`` is the restatement the GPU tests use and ``tests/test_penalty_cpu.py`` requires
it to reproduce this file bit for bit.  Data only.

    python tests/golden/gen_golden_penalty.py

Case ``<name>``: ``logits`` (V = 1003 rows stored whole; V = 166 000 rows regenerated from ``seed``), ``prompt``,
``gen`` (the generated ids so far, in order), ``eos``, ``params`` = (r, p, f, n, penalize_prompt) and the processed row: whole
for V = 1003, as (``ids``, ``vals``) of the entries that differ from the input for V = 166 000.
"""
from __future__ import annotations

import os

import numpy as np
import torch
from transformers.generation.logits_process import MinNewTokensLengthLogitsProcessor, RepetitionPenaltyLogitsProcessor

HERE = os.path.dirname(os.path.abspath(__file__))
BIG_V = 166000


def base_row(v: int, seed: int) -> np.ndarray:
    x = (np.random.Generator(np.random.PCG64(seed)).standard_normal(v) * 2.0).astype(np.float32)
    x[::97] = 0.0   # exact zeros: x / r and x * r keep them, the additive stage moves them
    return x


def hf_process(logits: np.ndarray, prompt, gen, eos, r: float, p: float, f: float, n: int, pp: int) -> np.ndarray:
    scores = torch.from_numpy(logits.copy())[None]
    ids = torch.tensor([list(prompt) + list(gen)], dtype=torch.long)
    if r != 1.0:
        proc = RepetitionPenaltyLogitsProcessor(r, prompt_ignore_length=None if pp else len(prompt))
        scores = proc(ids, scores)
    if p != 0.0 or f != 0.0:
        c = torch.bincount(torch.tensor(list(gen), dtype=torch.long), minlength=logits.shape[0]).to(torch.float32)[None] \
            if len(gen) else torch.zeros_like(scores)
        scores = scores - (torch.tensor(f, dtype=torch.float32) * c + torch.tensor(p, dtype=torch.float32) * (c > 0).to(torch.float32))
    if n > 0:
        proc = MinNewTokensLengthLogitsProcessor(len(prompt), n, list(eos))
        scores = proc(ids, scores)
    return scores[0].numpy()


def cases():
    """(name, V, seed, prompt, gen, eos, (r, p, f, n, pp), logits override or None)"""
    eos = [7, 900]
    pr = [3, 5, 5, 11, 42, 42, 42, 600, 7, 0]         # repeated ids; 7 is an eos id; logit 0 (and 194) is an exact zero
    gn = [5, 12, 12, 12, 600, 33, 998, 194]           # 5 and 600 in both the prompt and the output
    out = [
        ("rep_prompt", 1003, 11, pr, gn, eos, (1.3, 0.0, 0.0, 0, 1)),
        ("rep_gen_only", 1003, 11, pr, gn, eos, (1.3, 0.0, 0.0, 0, 0)),
        ("rep_below_one", 1003, 12, pr, gn, eos, (0.7, 0.0, 0.0, 0, 1)),
        ("additive", 1003, 13, pr, gn, eos, (1.0, 0.5, 0.3, 0, 1)),
        ("additive_neg", 1003, 13, pr, gn, eos, (1.0, -0.75, -1.25, 0, 1)),
        ("min_below", 1003, 14, pr, gn[:3], eos, (1.0, 0.0, 0.0, 5, 1)),
        ("min_at", 1003, 14, pr, gn[:5], eos, (1.0, 0.0, 0.0, 5, 1)),
        ("min_above", 1003, 14, pr, gn + [1, 2], eos, (1.0, 0.0, 0.0, 5, 1)),
        ("min_first", 1003, 15, pr, [], eos, (1.0, 0.0, 0.0, 1, 1)),
        ("all", 1003, 16, pr, gn, eos, (1.2, 0.4, -0.2, 9, 0)),
    ]
    # the arg-max moves: the top logit is an already generated id
    top = int(np.argmax(base_row(1003, 17)))
    out.append(("argmax_moves", 1003, 17, pr, [top, top], eos, (1.5, 0.2, 0.1, 0, 1)))
    bp = [int(i) for i in np.random.Generator(np.random.PCG64(5)).integers(0, BIG_V, 300)] + [165999, 0]
    bg = [int(i) for i in np.random.Generator(np.random.PCG64(6)).integers(0, BIG_V, 120)] + [bp[3], bp[3], 165999]
    btop = int(np.argmax(base_row(BIG_V, 21)))
    big_eos = [165998, 151643]
    out += [
        ("big_all", BIG_V, 21, bp, bg + [btop], big_eos, (1.3, 0.5, 0.25, 200, 1)),
        ("big_gen_only", BIG_V, 22, bp, bg, big_eos, (0.8, -0.3, 0.6, 0, 0)),
        ("big_min", BIG_V, 23, bp, bg[:10], big_eos + [int(np.argmax(base_row(BIG_V, 23)))], (1.0, 0.0, 0.0, 11, 1)),
    ]
    return out


def main() -> None:
    data = {}
    names = []
    for name, v, seed, prompt, gen, eos, prm in cases():
        x = base_row(v, seed)
        y = hf_process(x, prompt, gen, eos, *prm)
        names.append(name)
        data[f"{name}.V"] = np.int64(v)
        data[f"{name}.seed"] = np.int64(seed)
        data[f"{name}.prompt"] = np.asarray(prompt, dtype=np.int64)
        data[f"{name}.gen"] = np.asarray(gen, dtype=np.int64)
        data[f"{name}.eos"] = np.asarray(eos, dtype=np.int64)
        data[f"{name}.params"] = np.asarray(prm, dtype=np.float64)
        if v == BIG_V:
            d = np.nonzero(x.view(np.uint32) != y.view(np.uint32))[0]
            data[f"{name}.ids"] = d.astype(np.int64)
            data[f"{name}.vals"] = y[d]
        else:
            data[f"{name}.logits"] = x
            data[f"{name}.out"] = y
        print(f"{name}: V {v}, {int((x.view(np.uint32) != y.view(np.uint32)).sum())} entries changed, "
              f"arg-max {int(np.argmax(x))} -> {int(np.argmax(y))}")
    data["names"] = np.asarray(names)
    np.savez_compressed(os.path.join(HERE, "penalty.npz"), **data)


if __name__ == "__main__":
    main()
