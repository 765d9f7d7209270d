"""Writes tests/golden/ngram.npz: rows of transformers' own NoRepeatNGramLogitsProcessor (CPU, fp32), alone and behind
RepetitionPenaltyLogitsProcessor.

    python tests/golden/gen_golden_ngram.py

A row's logits are NOT stored: they are ``logits_row(seed, V, holes)`` below (tests regenerate them; ``holes`` seeded ids are
-inf before the stage).  A row's context is ``context(seed, V, L, alpha)``: L ids over ``alpha`` distinct ids, so that matches are
frequent.  Stored per row r: V, seed, holes, n, the context, the chain (0: the stage alone; 1: the repetition penalty ``par``
first), ``ninf`` = the ids at which transformers' output is -inf, the arg-max (lowest id), and for V = 1003 the whole output row.
The generator itself checks that every other value of the output equals the stage's input bit for bit.
"""
from pathlib import Path

import numpy as np
import torch
from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor


def logits_row(seed: int, V: int, holes: int = 0) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(V) * 3.0).astype(np.float32)
    if holes:
        x[rng.integers(0, V, size=holes)] = -np.inf
    return x


def context(seed: int, V: int, L: int, alpha: int) -> list:
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    ids = np.concatenate([[0, V - 1], rng.choice(np.arange(1, V - 1), size=max(alpha - 2, 0), replace=False)])[:alpha]
    return ids[rng.integers(0, alpha, size=L)].astype(np.int64).tolist()


# (n, context length, alphabet, holes, chain parameter or 0)
CASES = [(1, 1, 3, 0, 0.0), (1, 37, 5, 0, 0.0), (1, 300, 40, 9, 0.0),
         (2, 1, 3, 0, 0.0), (2, 2, 2, 0, 0.0), (2, 50, 5, 0, 0.0), (2, 300, 6, 17, 0.0), (2, 120, 4, 0, 1.3),
         (3, 1, 2, 0, 0.0), (3, 2, 2, 0, 0.0), (3, 3, 1, 0, 0.0), (3, 100, 3, 0, 0.0), (3, 257, 4, 5, 0.0), (3, 90, 3, 0, 1.7),
         (4, 2, 2, 0, 0.0), (4, 3, 1, 0, 0.0), (4, 40, 2, 0, 0.0), (4, 300, 3, 0, 0.0), (4, 256, 2, 3, 1.2),
         (8, 6, 1, 0, 0.0), (8, 7, 1, 0, 0.0), (8, 64, 2, 0, 0.0), (8, 300, 2, 11, 0.0),
         (64, 30, 1, 0, 0.0), (64, 62, 1, 0, 0.0), (64, 63, 1, 0, 0.0), (64, 64, 1, 0, 0.0), (64, 300, 1, 0, 0.0), (64, 299, 2, 0, 0.0)]


def periodic(ctx: list, n: int) -> list:
    """n = 64 over two ids: a random context has no repeated 63-gram, so the context is made periodic (period 67)."""
    return [ctx[i % 67] for i in range(len(ctx))]


def main():
    data = {}
    r = 0
    for V in (1003, 166000):
        for case, (n, L, alpha, holes, par) in enumerate(CASES):
            seed = 100 + case
            ctx = context(seed, V, L, alpha)
            if n == 64 and alpha > 1:
                ctx = periodic(ctx, n)
            x = torch.from_numpy(logits_row(seed, V, holes))[None]
            ids = torch.tensor([ctx], dtype=torch.long)
            pre = RepetitionPenaltyLogitsProcessor(par)(ids, x.clone()) if par else x
            out = NoRepeatNGramLogitsProcessor(n)(ids, pre.clone())[0].numpy()
            pre = pre[0].numpy()
            ninf = np.flatnonzero(np.isneginf(out)).astype(np.int32)
            keep = np.ones(V, dtype=bool)
            keep[ninf] = False
            assert np.array_equal(out[keep].view(np.uint32), pre[keep].view(np.uint32)), "the stage moved a finite logit"
            assert not np.isneginf(out).all()
            k = f"r{r}_"
            data[k + "V"], data[k + "seed"], data[k + "holes"], data[k + "n"] = np.int32(V), np.int32(seed), np.int32(holes), np.int32(n)
            data[k + "ctx"] = np.asarray(ctx, dtype=np.int64)
            data[k + "par"] = np.float32(par)
            data[k + "ninf"] = ninf
            data[k + "argmax"] = np.int32(int(np.argmax(out)))
            if V <= 2048:
                data[k + "out"] = out
            r += 1
    data["n_rows"] = np.int32(r)
    path = Path(__file__).resolve().parent / "ngram.npz"
    np.savez_compressed(path, **data)
    print(path, path.stat().st_size, "bytes,", r, "rows")


if __name__ == "__main__":
    main()
