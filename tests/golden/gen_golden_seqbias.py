"""Writes tests/golden/seqbias.npz: rows of transformers' own SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor (CPU,
fp32), alone and chained with RepetitionPenaltyLogitsProcessor and TemperatureLogitsWarper + log_softmax.

    python tests/golden/gen_golden_seqbias.py

A row's logits are NOT stored: they are ``logits_row(seed, V)`` below (tests regenerate them).  Stored per row r: V, seed,
the context (prompt + generated ids) and the prompt length, the entries (ids padded with -1, lengths, fp32 biases, in record
order), the chain, and the expected values -- the whole row for V = 1003; for V = 166000 the values at ``probe`` (every id an
entry ends in, every context id, 64 seeded ids) and the arg-max, which is what the stage can change.
"""
from pathlib import Path

import numpy as np
import torch
from transformers.generation.logits_process import (NoBadWordsLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                    SequenceBiasLogitsProcessor, TemperatureLogitsWarper)

NINF = float("-inf")
CHAIN_NONE, CHAIN_REP, CHAIN_TEMP_LSM = 0, 1, 2


def logits_row(seed: int, V: int) -> np.ndarray:
    return (np.random.Generator(np.random.PCG64(seed)).standard_normal(V) * 3.0).astype(np.float32)


def rows_for(V: int):
    """(seed, context, prompt_len, entries, chain, chain parameter)"""
    a, b, c, d = V // 5, V // 3, V // 2, V - 7
    ctx = [a, b, c, d, 5, 9, b, c]
    out = []
    # length-1 entries, positive and negative
    out.append((1, ctx, 8, [((a,), 2.5), ((V - 1,), -3.25), ((0,), 0.125)], CHAIN_NONE, 0.0))
    # multi-token entries that match the context tail (generated tokens only), and one that does not
    out.append((2, ctx, 3, [((b, c, 11), 4.0), ((c, 12), -1.5), ((9, b, c, 13), 7.75), ((b, b, 14), 100.0)], CHAIN_NONE, 0.0))
    # entries ending in the same id, the length-1 entry listed LAST: the order of summation.  Id 21: ((0 - 1e8) + 1e8) + 1 = 1,
    # in record order (1e8 + 1) - 1e8 = 0; id 22: (1e8 - 1e8) + 1 = 1, any other order of the three gives 0.
    out.append((3, ctx, 8, [((c, 21), 1e8), ((b, c, 21), 1.0), ((21,), -1e8), ((b, c, 22), 1e8), ((c, 22), -1e8), ((9, b, c, 22), 1.0)],
                CHAIN_NONE, 0.0))
    # an entry longer than the context (ignored even though its prefix would match what there is)
    out.append((4, [b, c], 2, [((a, b, c, 31), 9.0), ((b, c, 32), 9.0), ((c, 33), 5.0)], CHAIN_NONE, 0.0))
    # an entry whose prefix lies partly in the prompt: prompt = ctx[:7], one generated token
    out.append((5, ctx, 7, [((9, b, c, 41), 6.0), ((5, 9, b, c, 42), 6.5), ((d, 5, 9, b, c, 43), -2.0)], CHAIN_NONE, 0.0))
    # -inf on the row's arg-max (length 1 and by a matching sequence), NoBadWords
    lg = logits_row(6, V)
    am = int(np.argmax(lg))
    lg2 = lg.copy(); lg2[am] = NINF
    am2 = int(np.argmax(lg2))
    out.append((6, ctx, 4, [((am,), NINF), ((c, am2), NINF), ((b, b, 51), NINF)], CHAIN_NONE, 0.0))
    # chained: repetition penalty after the bias (a biased context id: the stages do not commute)
    out.append((7, ctx, 8, [((a,), 3.0), ((c, b), -2.0), ((b, c, 61), 1.5)], CHAIN_REP, 1.3))
    # chained: temperature + log_softmax
    out.append((8, ctx, 5, [((a,), 3.0), ((c, 71), NINF), ((b, c, 72), 2.0)], CHAIN_TEMP_LSM, 0.7))
    return out


def main():
    data = {}
    r = 0
    for V in (1003, 166000):
        for seed, ctx, plen, entries, chain, par in rows_for(V):
            x = torch.from_numpy(logits_row(seed, V))[None]
            ids = torch.tensor([ctx], dtype=torch.long)
            if all(bv == NINF for _, bv in entries):
                proc = NoBadWordsLogitsProcessor([list(i) for i, _ in entries])
            else:
                proc = SequenceBiasLogitsProcessor({tuple(i): bv for i, bv in entries})
            stage = proc(ids, x.clone())
            final = stage
            if chain == CHAIN_REP:
                final = RepetitionPenaltyLogitsProcessor(par)(ids, stage.clone())
            elif chain == CHAIN_TEMP_LSM:
                final = torch.log_softmax(TemperatureLogitsWarper(par)(ids, stage.clone()), dim=-1)
            stage, final = stage[0].numpy(), final[0].numpy()
            k = f"r{r}_"
            data[k + "V"], data[k + "seed"], data[k + "plen"] = np.int32(V), np.int32(seed), np.int32(plen)
            data[k + "ctx"] = np.asarray(ctx, dtype=np.int64)
            data[k + "len"] = np.asarray([len(i) for i, _ in entries], dtype=np.int32)
            data[k + "ids"] = np.asarray([list(i) + [-1] * (8 - len(i)) for i, _ in entries], dtype=np.int32)
            data[k + "bias"] = np.asarray([bv for _, bv in entries], dtype=np.float32)
            data[k + "chain"], data[k + "par"] = np.int32(chain), np.float32(par)
            data[k + "argmax"] = np.asarray([int(np.argmax(stage)), int(np.argmax(final))], dtype=np.int32)
            if V <= 2048:
                data[k + "stage"], data[k + "final"] = stage, final
            else:
                rng = np.random.Generator(np.random.PCG64(1000 + r))
                probe = sorted(set([i[-1] for i, _ in entries]) | set(ctx) | set(rng.integers(0, V, size=64).tolist()))
                data[k + "probe"] = np.asarray(probe, dtype=np.int32)
                data[k + "stage"], data[k + "final"] = stage[probe], final[probe]
            r += 1
    data["n_rows"] = np.int32(r)
    out = Path(__file__).resolve().parent / "seqbias.npz"
    np.savez_compressed(out, **data)
    print(out, out.stat().st_size, "bytes,", r, "rows")


if __name__ == "__main__":
    main()
