"""A plain restatement of the sequence-bias stage and the stop match of smi_llm_admit_biased (include/sparkmi.h), in fp32
numpy: what transformers' SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor compute for one row, and TensorRT-LLM's
stop_words_list rule on the generated tokens."""
from typing import Mapping, Sequence, Tuple

import numpy as np
import torch

from constrain_ref import constrain
from penalty_ref import history, penalize

Entry = Tuple[Sequence[int], float]


def applies(ctx: Sequence[int], ids: Sequence[int]) -> bool:
    """The entry ``ids`` applies to its last id after the context ``ctx`` (prompt + generated tokens)."""
    L = len(ids)
    if L == 1:
        return True
    if L > len(ctx):
        return False
    return list(ctx[len(ctx) - (L - 1):]) == list(ids[:-1])


def bias_totals(ctx: Sequence[int], entries: Sequence[Entry]) -> dict:
    """id -> fp32 total of the applying entries: from 0, the length-1 entry first, then the longer ones in record order."""
    tot: dict = {}
    for long_pass in (False, True):
        for ids, b in entries:
            if (len(ids) > 1) == long_pass and applies(ctx, ids):
                tot[ids[-1]] = np.float32(tot.get(ids[-1], np.float32(0.0)) + np.float32(b))
    return tot


def apply_bias(logits: np.ndarray, ctx: Sequence[int], entries: Sequence[Entry]) -> np.ndarray:
    """Stage 0b on one fp32 row: x + total at every id an applying entry ends in (a new array)."""
    out = np.array(logits, dtype=np.float32, copy=True)
    with np.errstate(invalid="ignore"):
        for i, t in bias_totals(ctx, entries).items():
            out[i] = np.float32(out[i] + t)
    return out


def stop_met(gen: Sequence[int], stops: Sequence[Sequence[int]], min_new: int = 0) -> bool:
    """``gen`` = the generated tokens, the new one included: some stop sequence equals its tail, and len(gen) >= min_new."""
    if len(gen) < min_new:
        return False
    return any(len(gen) >= len(s) and list(gen[len(gen) - len(s):]) == list(s) for s in stops)


def entries_of(rec: Mapping) -> list:
    """sequence_bias entries, then bad_words_ids as -inf: the order of the device record."""
    return [(tuple(i), float(b)) for i, b in (rec.get("sequence_bias") or [])] + \
           [(tuple(i), float("-inf")) for i in (rec.get("bad_words_ids") or [])]


def greedy_generate(ref, prompt: Sequence[int], max_new_tokens: int, rec: Mapping, eos: Sequence[int] = (), runs=None) -> list:
    """Greedy decoding through ``ref.forward`` (oracle.llm_ref.Qwen2Ref): stage 0 (``runs``), stage 0b, the penalty stages,
    arg-max; ends at an eos id or a stop sequence of ``rec``."""
    ref.reset()
    V = ref.cfg.vocab_size
    logits = ref.forward(prompt, last_only=True)
    out: list = []
    ent, stops, min_new = entries_of(rec), rec.get("stop_sequences") or [], int(rec.get("min_new_tokens", 0))
    for _ in range(max_new_tokens):
        row = logits[-1]
        if runs:
            row = constrain(row, runs)
        row = torch.from_numpy(apply_bias(row.numpy(), list(prompt) + out, ent))
        row = penalize(row, history(V, prompt, out), rec, len(out), eos)
        tok = int(torch.argmax(row).item())
        out.append(tok)
        if tok in set(eos) or stop_met(out, stops, min_new) or len(out) == max_new_tokens:
            break
        logits = ref.forward([tok], last_only=True)
    return out
