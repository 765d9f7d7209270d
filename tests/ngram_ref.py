"""A plain restatement of the no_repeat_ngram_size stage of smi_llm_admit_ngram (include/sparkmi.h), in numpy: what
transformers' NoRepeatNGramLogitsProcessor computes for one row."""
from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from penalty_ref import history, penalize


def banned_ids(ctx: Sequence[int], n: int) -> set:
    """The ids that would complete, after the context ``ctx`` (prompt + generated tokens), an n-gram ``ctx`` already holds."""
    ctx = list(ctx)
    L = len(ctx)
    if n <= 0 or L + 1 < n:
        return set()
    tail = ctx[L - n + 1:]
    return {ctx[i + n - 1] for i in range(L - n + 1) if ctx[i:i + n - 1] == tail}


def apply_ngram(logits: np.ndarray, ctx: Sequence[int], n: int) -> np.ndarray:
    """The stage on one fp32 row: -inf at every banned id, every other value as it was (a new array)."""
    out = np.array(logits, dtype=np.float32, copy=True)
    ids = sorted(banned_ids(ctx, n))
    if ids:
        out[ids] = -np.inf
    return out


def repeats(ctx: Sequence[int], n: int, start: int = 0) -> bool:
    """Some n-gram of ``ctx`` that ends at or after position ``start`` occurred before it."""
    ctx = list(ctx)
    seen = set()
    for i in range(len(ctx) - n + 1):
        g = tuple(ctx[i:i + n])
        if g in seen and i + n - 1 >= start:
            return True
        seen.add(g)
    return False


def greedy_generate(ref, prompt: Sequence[int], max_new_tokens: int, n: int, rec: Optional[Mapping] = None, margins: Optional[list] = None) -> list:
    """Greedy decoding through ``ref.forward`` (oracle.llm_ref.Qwen2Ref): the penalty stages of ``rec``, the n-gram ban, arg-max.
    ``margins``: gets top-1 minus top-2 of the processed row at every step."""
    ref.reset()
    V = ref.cfg.vocab_size
    logits = ref.forward(prompt, last_only=True)
    out: list = []
    for _ in range(max_new_tokens):
        row = logits[-1]
        if rec:
            row = penalize(row, history(V, prompt, out), rec, len(out), ())
        row = torch.from_numpy(apply_ngram(row.numpy(), list(prompt) + out, n))
        top = torch.topk(row, 2).values
        if margins is not None:
            margins.append(float(top[0] - top[1]))
        tok = int(torch.argmax(row).item())
        out.append(tok)
        if len(out) == max_new_tokens:
            break
        logits = ref.forward([tok], last_only=True)
    return out
