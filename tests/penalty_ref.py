"""Torch restatement of the logits penalties of smi_llm_admit_penalized (include/sparkmi.h, stages 1-3), on the history
layout the library keeps per KV slot: uint16 [vocab], bit 15 = the id is in the prompt, bits 0..14 = its count among the
generated tokens.  tests/test_penalty_cpu.py pins it to transformers' processors (tests/golden/penalty.npz); the GPU tests use
it as the oracle of the device path."""
from __future__ import annotations

from typing import Mapping, Sequence

import numpy as np
import torch

NEUTRAL = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0, penalize_prompt=True)


def history(vocab: int, prompt: Sequence[int], gen: Sequence[int]) -> np.ndarray:
    h = np.bincount(np.asarray(list(gen), dtype=np.int64), minlength=vocab).astype(np.uint16)
    h[np.asarray(list(prompt), dtype=np.int64)] |= np.uint16(0x8000)
    return h


def penalize(logits: torch.Tensor, hist: np.ndarray, rec: Mapping, emitted: int, eos: Sequence[int]) -> torch.Tensor:
    """One row [V] fp32 -> the processed row (a new tensor)."""
    r = dict(NEUTRAL, **rec)
    x = logits.to(torch.float32).clone()
    h = torch.from_numpy(hist.astype(np.int32))
    c = h & 0x7FFF
    seen = (c > 0) | (bool(r["penalize_prompt"]) & ((h & 0x8000) != 0))
    rep = torch.tensor(float(r["repetition_penalty"]), dtype=torch.float32)
    x = torch.where(seen, torch.where(x < 0, x * rep, x / rep), x)
    f = torch.tensor(float(r["frequency_penalty"]), dtype=torch.float32)
    p = torch.tensor(float(r["presence_penalty"]), dtype=torch.float32)
    x = x - (f * c.to(torch.float32) + p * (c > 0).to(torch.float32))
    if emitted < int(r["min_new_tokens"]) and len(eos):
        x[torch.as_tensor(list(eos), dtype=torch.long)] = -float("inf")
    return x


def greedy_generate(ref, prompt: Sequence[int], max_new_tokens: int, rec: Mapping, eos: Sequence[int] = (),
                    stop_at_eos: bool = True) -> list:
    """Greedy decoding through ``ref.forward`` (oracle.llm_ref.Qwen2Ref) with the penalties before each arg-max."""
    ref.reset()
    V = ref.cfg.vocab_size
    logits = ref.forward(prompt, last_only=True)
    out: list = []
    for _ in range(max_new_tokens):
        row = penalize(logits[-1], history(V, prompt, out), rec, len(out), eos)
        tok = int(torch.argmax(row).item())
        out.append(tok)
        if (stop_at_eos and tok in set(eos)) or len(out) == max_new_tokens:
            break
        logits = ref.forward([tok], last_only=True)
    return out
