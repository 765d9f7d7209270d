"""Torch restatement of the allowed-token stage 0 of smi_llm_admit_constrained (include/sparkmi.h): every id outside the row's
set gets -inf, then penalty_ref's stages 1-3.  tests/test_constrain_cpu.py pins stage 0 to transformers'
SuppressTokensLogitsProcessor of the complement; the GPU tests use the greedy oracle below as the device path's reference."""
from __future__ import annotations

from typing import Mapping, Sequence, Tuple

import torch

from penalty_ref import history, penalize


def allow_mask(vocab: int, runs: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """bool [vocab]: True for the ids of the half-open runs [lo, hi)."""
    m = torch.zeros(vocab, dtype=torch.bool)
    for lo, hi in runs:
        m[lo:hi] = True
    return m


def constrain(logits: torch.Tensor, runs: Sequence[Tuple[int, int]]) -> torch.Tensor:
    """Stage 0 on one row [V] fp32: ids outside the runs -> -inf (a new tensor)."""
    x = logits.to(torch.float32)
    return torch.where(allow_mask(x.shape[-1], runs), x, torch.tensor(-float("inf"), dtype=torch.float32))


def process(logits: torch.Tensor, runs, hist, rec: Mapping, emitted: int, eos: Sequence[int]) -> torch.Tensor:
    """Stage 0, then stages 1-3 (penalty_ref.penalize)."""
    return penalize(constrain(logits, runs), hist, rec, emitted, eos)


def greedy_generate(ref, prompt: Sequence[int], max_new_tokens: int, runs, rec: Mapping = None, eos: Sequence[int] = (),
                    stop_at_eos: bool = True) -> list:
    """Greedy decoding through ``ref.forward`` (oracle.llm_ref.Qwen2Ref) with stage 0 and the penalties before each arg-max."""
    ref.reset()
    V = ref.cfg.vocab_size
    logits = ref.forward(prompt, last_only=True)
    out: list = []
    for _ in range(max_new_tokens):
        row = process(logits[-1], runs, history(V, prompt, out), rec or {}, len(out), eos)
        tok = int(torch.argmax(row).item())
        out.append(tok)
        if (stop_at_eos and tok in set(eos)) or len(out) == max_new_tokens:
            break
        logits = ref.forward([tok], last_only=True)
    return out
