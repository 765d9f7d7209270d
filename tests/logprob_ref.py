"""Float64 restatement of the per-token log-probabilities of smi_llm_admit_logprobs (include/sparkmi.h):
lp = z[tok] - logsumexp(z) with z = the processed logits (penalties) times 1/T when the row samples.
tests/test_logprob_cpu.py pins it to transformers' processors (tests/golden/logprob.npz); the GPU tests use it as the oracle
of the device path."""
from __future__ import annotations

from typing import Mapping, Optional, Sequence

import numpy as np
import torch

from penalty_ref import history, penalize


def log_softmax64(z, temperature: float = 0.0) -> np.ndarray:
    """float64 log_softmax of one processed row; temperature > 0: the row samples (z / T), 0: it does not."""
    x = np.asarray(z, dtype=np.float64)
    if temperature > 0:
        x = x / float(temperature)
    m = np.max(x)
    return x - (m + np.log(np.sum(np.exp(x - m))))


def logprob(z, tok: int, temperature: float = 0.0) -> float:
    return float(log_softmax64(z, temperature)[int(tok)])


def fixture_rows(golden_dir: str):
    """(name, z float32 [V], temperature (0: no sampling), ids, lp float64) per case of tests/golden/logprob.npz"""
    import os
    g = np.load(os.path.join(golden_dir, "logprob.npz"))
    for name in g["names"]:
        name = str(name)
        V, seed = int(g[f"{name}.V"]), int(g[f"{name}.seed"])
        if f"{name}.z" in g:
            z = g[f"{name}.z"]
        else:
            z = (np.random.Generator(np.random.PCG64(seed)).standard_normal(V) * 3.0).astype(np.float32)
            z[g[f"{name}.z_ids"]] = g[f"{name}.z_vals"]
        r, T = g[f"{name}.params"]
        yield name, z, float(T), g[f"{name}.ids"], g[f"{name}.lp"]


def replay(logits_rows: torch.Tensor, prompt: Sequence[int], toks: Sequence[int], rec: Optional[Mapping] = None,
           eos: Sequence[int] = (), temperature: float = 0.0) -> np.ndarray:
    """Log-probabilities of a generated sequence from teacher-forced logits: ``logits_rows`` [len(prompt) + len(toks) - 1
    or more][V] = forward_logits(prompt + toks); row len(prompt) - 1 + t scored token t.  ``rec``: the request's penalty
    keys (tests/penalty_ref.penalize, on the history before token t); ``temperature`` > 0: the row samples with it."""
    V = logits_rows.shape[1]
    rec = {k: v for k, v in (rec or {}).items() if k in ("repetition_penalty", "presence_penalty", "frequency_penalty",
                                                       "min_new_tokens", "penalize_prompt")}
    out = np.zeros(len(toks), dtype=np.float64)
    for t, tok in enumerate(toks):
        row = logits_rows[len(prompt) - 1 + t].to(torch.float32).cpu()
        if rec:
            row = penalize(row, history(V, prompt, toks[:t]), rec, t, eos)
        out[t] = logprob(row.numpy(), tok, temperature)
    return out
