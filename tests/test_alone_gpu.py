"""A kernel-alone diagnostics call (smi_llm_debug_sample / _penalize / _logprob / _seqbias / _ngram / _head) leaves the handle
clean: whatever records, features, controls and row descriptors it installed are gone when it returns, so the generations after
it are the generations before it.  Tiny shape, greedy tokens compared with themselves.

prompts.json holds prompt STRINGS and the tiny model has no text tokenizer, so a prompt here is the UTF-8 bytes of a stored
string (ids 0 .. 255 of the 1003-id vocabulary): three of them, 166 .. 269 ids long."""
import json
import os

import numpy as np
import pytest

from sparkmi import config as C, weights as W

pytestmark = pytest.mark.gpu

N = 16          # tokens per generation
CASES = (0, 19, 30)   # a control prompt of each gender (173 and 166 bytes) and the longer clone prompt (269 bytes)


def _golden_prompts(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "prompts.json")))["cases"]
    return [list(cases[i]["expect"].encode("utf-8")) for i in CASES]


def _generations(llm, prompts):
    """(the batch generated greedily, the first prompt admitted alone, without records, into a fresh session)"""
    batch = llm.generate_ids(prompts, N)
    llm.session_begin()
    slots = llm.admit(prompts[:1])
    llm.decode(N - 1)
    (toks, _), = llm.slots_tokens(slots, N)
    return batch, list(toks)


def _every_diagnostic_once(llm, cfg, M, rng):
    V = cfg.vocab_size
    x = rng.standard_normal((M, V)).astype(np.float32) * 3
    ctxs = [rng.integers(0, V, size=7 + 2 * m).tolist() for m in range(M)]
    assert llm.debug_sample(x[0], M, seed=11 + M).shape == (M,)
    assert llm.debug_sample(None, M, seed=12, use_bound=False).shape == (M,)
    hist = (rng.integers(0, 4, size=(M, V)) * (rng.random((M, V)) < 0.05)).astype(np.uint16)
    out, am = llm.debug_penalize(x, hist, [{"repetition_penalty": 1.3, "presence_penalty": 0.2, "min_new_tokens": 2}] * M, [1] * M)
    assert out.shape == (M, V) and am.shape == (M,)
    assert np.isfinite(llm.debug_logprob(x, [0.7] * M, [3 + m for m in range(M)])).all()
    reqs = [{"sequence_bias": [([5], 2.0), ([ctxs[0][-1], 9], -1.5)], "stop_sequences": [[7, 8]]}] + [None] * (M - 1)
    out, tok, fin = llm.debug_seqbias(x, reqs, ctxs, [3] * M, min_new=[1] * M)
    assert out.shape == (M, V) and tok.shape == fin.shape == (M,)
    out, tok = llm.debug_ngram(x, [2] * M, ctxs, [2 + m for m in range(M)])
    assert out.shape == (M, V) and tok.shape == (M,)
    hidden = rng.standard_normal((M, cfg.hidden_size)).astype(np.float32)
    head = llm.debug_head(hidden, reads=[1] * M, allow=[[(16 + m, 90)] for m in range(M)])   # every row constrained
    assert head["form"].endswith(",RT>") and all(16 + m <= int(t) < 90 for m, t in enumerate(head["tokens"]))


def test_the_diagnostics_leave_the_handle_as_they_found_it(golden_dir):
    from sparkmi.llm import SparkLLM
    cfg = C.tiny_llm()
    prompts = _golden_prompts(golden_dir)
    llm = SparkLLM(cfg, W.SyntheticLLM(cfg), device="cuda:0", max_slots=3, max_positions=320, diag=True)
    before = _generations(llm, prompts)
    assert all(len(t) == N for t in before[0]) and len(before[1]) == N
    rng = np.random.Generator(np.random.PCG64(2024))
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)
    for M in (1, 3):
        _every_diagnostic_once(llm, cfg, M, rng)
    llm.set_sampling(False)
    after = _generations(llm, prompts)
    assert after[0] == before[0], "greedy generation after the diagnostics differs from the one before"
    assert after[1] == before[1], "a prompt admitted without records into a fresh session decodes differently after the diagnostics"
