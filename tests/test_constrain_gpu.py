"""Allowed-token constraints (smi_llm_admit_constrained) at the tiny shape, vocab 1003 (scalar k_penalize path) and 166000:
greedy tokens against the masked CPU oracle, a constrained row's bits alone (restricted lm_head), beside an unconstrained
row (full lm_head + stage 0 in k_penalize) and beside rows with other sets, neutral records, sampling within the set,
log-probabilities over the set, penalties and min_new_tokens on top, forks, captured steps across admissions and
retirements that change the tile union, and records the library refuses."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from constrain_ref import allow_mask, constrain, greedy_generate
from oracle.llm_ref import Qwen2Ref
from sparkmi import _lib, config as C, weights as W
from sparkmi.llm import ALLOW_KEY

pytestmark = pytest.mark.gpu


def _llm(cfg, syn, **kw):
    from sparkmi.llm import SparkLLM
    kw.setdefault("diag", any(k.startswith("SPARKMI_") for k in os.environ))
    return SparkLLM(cfg, syn, device="cuda:0", **kw)


@pytest.fixture(scope="module", params=[1003, 166000])
def tiny(request):
    cfg = dataclasses.replace(C.tiny_llm(), vocab_size=request.param)
    return cfg, W.SyntheticLLM(cfg)


def _prompts(cfg, seed, n, lo=3, hi=30):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, cfg.vocab_size, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


def _runs(V, k):
    """Three ranges of set k (sets of different k differ, overlap in tiles, and stay clear of id 0)."""
    a = (V // 7) * (k + 1)
    return [(a, a + 23), (a + 40, a + 41), (V - 50 - 9 * k, V - 30 - 9 * k)]


def _ids(runs):
    return [i for lo, hi in runs for i in range(lo, hi)]


# 1 -------------------------------------------------------------------------------------------------------------------
def test_greedy_tokens_match_the_masked_oracle(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    prompt = _prompts(cfg, 11, 1, 10, 11)[0]
    N, runs = 24, _runs(V, 0)
    allowed = set(_ids(runs))
    llm = _llm(cfg, syn, max_slots=2, max_positions=96, kv_dtype="f32")
    got = llm.generate_ragged([prompt], [N], sampling=[{ALLOW_KEY: _ids(runs)}])[0]
    plain = llm.generate_ragged([prompt], [N])[0]
    assert len(got) == N and all(t in allowed for t in got)
    assert any(t not in allowed for t in plain), "the unconstrained run must leave the set for this test to mean anything"
    oracle = Qwen2Ref(cfg, syn, kv_dtype="f32")
    assert got == greedy_generate(oracle, prompt, N, runs)


# 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv, paged", [("bf16", True), ("f32", False)])
def test_a_constrained_row_has_the_same_bits_in_every_company(tiny, kv, paged):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 21, 4, 5, 40)
    N = 16
    extra = dict(kv_page_tokens=16, kv_pages=40) if paged else {}
    llm = _llm(cfg, syn, max_slots=4, max_positions=96, kv_dtype=kv, **extra)
    recs = [{ALLOW_KEY: _ids(_runs(V, 0)), "return_log_probs": True},
            {ALLOW_KEY: _ids(_runs(V, 0)), "return_log_probs": True, "do_sample": True, "temperature": 1.3, "top_k": 40,
             "top_p": 0.97, "seed": 9}]
    free = [None, {"do_sample": True, "temperature": 0.9, "top_k": 30, "top_p": 0.9, "seed": 4}]
    for rec in recs:
        alone = llm.generate_ragged([ps[0]], [N], sampling=[rec])[0]                    # every row constrained: restricted
        assert all(t in set(_ids(_runs(V, 0))) for t in alone[0]) and np.isfinite(alone[1]).all()
        for other in free:
            pair = llm.generate_ragged([ps[0], ps[1]], [N, N], sampling=[rec, other])   # full lm_head + stage 0
            assert pair[0][0] == alone[0] and np.array_equal(pair[0][1], alone[1])
            assert pair[1] == llm.generate_ragged([ps[1]], [N], sampling=[other])[0], "the unconstrained row keeps its bits"
        trio = llm.generate_ragged(ps[:3], [N] * 3, sampling=[rec, {ALLOW_KEY: _ids(_runs(V, 1))}, {ALLOW_KEY: _ids(_runs(V, 2))}])
        assert trio[0][0] == alone[0] and np.array_equal(trio[0][1], alone[1])
        assert all(t in set(_ids(_runs(V, k))) for k in (1, 2) for t in trio[k])


# 3 -------------------------------------------------------------------------------------------------------------------
def test_neutral_records_give_the_bits_of_no_record(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 31, 2, 5, 30)
    llm = _llm(cfg, syn, max_slots=2, max_positions=96)
    samp = {"do_sample": True, "temperature": 1.1, "top_k": 50, "top_p": 0.95, "seed": 3, "return_log_probs": True}
    for rec in (None, samp):
        base = llm.generate_ragged(ps, [12, 12], sampling=[rec, None])
        full = llm.generate_ragged(ps, [12, 12], sampling=[dict(rec or {}, **{ALLOW_KEY: range(V)}), None])
        for a, b in zip(base, full):
            if isinstance(a, tuple):
                assert a[0] == b[0] and np.array_equal(a[1], b[1])
            else:
                assert a == b


# 4 -------------------------------------------------------------------------------------------------------------------
def test_sampled_draws_follow_the_masked_distribution(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    prompt = _prompts(cfg, 41, 1, 8, 9)[0]
    runs = [(V // 3, V // 3 + 9), (V - 3, V)]                        # 12 ids: top-k = 256 and top-p = 1 never bind
    T, takes, rounds = 1.7, 64, 320                                 # 20 480 first tokens
    llm = _llm(cfg, syn, max_slots=64, max_positions=64, kv_dtype="f32")
    llm.session_begin()
    counts = np.zeros(V, dtype=np.int64)
    for r in range(rounds):
        rec = {ALLOW_KEY: _ids(runs), "do_sample": True, "temperature": T, "top_k": 256, "top_p": 1.0, "seed": 1000 + takes * r}
        slots = llm.admit([prompt], [rec], n_return=[takes])
        for t, _ in llm.slots_tokens(slots, 1):
            counts[t[0]] += 1
        llm.retire_many(slots)
    assert counts[~allow_mask(V, runs).numpy()].sum() == 0, "a draw left the set"
    row = llm.forward_logits(prompt)[-1].cpu()
    p = torch.softmax(constrain(row, runs) / T, dim=-1).double().numpy()
    tv = 0.5 * np.abs(counts / counts.sum() - p).sum()
    assert tv < 0.03, f"total variation distance {tv:.4f} over {counts.sum()} draws"


# 5 -------------------------------------------------------------------------------------------------------------------
def test_log_probabilities_are_normalised_over_the_set(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    prompt = _prompts(cfg, 51, 1, 12, 13)[0]
    N, runs = 20, _runs(V, 1)
    llm = _llm(cfg, syn, max_slots=2, max_positions=96, kv_dtype="f32")
    toks, lps = llm.generate_ragged([prompt], [N], sampling=[{ALLOW_KEY: _ids(runs), "return_log_probs": True}])[0]
    rows = llm.forward_logits(prompt + toks[:-1]).cpu()
    for t in range(N):
        z = torch.log_softmax(constrain(rows[len(prompt) - 1 + t], runs).double(), dim=-1)
        assert abs(float(lps[t]) - float(z[toks[t]])) <= 1e-4, t
        assert abs(float(torch.exp(z[allow_mask(V, runs)]).sum()) - 1.0) <= 1e-9
    assert all(float(lps[t]) > float(torch.log_softmax(rows[len(prompt) - 1 + t].double(), -1)[toks[t]]) for t in range(N)), \
        "normalised over the set, a value is above the one over the whole vocabulary"
    # a single-id set: every token is that id, with probability 1
    one = llm.generate_ragged([prompt], [6], sampling=[{ALLOW_KEY: [V - 2], "return_log_probs": True, "do_sample": True,
                                                          "temperature": 0.7, "top_k": 5, "top_p": 0.9, "seed": 1}])[0]
    assert one[0] == [V - 2] * 6 and np.abs(one[1]).max() <= 1e-6


# 6 -------------------------------------------------------------------------------------------------------------------
def test_constraints_with_penalties_and_min_new_tokens(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    prompt = _prompts(cfg, 61, 1, 12, 13)[0]
    N, runs = 24, _runs(V, 2)
    llm = _llm(cfg, syn, max_slots=2, max_positions=96, kv_dtype="f32")
    oracle = Qwen2Ref(cfg, syn, kv_dtype="f32")
    base = llm.generate_ragged([prompt], [N], sampling=[{ALLOW_KEY: _ids(runs)}])[0]
    eos = [base[1]]                                                  # a set id the constrained run emits early
    rec = dict(repetition_penalty=1.4, frequency_penalty=0.3, min_new_tokens=8)
    got = llm.generate_ragged([prompt], [N], eos, sampling=[dict(rec, **{ALLOW_KEY: _ids(runs)})])[0]
    assert got == greedy_generate(oracle, prompt, N, runs, rec, eos)
    assert eos[0] not in got[:8] and all(t in set(_ids(runs)) for t in got)
    assert got != base


# 7 -------------------------------------------------------------------------------------------------------------------
def test_forked_takes_equal_the_expanded_admission(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 71, 2, 20, 40)
    llm = _llm(cfg, syn, max_slots=6, max_positions=96, kv_page_tokens=16, kv_pages=40)
    recs = [{ALLOW_KEY: _ids(_runs(V, 0)), "do_sample": True, "temperature": 1.2, "top_k": 20, "top_p": 0.95, "seed": 5,
             "return_log_probs": True}, {ALLOW_KEY: _ids(_runs(V, 1))}]
    forked = llm.generate_ragged(ps, [10, 10], sampling=recs, n_return=[3, 2])
    flat = [ps[0]] * 3 + [ps[1]] * 2
    exp = [dict(recs[0], seed=5 + j) for j in range(3)] + [recs[1]] * 2
    want = llm.generate_ragged(flat, [10] * 5, sampling=exp)
    got = forked[0] + forked[1]
    for a, b in zip(got, want):
        if isinstance(a, tuple):
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
        else:
            assert a == b


# 8 -------------------------------------------------------------------------------------------------------------------
def test_captured_steps_follow_the_tile_union(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 81, 4, 5, 30)
    samp = {"do_sample": True, "temperature": 1.0, "top_k": 50, "top_p": 0.95, "seed": 8}

    def run(graph):
        llm = _llm(cfg, syn, max_slots=4, max_positions=128, use_graph=graph)
        llm.session_begin()
        a = llm.admit([ps[0]], [{ALLOW_KEY: _ids(_runs(V, 0))}])
        llm.decode(5)
        b = llm.admit([ps[1]], [dict(samp, **{ALLOW_KEY: _ids(_runs(V, 1))})])    # the union grows
        llm.decode(5)
        out = [llm.slots_tokens(a, 64)[0][0]]                                     # (slots are reused below)
        llm.retire(a[0])                                                          # ... and shrinks
        llm.decode(5)
        c = llm.admit([ps[2]], [None])                                            # a mixed step: full lm_head
        llm.decode(5)
        out.append(llm.slots_tokens(c, 64)[0][0])
        llm.retire_many(c)                                                        # every row constrained again
        d = llm.admit([ps[3]], [{ALLOW_KEY: _ids(_runs(V, 2))}])
        llm.decode(10)
        return out + [t for t, _ in llm.slots_tokens(b + d, 64)]

    got, want = run(True), run(False)
    assert got == want
    for toks, k in zip([got[0], got[2], got[3]], (0, 1, 2)):
        assert all(t in set(_ids(_runs(V, k))) for t in toks)


# 9 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["n17", "neg", "reserved", "lo<0", "hi>V", "empty", "overlap", "unsorted", "eos_only"])
def test_a_bad_record_fails_the_admission_and_changes_nothing(tiny, bad):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 91, 5, 5, 40)
    eos = [7]
    llm = _llm(cfg, syn, max_slots=6, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)   # unseeded rows: their streams are keyed by admission numbers

    def admit_raw(prompts):
        n, pmax = len(prompts), max(len(p) for p in prompts)
        ids = np.zeros((n, pmax), dtype=np.int64)
        for b, p in enumerate(prompts):
            ids[b, : len(p)] = p
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        allow = (_lib.AllowParams * n)()
        pens = (_lib.PenaltyParams * n)()
        for b in range(n):
            allow[b].n_ranges, allow[b].lo[0], allow[b].hi[0] = 1, 5, 60
            pens[b].repetition_penalty, pens[b].penalize_prompt = 1.0, 1
        r = allow[1]
        if bad == "n17":
            r.n_ranges = 17
        elif bad == "neg":
            r.n_ranges = -1
        elif bad == "reserved":
            r.reserved = 1
        elif bad == "lo<0":
            r.lo[0] = -1
        elif bad == "hi>V":
            r.hi[0] = V + 1
        elif bad == "empty":
            r.lo[0] = r.hi[0] = 9
        elif bad == "overlap":
            r.n_ranges, r.lo[1], r.hi[1] = 2, 59, 70
        elif bad == "unsorted":
            r.n_ranges, r.lo[1], r.hi[1] = 2, 0, 3
        elif bad == "eos_only":
            r.lo[0], r.hi[0] = 7, 8
            pens[1].min_new_tokens = 2
        slots = np.zeros(n, dtype=np.int32)
        P = ctypes.POINTER
        return llm._lib.smi_llm_admit_constrained(llm._h, ids.ctypes.data_as(P(ctypes.c_int64)), lens.ctypes.data_as(P(ctypes.c_int32)),
                                                  n, pmax, None, None, pens, None, allow, slots.ctypes.data_as(P(ctypes.c_int32)),
                                                  llm._stream())

    def run(fail):
        llm.session_begin(eos)
        first = llm.admit(ps[:2], [{ALLOW_KEY: range(5, 60)}, None])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            assert admit_raw(ps[2:]) == -1   # SMI_EINVAL
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        slots = first + llm.admit(ps[2:], [{ALLOW_KEY: range(5, 60)}] * 3)   # the slots and admission numbers the failed call left
        llm.decode(10)
        return [t for t, _ in llm.slots_tokens(slots, 16)]

    assert run(True) == run(False)
