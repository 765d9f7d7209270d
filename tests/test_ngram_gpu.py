"""no_repeat_ngram_size (smi_llm_admit_ngram) on the device, tiny shape with vocab 1003 (and 166000 for the kernel) and past 32
rows at the 0.5B shape: the ban kernel against the transformers fixture bit for bit, the guarantee, a teacher-forced replay,
every mix of rows against its solo runs, the restricted lm_head, log-probabilities, forks, slot reuse, a mid-session admission
and the values the library refuses."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from conftest import FULL_MAX_POS
from ngram_ref import apply_ngram, repeats
from penalty_ref import history, penalize
from sparkmi import _lib, config as C, weights as W
from sparkmi.llm import ALLOW_KEY, NGRAM_KEY
from test_ngram_cpu import CHAIN_PEN, GUARANTEE_SEED, REPLAY_SEED, _bits, expected, fixture_rows, gpu_prompt, stage_input

pytestmark = pytest.mark.gpu


def _llm(cfg, syn, **kw):
    from sparkmi.llm import SparkLLM
    kw.setdefault("diag", any(k.startswith("SPARKMI_") for k in os.environ))
    return SparkLLM(cfg, syn, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def tiny():
    cfg = C.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


def _prompts(cfg, seed, n, lo=3, hi=30):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, cfg.vocab_size, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


def _same(a, b):
    if isinstance(a, tuple):
        return a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1]))
    return a == b


def _splits(L, n):
    """prompt lengths: all generated, all prompt, the seam inside the tail, the seam just before the tail, the middle"""
    return sorted({0, L, max(L - 1, 0), max(L - n // 2 - 1, 0), max(L - n + 1, 0), max(L - n, 0), L // 2, min(1, L)})


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [1003, 166000])
def test_the_kernel_reproduces_the_transformers_fixture(V):
    cfg = dataclasses.replace(C.tiny_llm(), vocab_size=V)
    rows = [r for r in fixture_rows() if r["V"] == V]
    assert len(rows) == 29
    llm = _llm(cfg, W.SyntheticLLM(cfg), max_slots=3, max_positions=320, diag=True)
    llm.session_begin()
    for r in rows:
        x, want, L = stage_input(r), expected(r), len(r["ctx"])
        for plen in (_splits(L, r["n"]) if V == 1003 else [0, L, max(L - r["n"] // 2 - 1, 0)]):
            out, tok = llm.debug_ngram(x[None], [r["n"]], [r["ctx"]], [plen])
            assert np.array_equal(_bits(out[0]), _bits(want)), f"fixture row {r['r']}, prompt of {plen}"
            assert int(tok[0]) == r["argmax"] == int(np.argmax(want))
    # three rows per call, n and the seam differing per row, one row with n = 0 (its logits stay as they were)
    for i in range(0, len(rows) - 2, 3 if V == 1003 else 9):
        trio = rows[i:i + 3]
        xs = np.stack([stage_input(r) for r in trio])
        sizes = [trio[0]["n"], 0, trio[2]["n"]]
        plens = [len(trio[0]["ctx"]) // 2, 1, max(len(trio[2]["ctx"]) - 1, 0)]
        out, tok = llm.debug_ngram(xs, sizes, [r["ctx"] for r in trio], plens)
        for m, want in enumerate([expected(trio[0]), xs[1], expected(trio[2])]):
            assert np.array_equal(_bits(out[m]), _bits(want)), (i, m)
            assert int(tok[m]) == int(np.argmax(want))
    # ties: the lowest id wins, also when the ban removes the first of the tied ids
    x = np.full((1, V), -3.0, dtype=np.float32)
    x[0, [5, 9, V - 1]] = 2.0
    out, tok = llm.debug_ngram(x, [2], [[7, 5, 7]], [1])
    assert np.isneginf(out[0, 5]) and int(tok[0]) == 9


def test_a_context_store_too_long_for_lds_is_read_in_place():
    """max_positions ids beside the tail no longer fit in 48 KiB of LDS: k_ngram_ban compares against the store and the history
    themselves.  The same fixture rows, the same bits."""
    cfg = C.tiny_llm()
    llm = _llm(cfg, W.SyntheticLLM(cfg), max_slots=3, max_positions=12288, diag=True)   # (12288 - 64 ids is the most LDS takes)
    llm.session_begin()
    rows = [r for r in fixture_rows() if r["V"] == 1003]
    for r in rows:
        x, want, L = stage_input(r), expected(r), len(r["ctx"])
        for plen in (0, L, max(L - r["n"] // 2 - 1, 0), L // 2):
            out, tok = llm.debug_ngram(x[None], [r["n"]], [r["ctx"]], [plen])
            assert np.array_equal(_bits(out[0]), _bits(want)), f"fixture row {r['r']}, prompt of {plen}"
            assert int(tok[0]) == r["argmax"]
    trio = [rows[3], rows[11], rows[20]]
    xs = np.stack([stage_input(r) for r in trio])
    out, tok = llm.debug_ngram(xs, [r["n"] for r in trio], [r["ctx"] for r in trio], [len(r["ctx"]) // 2 for r in trio])
    for m, r in enumerate(trio):
        assert np.array_equal(_bits(out[m]), _bits(expected(r))) and int(tok[m]) == r["argmax"]


# 2 -------------------------------------------------------------------------------------------------------------------
def test_no_ngram_is_emitted_twice(tiny):
    cfg, syn = tiny
    N = 96
    p = gpu_prompt(GUARANTEE_SEED, cfg)
    llm = _llm(cfg, syn, max_slots=2, max_positions=128, kv_dtype="f32")
    plain = llm.generate_ragged([p], [N])[0]
    assert repeats(p + plain, 3, len(p)), "precondition: the plain greedy run repeats a 3-gram"
    got = llm.generate_ragged([p], [N], sampling=[{NGRAM_KEY: 3}])[0]
    assert len(got) == N and not repeats(p + got, 3), "no 3-gram occurs twice in prompt + generated"
    first = next(i for i in range(N) if repeats(p + plain[:i + 1], 3, len(p)))
    assert got[:first] == plain[:first] and got[first] != plain[first], "the run changes exactly where the plain one repeats"
    one = llm.generate_ragged([p], [N], sampling=[{NGRAM_KEY: 1}])[0]
    assert len(set(one)) == N and not set(one) & set(p), "n = 1: every generated id is new to the context"
    assert llm.generate_ragged([p], [N], sampling=[{NGRAM_KEY: 0}])[0] == plain


# 3 -------------------------------------------------------------------------------------------------------------------
LP_TOL = 1e-4       # tests/test_logprob_gpu.py: session log-probabilities against log_softmax of the teacher-forced rows
LP_TOL_PEN = 2e-4   # ... and of the penalised teacher-forced rows (the repetition penalty scales the logits' own error)


def _replay(llm, cfg, p, n, pen, N=64):
    """A greedy run with no_repeat_ngram_size = n (and the penalties ``pen``) against its own teacher-forced logits behind the
    CPU restatements: (skipped arg-max checks, max |log-prob diff| over EVERY step)."""
    got, lps = llm.generate_ragged([p], [N], sampling=[dict(pen, **{NGRAM_KEY: n, "return_log_probs": True})])[0]
    assert len(got) == N and not repeats(p + got, n)
    logits = llm.forward_logits(p + got[:-1]).cpu()
    skipped, worst = 0, 0.0
    for t in range(N):
        row = logits[len(p) - 1 + t]
        if pen:
            row = penalize(row, history(cfg.vocab_size, p, got[:t]), pen, t, ())
        row = apply_ngram(row.numpy(), p + got[:t], n)
        # log-probabilities are taken after the stage: log_softmax of the processed teacher-forced row at the emitted id
        want = torch.log_softmax(torch.from_numpy(row).double(), dim=-1)[got[t]].item()
        worst = max(worst, abs(float(lps[t]) - want))
        top = np.sort(row)[-2:]
        if top[1] - top[0] < 1e-3:   # (a near tie leaves the arg-max open, not the emitted id's log-probability)
            skipped += 1
            continue
        assert int(np.argmax(row)) == got[t], f"step {t}"
    print(f"replay n={n} {pen}: {skipped} steps skipped, max |log-prob diff| {worst:.2e}")
    return skipped, worst


def test_teacher_forced_replay_and_log_probabilities(tiny):
    cfg, syn = tiny
    llm = _llm(cfg, syn, max_slots=1, max_positions=128, kv_dtype="f32")
    skipped, worst = _replay(llm, cfg, gpu_prompt(REPLAY_SEED, cfg), 2, {})
    assert skipped <= 64 // 10
    assert worst < LP_TOL


def test_the_ban_behind_the_penalties_on_the_device(tiny):
    """repetition penalty -> ban in one k_penalize pass of a session, against penalty_ref -> ngram_ref on teacher-forced logits."""
    cfg, syn = tiny
    llm = _llm(cfg, syn, max_slots=1, max_positions=128, kv_dtype="f32")
    skipped, worst = _replay(llm, cfg, gpu_prompt(REPLAY_SEED, cfg), 2, CHAIN_PEN)
    assert skipped <= 64 // 10
    assert worst < LP_TOL_PEN


# 4 -------------------------------------------------------------------------------------------------------------------
def _mix(cfg, plain):
    V = cfg.vocab_size
    samp = {"do_sample": True, "temperature": 1.1, "top_k": 40, "top_p": 0.95, "seed": 9}
    allowed = list(range(2, V - V // 8))
    recs = [{NGRAM_KEY: 1},
            {NGRAM_KEY: 2, "return_log_probs": True},
            dict(samp, **{NGRAM_KEY: 3}),
            {NGRAM_KEY: 2, "repetition_penalty": 1.3, "presence_penalty": 0.5},
            {NGRAM_KEY: 1, ALLOW_KEY: allowed, "return_log_probs": True},
            dict(samp, **{NGRAM_KEY: 64, "bad_words_ids": [[plain[0]]], "return_log_probs": True})]
    others = [None, {"repetition_penalty": 1.2}, dict(samp, seed=4), {ALLOW_KEY: allowed}, {"bad_words_ids": [[plain[1]]]}]
    return recs, others


@pytest.mark.parametrize("kv, paged", [("bf16", True), ("f32", False), ("bf16", False), ("f32", True)])
def test_rows_of_any_mix_equal_their_solo_runs(tiny, kv, paged):
    cfg, syn = tiny
    N = 96   # (long enough for the plain run to emit some id twice, so that n = 1 changes it)
    ps = _prompts(cfg, 21, 6, 5, 40)
    extra = dict(kv_page_tokens=16, kv_pages=90) if paged else {}
    llm = _llm(cfg, syn, max_slots=8, max_positions=160, kv_dtype=kv, **extra)
    plain = llm.generate_ragged([ps[0]], [N])[0]
    recs, others = _mix(cfg, plain)
    solo = [llm.generate_ragged([ps[0]], [N], sampling=[r])[0] for r in recs]
    solo_o = [llm.generate_ragged([ps[1 + i % 5]], [N], sampling=[o])[0] for i, o in enumerate(others)]
    assert solo[0] != plain and not set(solo[0]) & set(ps[0])
    for i, r in enumerate(recs):
        for j, o in enumerate(others):
            pair = llm.generate_ragged([ps[0], ps[1 + j % 5]], [N, N], sampling=[r, o])
            assert _same(pair[0], solo[i]), (i, j)
            assert _same(pair[1], solo_o[j]), (i, j)
    allrows = llm.generate_ragged([ps[0]] * 6 + [ps[1]], [N] * 7, sampling=recs + [None])
    assert all(_same(a, b) for a, b in zip(allrows[:6], solo)) and _same(allrows[6], solo_o[0])


def test_past_32_rows_at_the_0p5b_shape(full_llm):
    """44 rows (the two-pass lm_head with its 256-block partition): plain, n-gram, penalised, sampled, biased and constrained
    rows, the last two alone and beside a ban.  The plain runs of this shape repeat nothing within 10 tokens, so the biased rows
    carry a large finite bias towards one id: alone such a row emits that id at every step, with a ban it cannot."""
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(78))
    B, N, V = 44, 10, cfg.vocab_size
    ps = [rng.integers(0, 64, size=int(rng.integers(4, 24))).tolist() for _ in range(B)]
    big = SparkLLM(cfg, None, "cuda:0", max_positions=FULL_MAX_POS, arena=arena, max_slots=B, kv_dtype="f32")
    one = SparkLLM(cfg, None, "cuda:0", max_positions=FULL_MAX_POS, arena=arena, max_slots=1, kv_dtype="f32")
    plain = big.generate_ragged(ps, [N] * B)
    allowed = list(range(2, V - V // 8))
    assert len(allowed) - 1 >= FULL_MAX_POS, "the survivor rule holds for the constrained n-gram rows"
    recs = []
    for b in range(B):
        pull = [([1000 + b], 1000.0)]   # (an id of the allowed set, outside the prompts' alphabet)
        rec = [None,
               {NGRAM_KEY: 1 + b % 3},
               {NGRAM_KEY: 2, "repetition_penalty": 1.2, "return_log_probs": True},
               {NGRAM_KEY: 1, "do_sample": True, "temperature": 1.1, "top_k": 30, "top_p": 0.9, "seed": b},
               {"sequence_bias": pull},
               {ALLOW_KEY: allowed},
               {NGRAM_KEY: 1 + (b // 8) % 2, "sequence_bias": pull, "return_log_probs": True},
               {NGRAM_KEY: 1, ALLOW_KEY: allowed, "bad_words_ids": [[plain[b][0]]]}][b % 8]
        recs.append(rec)
    got = big.generate_ragged(ps, [N] * B, sampling=recs)
    acted = 0
    for b in range(B):
        if recs[b] is None:
            assert got[b] == plain[b]
            continue
        assert _same(got[b], one.generate_ragged([ps[b]], [N], sampling=[recs[b]])[0]), f"row {b}"
        toks = got[b][0] if isinstance(got[b], tuple) else got[b]
        if b % 8 == 4:
            assert toks == [1000 + b] * N
        if b % 8 in (5, 7):
            assert set(toks) <= set(allowed)
        if b % 8 == 7:
            assert plain[b][0] not in toks
        if NGRAM_KEY in recs[b]:
            assert not repeats(ps[b] + toks, recs[b][NGRAM_KEY], len(ps[b]))
        if b % 8 == 6:   # the same record without the ban emits the pulled id throughout: the stage acts at this shape
            n = recs[b][NGRAM_KEY]
            assert toks[:n] == [1000 + b] * n and toks[n] != 1000 + b
            acted += 1
    assert acted == 5


# 5 -------------------------------------------------------------------------------------------------------------------
def test_constrained_rows_on_the_restricted_lm_head(tiny):
    cfg, syn = tiny
    P, N = 128, 60
    ps = _prompts(cfg, 61, 2, 8, 20)
    allowed = list(range(300, 300 + P + 8))
    ps = [[allowed[t % len(allowed)] for t in p] for p in ps]   # prompts inside the set: the bans land inside it
    llm = _llm(cfg, syn, max_slots=3, max_positions=P)
    recs = [{NGRAM_KEY: 1, ALLOW_KEY: allowed}, {NGRAM_KEY: 2, ALLOW_KEY: allowed}]
    both = llm.generate_ragged(ps, [N, N], sampling=recs)             # every row constrained: the restricted lm_head
    for p, r, g in zip(ps, recs, both):
        assert set(g) <= set(allowed) and not repeats(p + g, r[NGRAM_KEY], len(p))
    assert len(set(both[0]) | set(ps[0])) == len(set(ps[0])) + N
    dense = llm.generate_ragged(ps + [ps[0]], [N, N, N], sampling=recs + [None])   # an unconstrained row: the whole table
    assert dense[0] == both[0] and dense[1] == both[1]


# 6 -------------------------------------------------------------------------------------------------------------------
def test_forked_takes_ban_the_ngrams_of_the_shared_prompt(tiny):
    cfg, syn = tiny
    N = 24
    ps = _prompts(cfg, 71, 2, 8, 30)
    samp = {"do_sample": True, "temperature": 1.3, "top_k": 50, "top_p": 0.95, "seed": 3, NGRAM_KEY: 3, "return_log_probs": True}
    for extra in ({}, dict(kv_page_tokens=16, kv_pages=40)):
        llm = _llm(cfg, syn, max_slots=6, max_positions=96, **extra)
        takes = llm.generate_ragged(ps, [N, N], sampling=[samp, {NGRAM_KEY: 1}], n_return=[3, 2])
        for j in range(3):
            alone = llm.generate_ragged([ps[0]], [N], sampling=[dict(samp, seed=3 + j)])[0]
            assert _same(takes[0][j], alone), j
            assert not repeats(ps[0] + takes[0][j][0], 3)
        for t in takes[1]:
            assert not set(t) & set(ps[1]) and len(set(t)) == N, "the take bans the ids of its prompt"
        expanded = llm.generate_ragged([ps[0]] * 3 + [ps[1]] * 2, [N] * 5,
                                       sampling=[dict(samp, seed=3 + j) for j in range(3)] + [{NGRAM_KEY: 1}] * 2)
        assert all(_same(a, b) for a, b in zip(takes[0] + takes[1], expanded))


# 7 -------------------------------------------------------------------------------------------------------------------
def test_slot_reuse_and_mid_session_admission(tiny):
    cfg, syn = tiny
    N = 24
    ps = _prompts(cfg, 31, 4, 8, 30)
    ps[1] = ps[1][:5]                                   # a shorter prompt for the reused slot
    llm = _llm(cfg, syn, max_slots=3, max_positions=96)
    # the former occupant's prompt holds ids the later one emits: were they still banned, its tokens would change
    ps[0] = ps[0] + llm.generate_ragged([ps[1]], [N], sampling=[{NGRAM_KEY: 1}])[0][2:14]
    solo = [llm.generate_ragged([ps[0]], [N], sampling=[{NGRAM_KEY: 1}])[0], llm.generate_ragged([ps[1]], [N], sampling=[{NGRAM_KEY: 1}])[0],
            llm.generate_ragged([ps[2]], [N])[0], llm.generate_ragged([ps[3]], [N])[0]]
    llm.session_begin()
    a = llm.admit([ps[3]])                              # a step graph without the bit
    llm.decode(5)
    b = llm.admit([ps[0]], [{NGRAM_KEY: 1}])            # an n-gram row joins while another is mid-generation
    llm.decode(9)
    assert llm.slots_tokens(b, N)[0][0] == solo[0][:10] and llm.slots_tokens(a, N)[0][0] == solo[3][:15]
    llm.retire_many(b)
    llm.decode(2)
    c = llm.admit([ps[1]], [{NGRAM_KEY: 1}])            # the slot again, a shorter prompt, with the feature
    assert c == b
    llm.decode(N - 1)
    assert llm.slots_tokens(c, N)[0][0] == solo[1], "no id of the former occupant is banned"
    llm.retire_many(c)
    d = llm.admit([ps[2]])                              # ... and without it
    assert d == c
    llm.decode(N - 1)
    assert llm.slots_tokens(d, N)[0][0] == solo[2]


# 8 -------------------------------------------------------------------------------------------------------------------
def _raw_admit(llm, prompts, ngram, allow=None):
    n, pmax = len(prompts), max(len(p) for p in prompts)
    ids = np.zeros((n, pmax), dtype=np.int64)
    for b, p in enumerate(prompts):
        ids[b, : len(p)] = p
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    ng = None if ngram is None else np.asarray(ngram, dtype=np.int32)
    slots = np.zeros(n, dtype=np.int32)
    P = ctypes.POINTER
    i32 = P(ctypes.c_int32)
    rc = llm._lib.smi_llm_admit_ngram(llm._h, ids.ctypes.data_as(P(ctypes.c_int64)), lens.ctypes.data_as(i32), n, pmax, None, None, None,
                                      None, allow, None, None if ng is None else ng.ctypes.data_as(i32), slots.ctypes.data_as(i32),
                                      llm._stream())
    return rc, slots.tolist()


@pytest.mark.parametrize("bad", ["n<0", "n=65", "small_set"])
def test_invalid_values_are_refused_and_take_nothing(tiny, bad):
    cfg, syn = tiny
    ps = _prompts(cfg, 51, 5, 5, 30)
    llm = _llm(cfg, syn, max_slots=6, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)   # unseeded rows: their streams are keyed by admission numbers

    def admit_bad(prompts):
        allow = (_lib.AllowParams * len(prompts))()
        ng = [2] * len(prompts)
        if bad == "n<0":
            ng[1] = -1
        elif bad == "n=65":
            ng[1] = 65
        else:
            allow[1].n_ranges, allow[1].lo[0], allow[1].hi[0] = 1, 100, 100 + 95   # 95 ids < max_positions = 96
        return _raw_admit(llm, prompts, ng, allow)[0]

    def run(fail):
        llm.session_begin([7])
        first = llm.admit(ps[:2], [{NGRAM_KEY: 2}, None])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            assert admit_bad(ps[2:]) == -1   # SMI_EINVAL
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        allow = (_lib.AllowParams * 3)()
        allow[1].n_ranges, allow[1].lo[0], allow[1].hi[0] = 1, 100, 100 + 96             # exactly max_positions survivors
        rc, slots = _raw_admit(llm, ps[2:], [2, 2, 0], allow)   # the slots and admission numbers the failed call left
        assert rc == 0
        llm.decode(10)
        return slots, [t for t, _ in llm.slots_tokens(first + slots, 16)]

    assert run(True) == run(False)


def test_null_and_zero_records_equal_the_biased_admission(tiny):
    cfg, syn = tiny
    ps = _prompts(cfg, 41, 3, 5, 30)
    llm = _llm(cfg, syn, max_slots=3, max_positions=96)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)
    out = []
    for ng in (None, [0, 0, 0]):
        llm.session_begin([7])
        rc, slots = _raw_admit(llm, ps, ng)
        assert rc == 0
        llm.decode(20)
        out.append((slots, llm.slots_tokens(slots, 32)))
    llm.session_begin([7])
    slots = llm.admit(ps)
    llm.decode(20)
    assert out[0] == out[1] == (slots, llm.slots_tokens(slots, 32))
