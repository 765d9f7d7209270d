"""Sequence bias, banned and stop sequences (smi_llm_admit_biased) on the device, tiny shape with vocab 1003 (scalar k_penalize
path) and 166000, and past 32 rows at the 0.5B shape: the bias stage against the transformers fixture bit for bit, greedy
sessions against the CPU oracle, banned sequences, stop sequences across decode-call boundaries and under min_new_tokens, every
mix of rows against its solo runs, slot reuse, neutral records and the records the library refuses."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

from conftest import FULL_MAX_POS
from oracle.llm_ref import Qwen2Ref
from seqbias_ref import greedy_generate, stop_met
from sparkmi import _lib, config as C, weights as W
from sparkmi.llm import ALLOW_KEY
from test_seqbias_cpu import _bits, fixture_rows, logits_row

pytestmark = pytest.mark.gpu
NINF = float("-inf")


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


def _same(a, b):
    if isinstance(a, tuple):
        return a[0] == b[0] and np.array_equal(_bits(a[1]), _bits(b[1]))
    return a == b


def _record_that_bites(llm, prompt, N):
    """A record built from the unbiased greedy run: its most frequent token banned outright, a bigram of it banned, a bias
    against another of its tokens and one in favour of an id after a bigram -- so the biased run must differ."""
    plain = llm.generate_ragged([prompt], [N])[0]
    vals, cnt = np.unique(plain, return_counts=True)
    top = int(vals[np.argmax(cnt)])
    rest = [t for t in plain if t != top]
    rec = {"bad_words_ids": [[top], [rest[1], rest[2]]],
           "sequence_bias": [((rest[4],), -6.5), ((prompt[-1], plain[0], 3), 4.0), ((rest[6], 5), 30.0), ((5, 3), 30.0)]}
    return plain, rec


# 1 -------------------------------------------------------------------------------------------------------------------
def test_debug_seqbias_reproduces_the_transformers_fixture(tiny):
    cfg, syn = tiny
    V = cfg.vocab_size
    rows = [r for r in fixture_rows() if r["V"] == V]
    assert len(rows) == 8
    llm = _llm(cfg, syn, max_slots=8, max_positions=64, diag=True)
    llm.session_begin()
    x = np.stack([logits_row(r["seed"], V) for r in rows])
    reqs = [{"sequence_bias": r["entries"]} for r in rows]
    out, tok, fin = llm.debug_seqbias(x, reqs, [r["ctx"] for r in rows], [r["plen"] for r in rows])
    for m, r in enumerate(rows):
        probe = slice(None) if r["probe"] is None else r["probe"]
        assert np.array_equal(_bits(out[m][probe]), _bits(r["stage"])), f"fixture row {r['r']}"
        keep = np.ones(V, dtype=bool)
        keep[[e[0][-1] for e in r["entries"]]] = False
        assert np.array_equal(_bits(out[m][keep]), _bits(x[m][keep]))
        assert int(tok[m]) == r["argmax"][0] and not fin[m]
    # the stop match on the same rows: the arg-max completes a sequence of the generated tokens only
    stops = []
    for m, r in enumerate(rows):
        gen = r["ctx"][r["plen"]:]
        stops.append([[int(tok[m])], (gen[-1:] + [int(tok[m])]) if gen else [int(tok[m]), 1], [1, 2, 3]])
    reqs2 = [dict(q, stop_sequences=s) for q, s in zip(reqs, stops)]
    out2, tok2, fin2 = llm.debug_seqbias(x, reqs2, [r["ctx"] for r in rows], [r["plen"] for r in rows])
    assert np.array_equal(_bits(out2), _bits(out)) and np.array_equal(tok2, tok) and fin2.all()
    # ... not a sequence that reaches back into the prompt, and not below min_new_tokens
    reqs3 = [dict(q, stop_sequences=[[r["ctx"][r["plen"] - 1]] + r["ctx"][r["plen"]:][-6:] + [int(t)]]) for q, r, t in zip(reqs, rows, tok)]
    assert not llm.debug_seqbias(x, reqs3, [r["ctx"] for r in rows], [r["plen"] for r in rows])[2].any()
    many = [len(r["ctx"]) - r["plen"] + 2 for r in rows]
    assert not llm.debug_seqbias(x, reqs2, [r["ctx"] for r in rows], [r["plen"] for r in rows], min_new=many)[2].any()
    exact = [len(r["ctx"]) - r["plen"] + 1 for r in rows]
    assert llm.debug_seqbias(x, reqs2, [r["ctx"] for r in rows], [r["plen"] for r in rows], min_new=exact)[2].all()


# 2 -------------------------------------------------------------------------------------------------------------------
def test_greedy_sessions_equal_the_cpu_oracle(tiny):
    cfg, syn = tiny
    N = 64
    prompt = _prompts(cfg, 11, 1, 10, 11)[0]
    llm = _llm(cfg, syn, max_slots=2, max_positions=96, kv_dtype="f32")
    plain, rec = _record_that_bites(llm, prompt, N)
    got = llm.generate_ragged([prompt], [N], sampling=[rec])[0]
    assert got != plain, "the record must visibly change the tokens"
    oracle = Qwen2Ref(cfg, syn, kv_dtype="f32")
    assert got == greedy_generate(oracle, prompt, N, rec)
    # with a repetition penalty behind the bias (the order is part of the contract) and an allowed set in front of it
    rec2 = dict(rec, repetition_penalty=1.4)
    assert llm.generate_ragged([prompt], [N], sampling=[rec2])[0] == greedy_generate(oracle, prompt, N, rec2)


# 3 -------------------------------------------------------------------------------------------------------------------
def test_a_banned_sequence_never_appears(tiny):
    cfg, syn = tiny
    N = 64
    prompt = _prompts(cfg, 12, 1, 10, 11)[0]
    llm = _llm(cfg, syn, max_slots=2, max_positions=96)
    plain = llm.generate_ragged([prompt], [N])[0]
    banned = [[plain[3]], [plain[5], plain[6]], [plain[8], plain[9], plain[10]], [prompt[-1], plain[0]]]
    for samp in ({}, {"do_sample": True, "temperature": 1.2, "top_k": 50, "top_p": 0.95, "seed": 3}):
        got = llm.generate_ragged([prompt], [N], sampling=[dict(samp, bad_words_ids=banned)])[0]
        ctx = prompt + got
        for b in banned:
            assert not any(ctx[i:i + len(b)] == b for i in range(len(prompt) - len(b) + 1, len(ctx))), (b, got)


# 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3])
def test_a_stop_sequence_ends_the_row_at_the_right_token(tiny, L):
    cfg, syn = tiny
    N = 40
    prompt = _prompts(cfg, 13, 1, 10, 11)[0]
    llm = _llm(cfg, syn, max_slots=2, max_positions=96)
    plain = llm.generate_ragged([prompt], [N])[0]
    stop = plain[17 - L:17]
    want = next(k for k in range(1, N + 1) if stop_met(plain[:k], [stop]))
    assert L <= want <= 17
    rec = {"stop_sequences": [[cfg.vocab_size - 1] * 4, stop]}

    def run(strides, r=rec):
        llm.session_begin()
        slot = llm.admit([prompt], [r])
        seen = []
        for s in strides:
            llm.decode(s)
            seen.append(llm.slots_tokens(slot, N)[0])
        return seen

    def expect(stops, min_new=0):   # stop sequences do not touch the logits: the plain run, cut at the first match
        k = next((k for k in range(1, N + 1) if stop_met(plain[:k], stops, min_new)), None)
        return (plain, False) if k is None else (plain[:k], True)

    for strides in ([N - 1], [1] * (N - 1), [want - 1, N - want], [max(want - 2, 0), 5, 20], [7] * 5):
        seen = run(strides)
        toks, fin = seen[-1]
        assert toks == plain[:want] and fin, (strides, toks)
        for k, (t, f) in enumerate(seen):   # finished exactly from the call that emits the last token of the sequence
            assert f == (1 + sum(strides[:k + 1]) >= want) and t == plain[:min(want, 1 + sum(strides[:k + 1]))]
    # a sequence that starts in the prompt does not stop the row at its first token: generated tokens only
    straddle = [prompt[-L:] + plain[:1]]
    assert run([N - 1], {"stop_sequences": straddle})[-1] == expect(straddle) and expect(straddle)[0][:1] != plain[:0]
    assert len(expect(straddle)[0]) > 1
    # ignored below min_new_tokens: the row runs on to the next match at or after it (or to the budget)
    assert run([N - 1], dict(rec, min_new_tokens=want + 1))[-1] == expect([stop], want + 1)
    assert len(expect([stop], want + 1)[0]) > want
    assert run([N - 1], dict(rec, min_new_tokens=want))[-1] == (plain[:want], True)


# 5 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv, paged", [("bf16", True), ("f32", False)])
def test_rows_of_any_mix_equal_their_solo_runs(tiny, kv, paged):
    cfg, syn = tiny
    V, N = cfg.vocab_size, 20
    ps = _prompts(cfg, 21, 6, 5, 40)
    extra = dict(kv_page_tokens=16, kv_pages=60) if paged else {}
    llm = _llm(cfg, syn, max_slots=8, max_positions=96, kv_dtype=kv, **extra)
    plain, rec = _record_that_bites(llm, ps[0], N)
    samp = {"do_sample": True, "temperature": 1.1, "top_k": 40, "top_p": 0.95, "seed": 9}
    allowed = list(range(2, V - V // 4))
    recs = [rec,                                                            # greedy, biased
            dict(rec, **samp),                                              # sampled
            dict(rec, repetition_penalty=1.3, presence_penalty=0.5),        # penalised
            dict(rec, return_log_probs=True),                               # with log-probabilities
            dict(rec, **{ALLOW_KEY: allowed}),                              # constrained
            dict(rec, **samp, return_log_probs=True, stop_sequences=[plain[7:9]], **{ALLOW_KEY: allowed})]
    others = [None, {"repetition_penalty": 1.2}, dict(samp, seed=4), {ALLOW_KEY: allowed}, {"stop_sequences": [[plain[4]]]}]
    solo = [llm.generate_ragged([ps[0]], [N], sampling=[r])[0] for r in recs]
    solo_o = [llm.generate_ragged([ps[1 + i % 5]], [N], sampling=[o])[0] for i, o in enumerate(others)]
    assert solo[0] != plain
    for i, r in enumerate(recs):
        for j, o in enumerate(others):
            pair = llm.generate_ragged([ps[0], ps[1 + j % 5]], [N, N], sampling=[r, o])
            assert _same(pair[0], solo[i]), (i, j)
            assert _same(pair[1], solo_o[j]), (i, j)
    # every constrained row on the restricted lm_head, with and without bias records
    both = llm.generate_ragged([ps[0], ps[0]], [N, N], sampling=[recs[4], recs[5]])
    assert _same(both[0], solo[4]) and _same(both[1], solo[5])
    # all at once, and forked takes
    allrows = llm.generate_ragged([ps[0]] * 6 + [ps[1]], [N] * 7, sampling=recs + [None])
    assert all(_same(a, b) for a, b in zip(allrows[:6], solo)) and _same(allrows[6], solo_o[0])
    takes = llm.generate_ragged([ps[0], ps[1]], [N, N], sampling=[recs[5], None], n_return=[3, 2])
    assert _same(takes[0][0], solo[5]) and takes[1][0] == solo_o[0] and takes[1][1] == solo_o[0]
    for j in (1, 2):
        alone = llm.generate_ragged([ps[0]], [N], sampling=[dict(recs[5], seed=9 + j)])[0]
        assert _same(takes[0][j], alone)


# 6 -------------------------------------------------------------------------------------------------------------------
def test_mid_session_admission_and_slot_reuse(tiny):
    cfg, syn = tiny
    N = 24
    ps = _prompts(cfg, 31, 3, 8, 30)
    llm = _llm(cfg, syn, max_slots=3, max_positions=96)
    plain0, rec = _record_that_bites(llm, ps[0], N)
    rec = dict(rec, stop_sequences=[[cfg.vocab_size - 2]])
    solo = [llm.generate_ragged([ps[0]], [N], sampling=[rec])[0], llm.generate_ragged([ps[1]], [N])[0],
            llm.generate_ragged([ps[2]], [N])[0]]
    llm.session_begin()
    a = llm.admit([ps[1]])                      # a step graph without the bits
    llm.decode(5)
    b = llm.admit([ps[0]], [rec])               # a biased row joins: the bits change mid-session
    llm.decode(9)
    assert llm.slots_tokens(b, N)[0][0] == solo[0][:10] and llm.slots_tokens(a, N)[0][0] == solo[1][:15]
    llm.retire_many(b)                          # the record's slot is free again ...
    llm.decode(3)
    c = llm.admit([ps[0]])                      # ... and reused WITHOUT a record: neither record nor prompt tail is inherited
    assert c == b
    llm.decode(N - 1)
    assert llm.slots_tokens(c, N)[0][0] == plain0
    assert llm.slots_tokens(a, N)[0][0][:N] == solo[1]
    llm.retire_many(c)
    d = llm.admit([ps[2]], [{"stop_sequences": [[cfg.vocab_size - 2]]}])   # reused with a record that never fires
    llm.decode(N - 1)
    assert d == c and llm.slots_tokens(d, N)[0] == (solo[2], False)


# 7 -------------------------------------------------------------------------------------------------------------------
def _raw_admit(llm, prompts, seq=None, allow=None, pens=None, entry="smi_llm_admit_biased"):
    n, pmax = len(prompts), max(len(p) for p in prompts)
    ids = np.zeros((n, pmax), dtype=np.int64)
    for b, p in enumerate(prompts):
        ids[b, : len(p)] = p
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    slots = np.zeros(n, dtype=np.int32)
    P = ctypes.POINTER
    args = [llm._h, ids.ctypes.data_as(P(ctypes.c_int64)), lens.ctypes.data_as(P(ctypes.c_int32)), n, pmax, None, None, pens, None, allow]
    if entry == "smi_llm_admit_biased":
        args.append(seq)
    rc = getattr(llm._lib, entry)(*args, slots.ctypes.data_as(P(ctypes.c_int32)), llm._stream())
    return rc, slots.tolist()


def test_neutral_records_equal_the_constrained_admission(tiny):
    cfg, syn = tiny
    ps = _prompts(cfg, 41, 3, 5, 30)
    llm = _llm(cfg, syn, max_slots=3, max_positions=96)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)
    out = []
    for entry, seq in (("smi_llm_admit_constrained", None), ("smi_llm_admit_biased", (_lib.SeqParams * 3)()), ("smi_llm_admit_biased", None)):
        llm.session_begin([7])
        rc, slots = _raw_admit(llm, ps, seq=seq, entry=entry)
        assert rc == 0
        llm.decode(20)
        out.append((slots, llm.slots_tokens(slots, 32)))
    assert out[0] == out[1] == out[2]


# 8 -------------------------------------------------------------------------------------------------------------------
BAD = ["n_bias33", "n_bias<0", "n_stop9", "n_stop<0", "reserved", "len0", "len9", "id<0", "id=V", "nan", "+inf", "dup", "slen0",
       "slen9", "sid=V", "sdup", "no_survivor", "no_survivor_allow", "eos_only"]


@pytest.mark.parametrize("bad", BAD)
def test_invalid_records_are_refused_and_take_nothing(tiny, bad):
    cfg, syn = tiny
    V = cfg.vocab_size
    ps = _prompts(cfg, 51, 5, 5, 30)
    llm = _llm(cfg, syn, max_slots=6, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)   # unseeded rows: their streams are keyed by admission numbers
    L = _lib.SMI_MAX_SEQ_LEN

    def records(n):
        seq, allow, pens = (_lib.SeqParams * n)(), (_lib.AllowParams * n)(), (_lib.PenaltyParams * n)()
        for b in range(n):
            q = seq[b]
            q.n_bias, q.n_stop = 2, 2
            q.bias_len[0], q.bias[0], q.bias_ids[0], q.bias_ids[1] = 2, 1.5, 3, 4
            q.bias_len[1], q.bias[1], q.bias_ids[L] = 1, NINF, 9
            q.stop_len[0], q.stop_ids[0] = 1, 5
            q.stop_len[1], q.stop_ids[L], q.stop_ids[L + 1] = 2, 5, 6
            pens[b].repetition_penalty, pens[b].penalize_prompt = 1.0, 1
        return seq, allow, pens

    def admit_bad(prompts):
        seq, allow, pens = records(len(prompts))
        q = seq[1]
        if bad == "n_bias33":
            q.n_bias = 33
        elif bad == "n_bias<0":
            q.n_bias = -1
        elif bad == "n_stop9":
            q.n_stop = 9
        elif bad == "n_stop<0":
            q.n_stop = -1
        elif bad == "reserved":
            q.reserved[1] = 1
        elif bad == "len0":
            q.bias_len[0] = 0
        elif bad == "len9":
            q.bias_len[0] = 9
        elif bad == "id<0":
            q.bias_ids[1] = -1
        elif bad == "id=V":
            q.bias_ids[0] = V
        elif bad == "nan":
            q.bias[0] = float("nan")
        elif bad == "+inf":
            q.bias[0] = float("inf")
        elif bad == "dup":
            q.bias_len[1], q.bias_ids[L], q.bias_ids[L + 1] = 2, 3, 4
        elif bad == "slen0":
            q.stop_len[1] = 0
        elif bad == "slen9":
            q.stop_len[1] = 9
        elif bad == "sid=V":
            q.stop_ids[L + 1] = V
        elif bad == "sdup":
            q.stop_len[1] = 1
        elif bad == "no_survivor_allow":
            allow[1].n_ranges, allow[1].lo[0], allow[1].hi[0] = 1, 9, 10
        elif bad == "no_survivor":
            allow[1].n_ranges, allow[1].lo[0], allow[1].hi[0] = 1, 8, 10
            q.n_bias, q.bias_len[0], q.bias[0], q.bias_ids[1] = 2, 2, NINF, 8     # (3, 8) -inf: its last id counts
        elif bad == "eos_only":
            allow[1].n_ranges, allow[1].lo[0], allow[1].hi[0] = 1, 7, 10           # {7 (eos), 8, 9}; 9 banned, 8 banned below
            q.bias_len[0], q.bias[0], q.bias_ids[0], q.bias_ids[1] = 1, NINF, 8, 0
            pens[1].min_new_tokens = 2
        return _raw_admit(llm, prompts, seq=seq, allow=allow, pens=pens)[0]

    def run(fail):
        llm.session_begin([7])
        first = llm.admit(ps[:2], [{"bad_words_ids": [[9]], "stop_sequences": [[5]]}, None])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            assert admit_bad(ps[2:]) == -1   # SMI_EINVAL
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        seq, allow, pens = records(3)
        rc, slots = _raw_admit(llm, ps[2:], seq=seq, allow=allow, pens=pens)   # the slots and admission numbers the failed call left
        assert rc == 0
        llm.decode(10)
        return slots, [t for t, _ in llm.slots_tokens(first + slots, 16)]

    assert run(True) == run(False)


# 9 -------------------------------------------------------------------------------------------------------------------
def test_past_32_rows_at_the_0p5b_shape(full_llm):
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(77))
    B, N = 40, 10
    ps = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(4, 24))).tolist() for _ in range(B)]
    big = SparkLLM(cfg, None, "cuda:0", max_positions=FULL_MAX_POS, arena=arena, max_slots=B, kv_dtype="f32")
    one = SparkLLM(cfg, None, "cuda:0", max_positions=FULL_MAX_POS, arena=arena, max_slots=1, kv_dtype="f32")
    plain = big.generate_ragged(ps, [N] * B)
    recs = []
    for b in range(B):
        if b % 4 == 3:
            recs.append(None)
            continue
        rec = {"bad_words_ids": [[plain[b][0]], [plain[b][2], plain[b][3]]], "sequence_bias": [((plain[b][1],), -4.0), ((ps[b][-1], 11), 25.0)]}
        if b % 4 == 1:
            rec["stop_sequences"] = [[11]]
        if b % 4 == 2:
            rec.update(do_sample=True, temperature=1.1, top_k=30, top_p=0.9, seed=b, return_log_probs=True)
        recs.append(rec)
    got = big.generate_ragged(ps, [N] * B, sampling=recs)
    for b in range(B):
        if recs[b] is None:
            assert got[b] == plain[b]
        else:
            assert _same(got[b], one.generate_ragged([ps[b]], [N], sampling=[recs[b]])[0]), f"row {b}"
            toks = got[b][0] if isinstance(got[b], tuple) else got[b]
            assert toks[0] != plain[b][0]
