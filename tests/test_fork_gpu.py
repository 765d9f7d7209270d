"""num_return_sequences (smi_llm_admit_forked): one prompt prefilled once, forked into n takes.  Every take is bit for bit the
admission that lists the prompt n times -- slots, admission numbers, tokens, log-probabilities and K/V rows, contiguous and
paged, bf16 and f32; next to live sequences; in a paged cache the followers share the leader's leading pages, which survive
the leader's retirement; a failing call changes nothing.  At full size: a class-2 (k_pgemm) prompt, and the graph-captured
step at 40 rows."""
import ctypes

import numpy as np
import pytest

from conftest import FULL_MAX_POS
from sparkmi import _lib, config as C, weights as W
from sparkmi.llm import expand_takes, logprob_flags, penalty_records, sampling_records

pytestmark = pytest.mark.gpu

SMI_EINVAL, SMI_ENOMEM = -1, -3
SAMPLER = (True, 0.9, 40, 0.95)


def _llm(cfg, syn, **kw):
    from sparkmi.llm import SparkLLM
    return SparkLLM(cfg, syn, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def tiny():
    cfg = C.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


def _prompt(cfg, seed, n):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, cfg.vocab_size, size=n).tolist()


def _raw(llm, prompts, n_ret, takes):
    """smi_llm_admit_forked(prompts, n_ret) with per-take records, or (n_ret None) smi_llm_admit_logprobs of the prompts as
    given; returns (rc, slots)."""
    N = len(takes)
    n, pmax = len(prompts), max(len(p) for p in prompts)
    ids = np.zeros((n, pmax), dtype=np.int64)
    for b, p in enumerate(prompts):
        ids[b, : len(p)] = p
    lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
    recs, pens, flags = sampling_records(takes, N, llm._sampling), penalty_records(takes, N), logprob_flags(takes, N)
    fl = None if flags is None else flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    slots = np.zeros(max(N, 1), dtype=np.int32)
    P = ctypes.POINTER
    if n_ret is None:
        rc = llm._lib.smi_llm_admit_logprobs(llm._h, ids.ctypes.data_as(P(ctypes.c_int64)), lens.ctypes.data_as(P(ctypes.c_int32)),
                                             n, pmax, recs, pens, fl, slots.ctypes.data_as(P(ctypes.c_int32)), llm._stream())
    else:
        nr = np.asarray(n_ret, dtype=np.int32)
        rc = llm._lib.smi_llm_admit_forked(llm._h, ids.ctypes.data_as(P(ctypes.c_int64)), lens.ctypes.data_as(P(ctypes.c_int32)),
                                           n, pmax, nr.ctypes.data_as(P(ctypes.c_int32)), recs, pens, fl,
                                           slots.ctypes.data_as(P(ctypes.c_int32)), llm._stream())
    return rc, slots[:N].tolist()


def _expand(prompts, n_ret):
    return [p for p, k in zip(prompts, n_ret) for _ in range(k)]


def _pages(L, P, n):
    own = -(-L // P)
    return own + (n - 1) * (own - (L - 1) // P)


# 1 -------------------------------------------------------------------------------------------------------------------
# per take: inherit (the handle samples), greedy, sampled-seeded, penalised (penalize_prompt 0 and 1), return_log_probs
TAKES = [
    None,
    {"do_sample": False},
    {"do_sample": True, "temperature": 0.7, "top_k": 30, "top_p": 0.9, "seed": 11, "return_log_probs": True},
    {"do_sample": False, "repetition_penalty": 1.3, "penalize_prompt": True, "return_log_probs": True},
    {"do_sample": True, "seed": 12, "repetition_penalty": 1.2, "presence_penalty": 0.3, "penalize_prompt": False},
    {"frequency_penalty": 0.4, "return_log_probs": True},
]


@pytest.mark.parametrize("kv", ["bf16", "f32"])
def test_fork_equals_the_expanded_admission_contiguous(tiny, kv):
    cfg, syn = tiny
    prompts = [_prompt(cfg, 1, 23), _prompt(cfg, 2, 5), _prompt(cfg, 3, 41)]
    n_ret, steps = [3, 1, 2], 40
    llm = _llm(cfg, syn, max_slots=8, max_positions=128, kv_dtype=kv, diag=True)   # (debug_get_kv)
    llm.set_sampling(*SAMPLER, seed=5)
    lens = [len(p) for p in _expand(prompts, n_ret)]

    def run(forked):
        llm.session_begin()
        rc, slots = _raw(llm, prompts, n_ret, TAKES) if forked else _raw(llm, _expand(prompts, n_ret), None, TAKES)
        assert rc == 0, _lib.lib().smi_last_error()
        llm.decode(steps)
        toks = [t for t, _ in llm.slots_tokens(slots, steps + 1)]
        flagged = [j for j, d in enumerate(TAKES) if d and d.get("return_log_probs")]
        lps = llm.slots_logprobs([slots[j] for j in flagged], steps + 1)
        kv_rows = [[llm.debug_get_kv(layer, s, 0, L + steps) for layer in range(cfg.num_hidden_layers)] for s, L in zip(slots, lens)]
        return slots, toks, lps, kv_rows

    fs, ft, fl, fk = run(True)
    es, et, el, ek = run(False)
    assert fs == es == list(range(6))
    assert all(len(t) == steps + 1 for t in ft)
    assert ft == et
    assert len(fl) == 3 and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(fl, el))
    for j in range(6):
        for layer in range(cfg.num_hidden_layers):
            for a, b in zip(fk[j][layer], ek[j][layer]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"take {j} layer {layer}"
    assert ft[0] != ft[1] or ft[0] != ft[2]   # the takes are not one sequence copied


# 2 -------------------------------------------------------------------------------------------------------------------
def test_forked_admission_next_to_live_sequences(tiny):
    cfg, syn = tiny
    others = [_prompt(cfg, 10, 17), _prompt(cfg, 11, 33)]
    p = _prompt(cfg, 12, 27)
    rec = {"do_sample": True, "temperature": 0.8, "top_k": 40, "top_p": 0.95, "seed": 3}
    llm = _llm(cfg, syn, max_slots=8, max_positions=128)
    llm.set_sampling(*SAMPLER, seed=9)

    def run(forked, with_takes=True):
        llm.session_begin()
        live = llm.admit(others, [None, {"do_sample": False}])
        llm.decode(7)
        takes = []
        if with_takes:
            takes = llm.admit([p], [rec], n_return=[3]) if forked else llm.admit([p] * 3, expand_takes([rec], [3]))
        llm.decode(20)
        return [t for t, _ in llm.slots_tokens(live, 40)], [t for t, _ in llm.slots_tokens(takes, 40)] if takes else []

    solo_live, _ = run(False, with_takes=False)
    f_live, f_takes = run(True)
    e_live, e_takes = run(False)
    assert f_live == solo_live == e_live
    assert all(len(t) == 28 for t in f_live)
    assert f_takes == e_takes and len(f_takes) == 3 and all(len(t) == 21 for t in f_takes)


# 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [33, 32, 9, 45], ids=["Lm1_mult_P", "L_mult_P", "L_lt_P", "general"])
def test_paged_fork_shares_pages_and_survives_the_leader(tiny, L):
    cfg, syn = tiny
    P, n = 16, 3
    p = _prompt(cfg, 20 + L, L)
    newcomers = [_prompt(cfg, 30, 40), _prompt(cfg, 31, 29)]
    llm = _llm(cfg, syn, max_slots=8, max_positions=128, kv_page_tokens=P, kv_pages=24)
    llm.set_sampling(*SAMPLER, seed=4)   # inheriting takes: each draws its own stream (admission number)

    def run(forked):
        llm.session_begin()
        total, free0 = llm.kv_pages()
        assert free0 == total == 24
        slots = llm.admit([p], None, n_return=[n]) if forked else llm.admit([p] * n)
        used = free0 - llm.kv_pages()[1]
        llm.decode(4)
        llm.retire(slots[0])               # the leader leaves first ...
        late = llm.admit(newcomers)        # ... and the pages it freed are taken at once (the pool hands out the last freed first)
        llm.decode(20)
        toks = [t for t, _ in llm.slots_tokens(slots[1:] + late, 40)]
        llm.retire_many(slots[1:] + late)
        assert llm.kv_pages() == (total, total)
        return slots, used, toks

    fs, fused, ft = run(True)
    es, eused, et = run(False)
    assert fs == es
    assert fused == _pages(L, P, n), (fused, _pages(L, P, n))
    assert eused == n * -(-L // P)
    assert ft == et
    assert all(len(t) == 25 for t in ft[: n - 1])


# 4 -------------------------------------------------------------------------------------------------------------------
def test_a_failing_fork_changes_nothing(tiny):
    cfg, syn = tiny
    P = 16
    live_ps = [_prompt(cfg, 40, 20), _prompt(cfg, 41, 12)]
    nxt = [_prompt(cfg, 42, 15)]
    long_p = _prompt(cfg, 43, 60)                                   # 4 pages alone, 4 + 3 * 1 = 7 pages with 4 takes
    llm = _llm(cfg, syn, max_slots=6, max_positions=128, kv_page_tokens=P, kv_pages=9)
    llm.set_sampling(*SAMPLER, seed=6)   # unseeded rows: their streams are keyed by admission numbers

    def run(fail):
        llm.session_begin()
        first = llm.admit(live_ps)                                  # 2 + 1 pages: 6 of 9 left
        llm.decode(3)
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        assert pages == (9, 6)
        if fail:
            cases = [([long_p], [4], SMI_ENOMEM),                   # the leader fits, its followers do not
                     ([nxt[0]], [0], SMI_EINVAL), ([nxt[0]], [-1], SMI_EINVAL), ([nxt[0], long_p], [2, 0], SMI_EINVAL),
                     ([nxt[0]], [5], SMI_EINVAL)]                   # 5 takes, 4 free slots
            for prompts, n_ret, want in cases:
                rc, _ = _raw(llm, prompts, n_ret, [None] * max(sum(n_ret), 1))
                assert rc == want, (n_ret, rc, _lib.lib().smi_last_error())
                assert llm.kv_pages() == pages
                cnt2, fin2 = llm.status()
                assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        slots = first + llm.admit(nxt, None, n_return=[2])          # the slots and admission numbers the failed calls did not take
        llm.decode(10)
        return slots, [t for t, _ in llm.slots_tokens(slots, 20)]

    assert run(True) == run(False)


# 5 -------------------------------------------------------------------------------------------------------------------
def test_class2_prompt_forked_at_full_size(full_llm):
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    p = _prompt(cfg, 50, 460)                                       # 459 prompt rows: the k_pgemm prefill family
    llm = SparkLLM(cfg, None, "cuda:0", max_slots=8, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    solo = llm.generate_ragged([p], [150])[0]
    takes = llm.generate_ragged([p], [150], n_return=[8])
    assert len(takes) == 1 and len(takes[0]) == 8
    assert all(t == solo for t in takes[0])
    llm.set_sampling(True, 0.8, 50, 0.95, seed=3)
    takes = llm.generate_ragged([p], [150], n_return=[8])[0]
    assert takes == llm.generate_ragged([p] * 8, [150] * 8)
    assert len({tuple(t) for t in takes}) > 1


# 6 -------------------------------------------------------------------------------------------------------------------
def test_graph_step_past_32_rows_forked(full_llm):
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    p = _prompt(cfg, 60, 19)
    llm = SparkLLM(cfg, None, "cuda:0", max_slots=40, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16", use_graph=True)
    llm.set_sampling(True, 0.8, 50, 0.95, seed=8)
    takes = llm.generate_ragged([p], [24], n_return=[40])[0]
    assert len(takes) == 40
    assert takes == llm.generate_ragged([p] * 40, [24] * 40)
