"""smi_llm_poll (SparkLLM.poll): the new tokens of listed slots in one small round trip.  By definition it is smi_llm_slots_tokens
of the same slots, sliced -- checked on a session whose slots were admitted at different times, some retired; bad arguments are
SMI_EINVAL with nothing written; a poll between decode calls leaves the cached step graph (and so the tokens) alone."""
import ctypes as C

import numpy as np
import pytest

from sparkmi import _lib, config as CFG, weights as W

pytestmark = pytest.mark.gpu

MAX_POS = 128


def _prompts(cfg, n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, cfg.vocab_size, size=int(rng.integers(5, 20))).tolist() for _ in range(n)]


@pytest.fixture(scope="module")
def tiny():
    cfg = CFG.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


def _session(tiny, poll_between, use_graph=True):
    """Slots admitted at different times, one retired and reused, two retired and left; returns (llm, the slots in use)."""
    from sparkmi.llm import SparkLLM
    cfg, syn = tiny
    llm = SparkLLM(cfg, syn, "cuda:0", max_slots=6, max_positions=MAX_POS, use_graph=use_graph)
    p = _prompts(cfg, 7, 21)
    llm.session_begin(None)
    seen = []

    def maybe_poll():
        if poll_between and seen:
            llm.poll(seen, [0] * len(seen), 3)
            llm.poll(seen[::-1], [2] * len(seen), 64)

    seen += llm.admit(p[:2])
    llm.decode(5); maybe_poll()
    llm.decode(5); maybe_poll()
    seen += llm.admit(p[2:6])           # every slot is taken
    llm.decode(7); maybe_poll()
    llm.retire_many([seen[1]])
    maybe_poll()
    llm.decode(4); maybe_poll()
    reused = llm.admit(p[6:7])          # takes the one free slot: its history starts again
    assert reused == [seen[1]]
    llm.decode(6); maybe_poll()
    llm.retire_many([seen[0], seen[3]])  # retired and not reused: they stay readable
    llm.decode(3); maybe_poll()
    llm.decode(2); maybe_poll()
    return llm, seen


def test_poll_equals_slots_tokens_sliced(tiny):
    llm, seen = _session(tiny, poll_between=False)
    slots = sorted(set(seen))
    full = llm.slots_tokens(slots, MAX_POS)
    counts = [len(t) for t, _ in full]
    assert len(set(counts)) >= 4 and min(counts) >= 3, counts   # admitted at different times: different histories
    cases = [([0] * len(slots), MAX_POS), ([0] * len(slots), 1), ([1] * len(slots), 4), ([2] * len(slots), 1000),
             (counts, 8),                                  # from == count: zero ids
             ([c + 5 for c in counts], 8),                 # from > count: zero ids
             ([max(0, c - 3) for c in counts], 2),         # cap smaller than the backlog
             ([max(0, c - 3) for c in counts], 3), ([i % 3 for i in range(len(slots))], 5), ([MAX_POS + 7] * len(slots), 4)]
    for frm, cap in cases:
        got = llm.poll(slots, frm, cap)
        for i, (new, count, fin) in enumerate(got):
            toks, tfin = full[i]
            assert count == len(toks) and fin == tfin
            assert new == toks[frm[i]: frm[i] + cap], (slots[i], frm[i], cap)
            assert len(new) == max(0, min(count, frm[i] + cap) - frm[i])
    # any subset, in any order, a slot listed twice
    order = [slots[-1], slots[0], slots[2], slots[0]]
    got = llm.poll(order, [1, 0, 2, 3], 6)
    for s, f, (new, count, _) in zip(order, [1, 0, 2, 3], got):
        toks = full[slots.index(s)][0]
        assert new == toks[f: f + 6] and count == len(toks)
    # the older readers still agree with each other
    for i, s in enumerate(slots):
        assert llm.slot_tokens(s, MAX_POS)[0] == full[i][0]


def test_poll_reports_eos(tiny):
    """finished and a frozen count, as slots_tokens reports them."""
    from sparkmi.llm import SparkLLM
    cfg, syn = tiny
    llm = SparkLLM(cfg, syn, "cuda:0", max_slots=2, max_positions=MAX_POS)
    p = _prompts(cfg, 2, 5)
    llm.session_begin(None)
    s = llm.admit(p)
    llm.decode(12)
    toks = llm.slots_tokens(s, MAX_POS)[0][0]
    eos = toks[6]                       # whatever the 7th token was becomes the stop id of a second session
    llm.session_begin([eos])
    s = llm.admit(p)
    llm.decode(12)
    full = llm.slots_tokens(s, MAX_POS)
    assert full[0][1] and len(full[0][0]) == toks.index(eos) + 1
    got = llm.poll(s, [0, 0], MAX_POS)
    for (new, count, fin), (t, f) in zip(got, full):
        assert new == t and count == len(t) and fin == f


def test_bad_arguments_are_einval_and_write_nothing(tiny):
    llm, seen = _session(tiny, poll_between=False)
    lib = llm._lib
    i32, i64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)

    def call(slots, frm, n, cap):
        a, f = np.asarray(slots, np.int32), np.asarray(frm, np.int32)
        out = np.full((max(len(a), 1), max(cap, 4)), -77, np.int64)
        n_out, cnt, fin = (np.full(max(len(a), 1), -77, np.int32) for _ in range(3))
        rc = lib.smi_llm_poll(llm._h, a.ctypes.data_as(i32), f.ctypes.data_as(i32), n, out.ctypes.data_as(i64), cap,
                              n_out.ctypes.data_as(i32), cnt.ctypes.data_as(i32), fin.ctypes.data_as(i32), llm._stream())
        untouched = (out == -77).all() and (n_out == -77).all() and (cnt == -77).all() and (fin == -77).all()
        return rc, untouched

    EINVAL = -1
    assert call([seen[0]], [0], 1, 4) == (0, False)
    big = [0] * (_lib.SMI_MAX_ROWS + 1)
    for args in (([seen[0]], [0], 0, 4), (big, big, _lib.SMI_MAX_ROWS + 1, 4), ([_lib.SMI_MAX_ROWS], [0], 1, 4), ([-1], [0], 1, 4),
                 ([seen[0], seen[2]], [0, -1], 2, 4), ([seen[0]], [0], 1, 0), ([seen[0]], [0], 1, -3)):
        rc, untouched = call(*args)
        assert rc == EINVAL and untouched, args
        assert b"smi_llm_poll" in lib.smi_last_error()
    with pytest.raises(_lib.SparkMIError):
        llm.poll([seen[0]], [0], 0)
    with pytest.raises(ValueError):
        llm.poll([seen[0]], [0, 1], 4)


def test_poll_between_decode_calls_leaves_the_step_graph_alone(tiny):
    """use_graph=1: the same session with and without polls between its decode calls ends with the same tokens."""
    quiet, seen_q = _session(tiny, poll_between=False, use_graph=True)
    want = quiet.slots_tokens(sorted(set(seen_q)), MAX_POS)
    polled, seen_p = _session(tiny, poll_between=True, use_graph=True)
    assert seen_p == seen_q
    slots = sorted(set(seen_p))
    assert polled.slots_tokens(slots, MAX_POS) == want
    assert [(t, f) for t, _, f in polled.poll(slots, [0] * len(slots), MAX_POS)] == want
    polled.decode(5)
    quiet.decode(5)
    assert polled.slots_tokens(slots, MAX_POS) == quiet.slots_tokens(slots, MAX_POS)
