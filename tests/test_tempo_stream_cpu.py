"""Tempo of joined streams, host side (sparkmi/streaming.py: tempo_piece_len, tempo_history; smi_tempos_piece_len; sparkmi/audio.py:
StreamTempo with a stand-in library; streaming.Pacer with a tempo) against tests/tempo_stream_ref.py and tests/tempo_ref.py: the
piece lengths, that what a stream has emitted no longer depends on what follows, the history bound of the header, and the
bookkeeping.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import tempo_ref as tr
import tempo_stream_ref as ts
from sparkmi import audio, streaming

TEMPOS = [(5, 4), (4, 5), (2, 1), (1, 2), (3, 2), (101, 100), (99, 100), (4, 1), (1, 4), (1, 1)]
FRAMES = [(16, 4), (16, 0), (64, 8)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cuts(rng, total, m):
    """m push lengths that sum to total; zeros among them"""
    at = np.sort(rng.integers(0, total + 1, size=m - 1))
    return np.diff(np.concatenate([[0], at, [total]])).astype(int).tolist()


@pytest.mark.parametrize("N,D", FRAMES + [(512, 240)])
def test_piece_lengths_against_the_reference_and_the_library(N, D):
    from sparkmi import _lib
    l = _lib.lib()
    rng = np.random.default_rng(N + D)
    H, zero_pieces = N // 2, 0
    for p, q in TEMPOS:
        for trial in range(6):
            total = int(rng.integers(0, 20 * N + 38))
            cuts = _cuts(rng, total, int(rng.integers(1, 12)))
            n = f = got_sum = 0
            for i, c in enumerate(cuts):
                last = i == len(cuts) - 1
                piece, n1, f1 = streaming.tempo_piece_len(p, q, N, D, n, f, c, last)
                na, fa = C.c_longlong(-7), C.c_longlong(-7)
                assert l.smi_tempos_piece_len(p, q, N, D, n, f, c, int(last), C.byref(na), C.byref(fa)) == piece
                assert (na.value, fa.value) == (n1, f1)
                before = ts.emitted(n, p, q, N, D, False)
                assert piece == ts.emitted(n1, p, q, N, D, last) - before, (p, q, N, D, cuts, i)
                assert f1 == ts.frames(n1, p, q, N, D, last) and n1 == n + c
                assert last or p == q or (piece % H == 0 and before + piece <= tr.layout(n1, p, q, N)[0])
                zero_pieces += piece == 0 and c > 0
                n, f, got_sum = n1, f1, got_sum + piece
            assert got_sum == tr.layout(total, p, q, N)[0] == audio.tempo_len(total, p, q)   # pieces sum to M for any cuts
    assert zero_pieces > 0, "no push that emits nothing among the cuts"
    # arguments the arithmetic refuses
    assert l.smi_tempos_piece_len(5, 1, N, D, 0, 0, 10, 0, None, None) == -1
    assert l.smi_tempos_piece_len(5, 4, N + 1, D, 0, 0, 10, 0, None, None) == -1
    assert l.smi_tempos_piece_len(5, 4, N, D, 10, 4000, 10, 1, None, None) == -1     # more frames gone than the stream can hold
    for bad in ((5, 1, N, D, 0, 0, 10, False), (5, 4, N + 1, D, 0, 0, 10, False), (5, 4, N, D, 10, 4000, 10, True), (5, 4, N, D, 0, 0, -1, False)):
        with pytest.raises(ValueError):
            streaming.tempo_piece_len(*bad)


@pytest.mark.parametrize("N,D", FRAMES)
def test_what_a_stream_has_emitted_does_not_depend_on_what_follows(N, D):
    """the reference alone: for a prefix of n samples the first E(n) outputs are those of the whole row, whether nothing, other
    noise or NaNs follow the prefix; and the history the header keeps is enough for every n"""
    L = 20 * N + 37
    x = tr.signal(L, 7)
    other = tr.signal(L + 3 * N + 50, 8)
    nan = np.full(3 * N + 50, np.nan, dtype=np.float32)
    bound = streaming.tempo_history(N, D)
    assert bound == max(7 * (N // 2) + D, 5 * (N // 2) + 2 * D)
    for p, q in TEMPOS:
        full, s_full = tr.tempo(x, p, q, N, D)
        worst = 0
        for n in range(0, L + 1, 5 if N == 16 else 23):
            E = ts.emitted(n, p, q, N, D, False)
            F = ts.frames(n, p, q, N, D, False)
            assert E <= full.size, (p, q, n)
            for tail in (x[:0], other[n:], nan):
                o, s = tr.tempo(np.concatenate([x[:n], tail]), p, q, N, D)
                assert np.array_equal(_bits(o[:E]), _bits(full[:E])), (p, q, n, tail.size)
                if p != q:
                    assert np.array_equal(s[:F], s_full[:F])
            if p != q:
                h0 = ts.history_start(F, p, q, N, D)
                assert h0 == streaming.tempo_history_start(F, p, q, N, D)
                worst = max(worst, n - h0)
        assert worst <= bound, (p, q, worst, bound)


def test_history_bound_holds_for_every_n_at_the_default_frame():
    N, D = audio.tempo_frame(16000)
    assert (N, D) == (512, 240)
    bound = streaming.tempo_history(N, D)
    for p, q in TEMPOS[:-1] + [audio.tempo_ratio(t) for t in (0.5, 0.51, 1.99, 2.0)]:
        worst = f = 0
        for n in range(0, 12 * N):
            while (f + 1) * (N // 2) <= -((-n * q) // p) and n >= ts.ready(f, p, q, N, D):
                f += 1
            assert f == ts.frames(n, p, q, N, D, False)
            worst = max(worst, n - ts.history_start(f, p, q, N, D))
        assert 0 < worst <= bound, (p, q, worst, bound)


def test_stream_reference_cuts_the_batch_result():
    x = tr.signal(20 * 64 + 37, 3)
    pieces, places = ts.stream(x, [1, 0, 500, 300, 516, 0], 3, 2, 64, 8)
    out, s = tr.tempo(x, 3, 2, 64, 8)
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(out)) and np.array_equal(np.concatenate(places), s)
    assert pieces[0].size == 0 and pieces[2].size > 0 and all(p.size % 32 == 0 for p in pieces[:-1])
    one, _ = ts.stream(x, [7, 1300, 10], 1, 1, 64, 8)
    assert [p.size for p in one] == [7, 1300, 10] and np.array_equal(_bits(np.concatenate(one)), _bits(x))


class _FakeLib:
    """records what StreamTempo sends to the library"""

    def __init__(self):
        self.created, self.opened, self.pushes, self.destroyed = [], [], [], 0

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_tempos_create(self, max_streams, max_chunk, N, D, win, href):
        self.created.append((max_streams, max_chunk, N, D, [win[i] for i in range(N)]))
        href._obj.value = 4321
        return 0

    def smi_tempos_destroy(self, h):
        self.destroyed += 1
        return 0

    def smi_tempos_open(self, h, slot, p, q):
        self.opened.append((slot, p, q))
        return 0

    def smi_tempos_push_rows(self, h, src, stride, streams, lens, lasts, B, pos, pos_stride, dst, out_stride, n_out, stream):
        assert len(set(streams[:B])) == B, "a stream twice in one call"
        self.pushes.append((list(streams[:B]), list(lens[:B]), list(lasts[:B]), out_stride))
        return 0


def test_stream_tempo_slots_with_a_stand_in_library():
    fake = _FakeLib()
    t = audio.StreamTempo(3, 4000, (64, 8), lib=fake)
    assert fake.created[0][:4] == (3, 4000, 64, 8) and np.array_equal(fake.created[0][4], tr.window(64))
    assert t.history == streaming.tempo_history(64, 8) == 232
    assert t.open("a", 5, 4) == 0 and t.open("b", 4, 5) == 1
    with pytest.raises(ValueError):
        t.open("a", 5, 4)
    want = t.piece_lengths([("a", 30, False), ("b", 300, False), ("c", 40, True)])
    _, lens = t.push(None, [("a", 30, False), ("b", 300, False), ("c", 40, True)])
    assert lens == want == [ts.emitted(30, 5, 4, 64, 8, False), ts.emitted(300, 4, 5, 64, 8, False), 40]
    assert lens[0] == 0 and lens[1] > 0                    # 30 samples are not yet a frame; a stream never opened copies at 1/1
    assert fake.opened == [(0, 5, 4), (1, 4, 5), (2, 1, 1)] and t.calls == 1
    assert t.slot("c") is None and t.slot("a") == 0 and t.slot("b") == 1
    # a's last chunk and its empty flush in one poll: two calls; the freed slots are used again
    _, lens = t.push(None, [("a", 500, False), ("a", 0, True), ("b", 10, False), ("d", 12, False)])
    assert t.calls == 3 and [p[0] for p in fake.pushes[1:]] == [[0], [0, 1, 2]]
    assert sum(lens[:2]) == tr.layout(530, 5, 4, 64)[0] and lens[3] == 12
    assert t.slot("a") is None and t.slot("d") == 2
    t.open("e", 2, 1)
    assert t.slot("e") == 0
    with pytest.raises(ValueError):
        t.push(None, [("f", 12, False)])                   # a fourth open request
    with pytest.raises(ValueError):
        t.push(None, [("b", 4001, False)])                 # beyond max_chunk: refused before the library is called
    assert t.calls == 3
    t.reset()
    assert t.slot("b") is None and t.open("g", 1, 2) == 0
    t.close()
    assert fake.destroyed == 1


def test_pacer_counts_the_seconds_a_listener_receives():
    now = [0.0]
    pc = streaming.Pacer(1, max_open=2, max_ahead=0.5, frame_rate=50, clock=lambda: now[0])
    pc.yielded("slow", 50, 50 * 320 * 5 / 4 / 16000)       # a second of frames at tempo 0.8: 1.25 s of audio
    pc.yielded("fast", 50, 50 * 320 * 4 / 5 / 16000)       # at 1.25: 0.8 s
    pc.yielded("plain", 50)
    now[0] = 0.5
    assert pc.lead("slow") == pytest.approx(0.75) and pc.lead("fast") == pytest.approx(0.3) and pc.lead("plain") == pytest.approx(0.5)
    assert pc.to_park(["fast"], [], True) == [] and pc.to_park(["slow"], [], True) == ["slow"]
    pc.yielded("fast", 50, 0.0)                            # a push whose piece is empty adds nothing
    assert pc.lead("fast") == pytest.approx(0.3)
