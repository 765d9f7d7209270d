"""Pitch shift of joined streams, host side (sparkmi/streaming.py: pitch_piece_len; smi_pitchs_piece_len; sparkmi/audio.py:
StreamPitch with a stand-in library; the pipeline's refusals) against tests/pitch_stream_ref.py and tests/pitch_ref.py: the piece
lengths, that what a stream has emitted no longer depends on what follows -- the proof the kernel rests on --, the bounds of the
header, and the bookkeeping.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as pr
import pitch_stream_ref as ps
import tempo_ref as tr
from sparkmi import audio, streaming

RATIOS = [(3, 2), (2, 3), (28, 25), (89, 100), (199, 100), (101, 200)]
TEMPOS = [(1, 1), (5, 4), (4, 5)]
FRAMES = [(16, 3), (64, 8), (512, 240)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cuts(rng, total, m):
    """m push lengths that sum to total; zeros among them"""
    at = np.sort(rng.integers(0, total + 1, size=m - 1))
    return np.diff(np.concatenate([[0], at, [total]])).astype(int).tolist()


def _both(l, t, r, N, D, nt, n, f, k, c, last):
    """one push through the Python twin and the library: (piece, n, f, k), equal in both"""
    got = streaming.pitch_piece_len(t[0], t[1], r[0], r[1], N, D, nt, n, f, k, c, last)
    na, fa, ka = C.c_longlong(-7), C.c_longlong(-7), C.c_longlong(-7)
    piece = l.smi_pitchs_piece_len(t[0], t[1], r[0], r[1], N, D, nt, n, f, k, c, int(last), C.byref(na), C.byref(fa), C.byref(ka))
    assert (piece, na.value, fa.value, ka.value) == got, (t, r, N, D, n, c, last)
    return got


@pytest.mark.parametrize("N,D", FRAMES)
def test_piece_lengths_against_the_reference_and_the_library(N, D):
    """every n up to 6 N + 40 by pushes of one sample, then random cuts: the counters of the library and of its Python twin are
    the reference's, K(n) never falls and never passes ceil(n tq / tp), the tail never passes its bounds, and the pieces of any
    cuts sum to n_out"""
    from sparkmi import _lib
    l = _lib.lib()
    rng = np.random.default_rng(N + D)
    top = 6 * N + 40
    for r in RATIOS + [(1, 1)]:
        for t in TEMPOS:
            nt = ps.n_taps(t, r)
            pl = pr.plan(0, t, r, N)
            n = f = k = worst = 0
            for _ in range(top):
                piece, n, f, k1 = _both(l, t, r, N, D, nt, n, f, k, 1, False)
                assert k1 == ps.emitted(n, t, r, N, D, False) and f == ps.frames(n, t, r, N, D, False), (t, r, n)
                assert piece == k1 - k >= 0                                   # monotone
                assert k1 <= -((-n * t[1]) // t[0]), (t, r, n, k1)              # never more than the final n_out, whatever follows
                E = ps.stretched(n, t, r, N, D, False)
                t0 = ps.tail_start(k1, t, r)
                assert t0 == streaming.pitch_tail_start(k1, pl["up"], pl["down"], nt // 2) and 0 <= t0 <= E
                worst = max(worst, E - t0)
                k = k1
            assert worst <= ps.tail_bound(t, r) and worst <= nt // 2 * 2 // pl["up"] + (r == (1, 1)) and worst <= nt + 1, (t, r, worst)
            assert r == (1, 1) or worst > 0
            for trial in range(3):
                total = int(rng.integers(0, top))
                cuts = _cuts(rng, total, int(rng.integers(1, 9)))
                n = f = k = 0
                for i, c in enumerate(cuts):
                    last = i == len(cuts) - 1
                    piece, n, f, k = _both(l, t, r, N, D, nt, n, f, k, c, last)
                    assert k == ps.emitted(n, t, r, N, D, last) and f == ps.frames(n, t, r, N, D, last)
                assert k == pr.plan(total, t, r, N)["n_out"] == audio.tempo_len(total, *t)   # pieces sum to n_out for any cuts
    # a stream at the pitch ratio 1/1 is the tempo stream, one without a tempo either a copy
    assert streaming.pitch_piece_len(5, 4, 7, 7, N, D, 0, 0, 0, 0, 5 * N, False)[0] == streaming.tempo_piece_len(5, 4, N, D, 0, 0, 5 * N, False)[0]
    assert streaming.pitch_piece_len(1, 1, 1, 1, N, D, 0, 10, 0, 10, 33, False) == (33, 43, 43 // (N // 2), 43)


def test_bad_arguments_return_minus_one():
    from sparkmi import _lib
    l = _lib.lib()
    ok = (1, 1, 3, 2, 64, 8, 61, 0, 0, 0, 10, 0)
    assert l.smi_pitchs_piece_len(*ok, None, None, None) == 0
    for i, v in ((0, 0), (1, 40000), (2, 0), (3, -1), (4, 65), (4, 8), (5, 2000), (6, 60), (6, 1), (6, 0), (6, 3), (7, -1), (8, -1),
                 (9, -1), (10, -1), (11, 2), (10, (1 << 28) + 1)):
        bad = list(ok)
        bad[i] = v
        assert l.smi_pitchs_piece_len(*bad, None, None, None) == -1, (i, v)
        if i != 11:   # (the twin takes a bool)
            with pytest.raises(ValueError):
                streaming.pitch_piece_len(*bad[:11], bool(bad[11]))
    assert l.smi_pitchs_piece_len(1, 1, 1, 1, 64, 8, 61, 0, 0, 0, 10, 0, None, None, None) == -1     # taps at the ratio 1/1
    assert l.smi_pitchs_piece_len(1, 4, 4, 1, 64, 8, 81, 0, 0, 0, 10, 0, None, None, None) == -1     # a stretch of 1/16
    assert l.smi_pitchs_piece_len(1, 1, 3, 2, 64, 8, 61, 100, 0, 500, 10, 0, None, None, None) == -1  # more outputs gone than there are
    assert l.smi_pitchs_piece_len(1, 1, 2, 3, 64, 8, 5, 0, 0, 0, 10, 0, None, None, None) == -1      # G = 2 < up = 3
    with pytest.raises(ValueError):
        streaming.pitch_piece_len(1, 1, 2, 3, 64, 8, 5, 0, 0, 0, 10, False)
    with pytest.raises(ValueError):
        streaming.pitch_piece_len(1, 1, 3, 2, 64, 8, 61, 100, 0, 500, 10, False)


def _safety(N, D, L, step, ratios, tempos):
    x = tr.signal(L, 7)
    nan = np.full(3 * N + 50, np.nan, dtype=np.float32)
    told_apart = 0
    for r in ratios:
        for t in tempos:
            full, s_full = pr.pitch(x, t, r, N, D)
            pl = pr.plan(L, t, r, N)
            for n in range(0, L + 1, step):
                K, F = ps.emitted(n, t, r, N, D, False), ps.frames(n, t, r, N, D, False)
                assert K <= full.size and K <= pr.plan(n, t, r, N)["n_out"]
                for tail in (x[:0], nan):   # the stream ends at n; anything may follow
                    o, s = pr.pitch(np.concatenate([x[:n], tail]), t, r, N, D)
                    assert np.array_equal(_bits(o[:K]), _bits(full[:K])), (t, r, n, tail.size)
                    if pl["P"] != pl["Q"]:
                        assert np.array_equal(s[:F], s_full[:F])
                # the wrong variant emits ceil(E up / down) outputs, the last of them summed against an edge that is not there
                E, Kw = ps.stretched(n, t, r, N, D, False), ps.emitted(n, t, r, N, D, False, wrong="reach")
                if K < Kw <= full.size:
                    z = pr.stretched(x, t, r, N, D)[:E]
                    told_apart += not np.array_equal(_bits(pr._resample(z, pl["up"], pl["down"])[:Kw]), _bits(full[:Kw]))
    return told_apart


@pytest.mark.parametrize("N,D,step", [(16, 3, 7), (64, 8, 41)])
def test_what_a_stream_has_emitted_does_not_depend_on_what_follows(N, D, step):
    """the reference alone: the first K(n) outputs of ``pitch_ref.pitch`` are those of the whole row whether the input ends at n
    or NaNs follow it; and a variant that ignores the filter's reach differs on this signal, so the comparison can tell"""
    assert _safety(N, D, 8 * N + 37, step, RATIOS[:4], TEMPOS) > 0
    assert _safety(N, D, 6 * N + 5, 4 * step + 1, RATIOS[4:], TEMPOS[:2]) > 0


def test_the_long_filter_at_the_default_frame():
    assert _safety(512, 240, 6 * 512 + 40, 997, [(199, 100), (28, 25)], [(1, 1)]) > 0


def test_stream_reference_cuts_the_batch_result_and_the_wrong_variant_differs():
    x = tr.signal(20 * 64 + 37, 3)
    cuts = [1, 0, 500, 300, 516, 0]
    pieces, places = ps.stream(x, cuts, (5, 4), (28, 25), 64, 8)
    out, s = pr.pitch(x, (5, 4), (28, 25), 64, 8)
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(out)) and np.array_equal(np.concatenate(places), s)
    assert pieces[0].size == 0 and pieces[2].size > 0 and sum(p.size for p in pieces) == audio.tempo_len(x.size, 5, 4)
    wrong, _ = ps.stream(x, cuts, (5, 4), (28, 25), 64, 8, wrong="reach")
    assert [p.size for p in wrong] != [p.size for p in pieces]
    one, _ = ps.stream(x, [7, 1300, 10], (1, 1), (1, 1), 64, 8)
    assert [p.size for p in one] == [7, 1300, 10] and np.array_equal(_bits(np.concatenate(one)), _bits(x))


class _FakeLib:
    """records what StreamPitch sends to the library"""

    def __init__(self):
        self.created, self.opened, self.pushes, self.destroyed = [], [], [], 0

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_pitchs_create(self, max_streams, max_chunk, N, D, win, max_taps, href):
        self.created.append((max_streams, max_chunk, N, D, max_taps, [win[i] for i in range(N)]))
        href._obj.value = 4321
        return 0

    def smi_pitchs_destroy(self, h):
        self.destroyed += 1
        return 0

    def smi_pitchs_open(self, h, slot, tp, tq, rp, rq, taps, n_taps, stream):
        self.opened.append((slot, tp, tq, rp, rq, n_taps, None if n_taps == 0 else [taps[i] for i in range(n_taps)]))
        return 0

    def smi_pitchs_push_rows(self, h, src, stride, streams, lens, lasts, B, pos, pos_stride, dst, out_stride, n_out, stream):
        assert len(set(streams[:B])) == B, "a stream twice in one call"
        self.pushes.append((list(streams[:B]), list(lens[:B]), list(lasts[:B]), out_stride))
        return 0


def test_stream_pitch_slots_with_a_stand_in_library():
    fake = _FakeLib()
    t = audio.StreamPitch(3, 4000, (64, 8), lib=fake)
    assert fake.created[0][:5] == (3, 4000, 64, 8, audio.PITCH_STREAM_TAPS) and np.array_equal(fake.created[0][5], tr.window(64))
    assert t.history == streaming.tempo_history(64, 8) == 232 and t.max_chunk == 4000
    assert t.open("a", tempo=(5, 4), pitch=(28, 25)) == 0 and t.open("b", pitch=(2, 3)) == 1
    with pytest.raises(ValueError):
        t.open("a", (5, 4), (28, 25))
    # the taps are resample_taps(up, down) = (rq, rp) in lowest terms, rounded to fp32 once
    assert fake.opened[0][:6] == (0, 5, 4, 28, 25, 561) and fake.opened[1][:6] == (1, 1, 1, 2, 3, 61)
    assert np.array_equal(_bits(fake.opened[0][6]), _bits(pr.taps32(25, 28)))
    rows = [("a", 300, False), ("b", 300, False), ("c", 40, True)]
    want = t.piece_lengths(rows)
    _, lens = t.push(None, rows)
    assert lens == want == [ps.emitted(300, (5, 4), (28, 25), 64, 8, False), ps.emitted(300, (1, 1), (2, 3), 64, 8, False), 40]
    assert 0 < lens[0] < 240 and 0 < lens[1] < 300                # a stream never opened copies at 1/1 and 1/1
    assert fake.opened[2] == (2, 1, 1, 1, 1, 0, None) and t.calls == 1
    assert t.slot("c") is None and t.slot("a") == 0 and t.slot("b") == 1
    assert max(lens) <= t.longest()
    # a's last chunk and its empty flush in one poll: two calls; the freed slots are used again
    _, lens = t.push(None, [("a", 500, False), ("a", 0, True), ("b", 10, False), ("d", 12, False)])
    assert t.calls == 3 and [p[0] for p in fake.pushes[1:]] == [[0], [0, 1, 2]]
    assert want[0] + sum(lens[:2]) == audio.tempo_len(800, 5, 4) and lens[3] == 12
    assert t.slot("a") is None and t.slot("d") == 2
    t.open("e", (2, 1), (2, 1))                                 # the stretch is 1/1: a copy, resampled
    assert t.slot("e") == 0 and fake.opened[-1][:6] == (0, 2, 1, 2, 1, 41)
    with pytest.raises(ValueError):
        t.push(None, [("f", 12, False)])                       # a fourth open request
    with pytest.raises(ValueError):
        t.push(None, [("b", 4001, False)])                     # beyond max_chunk: refused before the library is called
    assert t.calls == 3
    t.reset()
    assert t.slot("b") is None and t.open("g", (1, 2)) == 0
    t.close()
    assert fake.destroyed == 1


def test_the_pipeline_refuses_without_a_device():
    from sparkmi.pipeline import SparkTTS
    tts = object.__new__(SparkTTS)
    for call, args in ((tts.inference_stream, ("text",)), (tts.serve_stream, ([{"text": "a"}],))):
        with pytest.raises(ValueError, match="stream_pitch_shift"):
            next(iter(call(*args, stream_pitch_shift=2.0)))                 # not joined
        with pytest.raises(ValueError, match="the batch calls take it"):
            next(iter(call(*args, joined=True, pitch_shift=2.0)))           # the batch keyword stays refused
    for bad in (13, -12.5, float("nan"), "2", True):
        with pytest.raises(ValueError, match="stream_pitch_shift"):
            SparkTTS._stream_pitch_ratios([{}], bad)
        with pytest.raises(ValueError, match="request 3: stream_pitch_shift"):
            SparkTTS._stream_pitch_ratios([{"stream_pitch_shift": bad}], None, first=3)
    assert SparkTTS._stream_pitch_ratios([{}, {"stream_pitch_shift": 0}, {"stream_pitch_shift": 0.05}, {"stream_pitch_shift": -2}], 2) == \
        [(28, 25), None, None, (89, 100)]
