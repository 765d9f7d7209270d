"""The limiter of joined streams, host side (tests/limit_stream_ref.py; smi_limits_piece_len; sparkmi/streaming.py:
limiter_piece_len): the emission arithmetic; the prefix property that the whole design rests on -- the limiter of a prefix x[:n]
equals the limiter of the whole row on [0, E(n)), bit for bit --; the carried-state model against the batch reference for every
chunking the GPU test uses; that the committed cases tell the wrong variants apart; the refusals a host can check.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import limit_ref as LR
import limit_stream_ref as S
from sparkmi import audio, streaming

EINVAL = -1   # include/sparkmi.h, SMI_EINVAL


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cuts(rng, total, m):
    at = np.sort(rng.integers(0, total + 1, size=m - 1))
    return np.diff(np.concatenate([[0], at, [total]])).astype(int).tolist()


@pytest.mark.parametrize("A,R", S.REACHES)
def test_piece_lengths_against_the_reference_and_the_library(A, R):
    from sparkmi import _lib
    l = _lib.lib()
    W = A + R
    rng = np.random.default_rng(1000 * A + R)
    zero_pieces = 0
    for trial in range(40):
        total = int(rng.integers(0, 4 * (W + 10) + 17))
        cuts = _cuts(rng, total, int(rng.integers(1, 14)))
        n = out = 0
        for i, c in enumerate(cuts):
            last = i == len(cuts) - 1
            piece, n1 = S.piece_len(A, R, n, c, last)
            assert streaming.limiter_piece_len(A, R, n, c, last) == (piece, n1)
            na = C.c_longlong(-7)
            assert l.smi_limits_piece_len(A, R, n, c, int(last), C.byref(na)) == piece and na.value == n1
            out += piece
            # sample i leaves once n >= i + A + R + 11, and no later
            assert last or out == max(0, n1 - (W + 10)) == streaming.limiter_emitted(n1, A, R)
            zero_pieces += piece == 0 and c > 0
            n = n1
        assert out == total                                  # the stage delays pieces and keeps the total
    assert zero_pieces > 0
    for L in (0, 1, W + 9, W + 10, W + 11):                  # single pushes
        assert S.piece_len(A, R, 0, L, False) == (1 if L == W + 11 else 0, L)
        assert S.piece_len(A, R, 0, L, True) == (L, L)
        assert l.smi_limits_piece_len(A, R, 0, L, 0, None) == (1 if L == W + 11 else 0)
        assert l.smi_limits_piece_len(A, R, 0, L, 1, None) == L
        assert streaming.limiter_piece_len(A, R, 0, L, True) == (L, L)
    for bad in ((-1, R, 0, 10, 0), (257, R, 0, 10, 0), (A, -1, 0, 10, 0), (A, 2049, 0, 10, 0), (A, R, -1, 10, 0), (A, R, 0, -1, 0),
                (A, R, 0, 10, 2), (A, R, 1 << 28, 1, 0), (A, R, 0, (1 << 28) + 1, 1)):
        assert l.smi_limits_piece_len(*bad, None) == -1, bad
    assert l.smi_limits_piece_len(A, R, (1 << 28) - 1, 1, 0, None) >= 0
    for bad in ((-1, R, 0, 10, False), (257, R, 0, 10, False), (A, 2049, 0, 10, False), (A, R, -1, 10, False), (A, R, 0, -1, True)):
        with pytest.raises(ValueError):
            streaming.limiter_piece_len(*bad)


def _spread(c):
    """lengths n of a prefix: around the reach, around a tile, the push edges of the "edge" cases, near the end"""
    L, W = c["x"].size, c["A"] + c["R"]
    ns = {W + 10, W + 11, W + 12, 2 * W + 21, S.edge_of(c["A"], c["R"]), 1024, 1025 + W, L - 1, L - W - 11, L // 2, (2 * L) // 3}
    return sorted(n for n in ns if 0 < n < L)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("A,R", S.REACHES)
def test_the_limiter_of_a_prefix_is_final_on_what_the_stream_emits(A, R, mode):
    """out[i] reads x up to i + A + R + 10 and no further: the property the streaming form rests on, bit for bit in the samples
    and in the float64 s -- and one sample further it does not hold for every case (the bound is not slack)"""
    w, h = audio.limiter_window(A, R), S.taps_of(mode)
    checked = beyond = 0
    for c in S.reference():
        if (c["A"], c["R"], c["mode"]) != (A, R, mode):
            continue
        for n in _spread(c):
            p = LR.limit(c["x"][:n], 1.0, c["ceiling"], h, A, R, w)
            E = S.emitted(n, A, R)
            assert np.array_equal(_bits(p["out"][:E]), _bits(c["want"]["out"][:E])), (c["name"], n)
            assert np.array_equal(p["s"][:E], c["want"]["s"][:E]), (c["name"], n)
            assert np.array_equal(p["e"][:E], c["want"]["e"][:E]), (c["name"], n)
            checked += E > 0
            beyond += not np.array_equal(p["s"][: E + 1], c["want"]["s"][: E + 1])
    assert checked >= 20
    if mode == "true":
        assert beyond > 0                                    # sample E(n) is not final: the interpolator reads the sample at n


@pytest.mark.parametrize("A,R", S.REACHES)
def test_the_carried_state_model_is_the_batch_reference_for_every_chunking(A, R):
    pushes = 0
    for c in S.reference():
        if (c["A"], c["R"]) != (A, R):
            continue
        for name, p in S.chunkings(c).items():
            r = S.run_stream(c, p)
            assert np.array_equal(_bits(r["out"]), _bits(c["want"]["out"])), (c["name"], name)
            assert np.array_equal(r["s"], c["want"]["s"]) and np.array_equal(r["stats"], c["want"]["stats"]), (c["name"], name)
            assert r["pieces"] == [S.piece_len(A, R, sum(p[:t]), p[t], t == len(p) - 1)[0] for t in range(len(p))]
            assert r["held"] <= 2 * (A + R) + 19               # the bound on the history (include/sparkmi.h)
            assert not r["out"].size or float(np.abs(r["out"]).max()) <= c["ceiling"]
            pushes += len(p)
    assert pushes > 500


def test_the_history_reaches_its_bound_and_the_stats_follow_n_alone():
    c = S.case("A40_R400_true_hot")
    r = S.run_stream(c, S._split(c["x"].size, 129))
    assert r["held"] == 2 * 440 + 19
    a, b = S.run_stream(c, [700, 300, c["x"].size - 1000]), S.run_stream(c, [999, 1, c["x"].size - 1000])
    assert np.array_equal(a["stats_after"][1], b["stats_after"][1])          # n = 1000 either way
    assert not np.array_equal(a["stats_after"][0], a["stats_after"][1])
    E = S.emitted(1000, 40, 400)
    w = c["want"]
    assert np.array_equal(a["stats_after"][1], [w["e"][:E].max(), 1.0, w["s"][:E].min(), np.count_nonzero(w["s"][:E] < 1.0)])


@pytest.mark.parametrize("variant,name,chunking", [
    ("drop_history", "A40_R400_true_hot", "129"),
    ("drop_history", "A3_R5_sample_edge", "edge"),
    ("short_history", "A40_R400_true_edge", "edge"),
    ("short_history", "A256_R2048_sample_edge", "edge"),
    ("early", "A40_R400_true_edge", "edge"),
    ("early", "A0_R0_true_edge", "edge"),
    ("stats_last", "A40_R400_true_hot", "129"),
    ("stats_last", "A3_R5_sample_first_last", "251"),
])
def test_the_committed_cases_tell_the_wrong_variants_apart(variant, name, chunking):
    c = S.case(name)
    p = S.chunkings(c)[chunking]
    assert len(p) > 1
    good, bad = S.run_stream(c, p), S.run_stream(c, p, variant=variant)
    assert np.array_equal(_bits(good["out"]), _bits(c["want"]["out"])) and np.array_equal(good["stats"], c["want"]["stats"])
    if variant == "stats_last":
        assert np.array_equal(_bits(bad["out"]), _bits(c["want"]["out"]))     # the samples are right, the stats are not
        assert not np.array_equal(bad["stats"], c["want"]["stats"])
    else:
        assert bad["out"].size == c["want"]["out"].size
        moved = int(np.count_nonzero(_bits(bad["out"]) != _bits(c["want"]["out"])))
        print(f"{variant} on {name} pushed by {chunking}: {moved} of {bad['out'].size} samples differ")
        assert moved > 0


def test_the_early_variant_is_harmless_in_the_sample_mode_only():
    """the sample-peak mode reads no neighbour, so E = n - (A + R) would do there; one rule serves both modes all the same"""
    c = S.case("A40_R400_sample_hot")
    bad = S.run_stream(c, S.chunkings(c)["129"], variant="early")
    assert np.array_equal(_bits(bad["out"]), _bits(c["want"]["out"]))


def test_refusals_that_follow_no_pointer():
    from sparkmi import _lib
    l = _lib.lib()
    A, R = 3, 5
    win = np.ascontiguousarray(audio.limiter_window(A, R), dtype=np.float64)
    taps = LR.taps()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    h = C.c_void_p()

    def create(what, max_streams=4, max_chunk=100, A=A, R=R, win=win, taps=taps, n_taps=None, phases=LR.PHASES, out=True):
        n_taps = (0 if taps is None else taps.size) if n_taps is None else n_taps
        rc = l.smi_limits_create(max_streams, max_chunk, A, R, dp(win), dp(taps), n_taps, phases, C.byref(h) if out else None)
        assert rc == EINVAL and what in l.smi_last_error().decode(), (what, rc, l.smi_last_error())
        assert not h.value

    create("null out", out=False)
    create("max_streams=0", max_streams=0)
    create("max_streams=4097", max_streams=4097)
    create("max_chunk=0", max_chunk=0)
    create("max_chunk=16777217", max_chunk=(1 << 24) + 1)
    create("lookahead=-1", A=-1)
    create("lookahead=257", A=257, win=np.ones(3000) / 3000)
    create("release=-1", R=-1)
    create("release=2049", R=2049, win=np.ones(3000) / 3000)
    create("phases=0", phases=0)
    create("phases=9", phases=9)
    create("n_taps=80", n_taps=80)
    create("null taps_host", taps=None, n_taps=81)
    bad = taps.copy()
    bad[7] = np.inf
    create("taps[7]", taps=bad)
    create("null win_host", win=None)
    bad = win.copy()
    bad[2] = -bad[2]
    create("win[2]", win=bad)
    bad = win.copy()
    bad[1] = np.nan
    create("win[1]", win=bad)
    create("win sums to", win=win * (1 + 1e-9))
    # a null handle, and the null pointers of a push
    assert l.smi_limits_open(None, 0, 1, 0.5) == EINVAL and "null handle" in l.smi_last_error().decode()
    one = (C.c_int32 * 1)(0)
    assert l.smi_limits_push_rows(None, None, 1, one, one, one, 1, None, 1, None, None, None) == EINVAL
    assert "null argument" in l.smi_last_error().decode()
    assert l.smi_limits_destroy(None) == 0


class _FakeLib:
    """a stand-in for the library: it fills the pieces' lengths with the reference's arithmetic and records the calls"""

    def __init__(self, A, R):
        self.A, self.R, self.n, self.opened, self.pushes = A, R, {}, [], []

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_limits_create(self, max_streams, max_chunk, A, R, win, taps, n_taps, phases, out):
        assert (A, R) == (self.A, self.R) and n_taps == 20 * phases + 1
        return 0

    def smi_limits_destroy(self, h):
        return 0

    def smi_limits_open(self, h, slot, true_peak, ceiling):
        self.n[slot] = 0
        self.opened.append((slot, true_peak, ceiling))
        return 0

    def smi_limits_push_rows(self, h, src, stride, slots, lens, lasts, B, dst, ostride, got, stats, stream):
        assert len(set(slots[:B])) == B          # a stream at most once in a call
        for b in range(B):
            got[b], self.n[slots[b]] = S.piece_len(self.A, self.R, self.n[slots[b]], lens[b], lasts[b])
        self.pushes.append([(slots[b], lens[b], lasts[b]) for b in range(B)])
        return 0


def test_stream_limiter_bookkeeping_with_a_stand_in_library():
    fake = _FakeLib(40, 400)
    sl = audio.StreamLimiter(2, 1000, lib=fake)
    assert (sl.lookahead, sl.release, sl.delay) == (40, 400, 450)
    sl.open("a", "sample", 0.5)
    with pytest.raises(ValueError, match="already open"):
        sl.open("a")
    with pytest.raises(ValueError, match="mode"):
        sl.open("z", "peak")
    assert sl.piece_lengths([("a", 500, False), ("b", 450, False), ("a", 0, True)]) == [50, 0, 450]
    out, lens = sl.push(None, [("a", 500, False), ("b", 450, False), ("a", 0, True)])     # "a" twice: two device calls
    assert lens == [50, 0, 450] and sl.calls == 2 and fake.pushes == [[(0, 500, 0), (1, 450, 0)], [(0, 0, 1)]]
    assert fake.opened == [(0, 0, 0.5), (1, 1, audio.PEAK_CEILING)]       # a key met unopened: the true-peak mode at the default ceiling
    assert sl.slot("a") is None and sl.slot("b") == 1
    sl.open("c")                                 # slot 0 is free again
    assert sl.slot("c") == 0
    with pytest.raises(ValueError, match="slots are in use"):
        sl.open("d")
    with pytest.raises(ValueError, match="max_chunk"):
        sl.push(None, [("b", 1001, False)])
    assert sl.push(None, [("b", 1, True)])[1] == [451]
    sl.reset()
    assert sl.slot("c") is None and sorted(sl._free) == [0, 1]
    sl8 = audio.StreamLimiter(1, 10, sr=24000, lookahead_ms=1.0, release_ms=10.0, lib=_FakeLib(24, 240))
    assert sl8.delay == 274
