"""The host side of the pitch shift (include/sparkmi.h, smi_pitch_layout; sparkmi/audio.py, pitch_ratio) and its reference
tests/pitch_ref.py: the ratios, the plan's integers, the length claim, the identities, what a shift does to a tone, and that the
reference tells the wrong variants apart.  No GPU."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pitch_ref as R
import tempo_ref
from sparkmi import _lib
from sparkmi.audio import pitch_ratio, tempo_ratio

N, D = 512, 240      # the production frame at 16 kHz
TEMPOS = ((1, 1), (5, 4), (4, 5), (2, 1), (1, 2), (133, 100))


def test_pitch_ratio_values():
    assert pitch_ratio(2) == (28, 25) and pitch_ratio(-2) == (89, 100) and pitch_ratio(7) == (3, 2) and pitch_ratio(12) == (2, 1)
    assert pitch_ratio(-12) == (1, 2) and pitch_ratio(0) == (1, 1) and pitch_ratio(0.0) == (1, 1) and pitch_ratio(np.float32(4)) == (63, 50)
    assert pitch_ratio(0.05) == (1, 1)      # below the resolution: a hundredth of the ratio is about 17 cents here
    for s in np.linspace(-12, 12, 97):
        p, q = pitch_ratio(float(s))
        assert math.gcd(p, q) == 1 and p / q == round(2 ** (s / 12) * 100) / 100 and 0.5 <= p / q <= 2.0


@pytest.mark.parametrize("bad", [True, "2", None, [2], float("nan"), float("inf"), 12.01, -12.5, 1 + 2j])
def test_pitch_ratio_errors(bad):
    with pytest.raises(ValueError, match="pitch_shift"):
        pitch_ratio(bad)
    with pytest.raises(ValueError):      # the same type and finiteness checks as tempo_ratio
        tempo_ratio(bad)


def _layout(L, t, r, n):
    P, Q, up, down = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    M, K = C.c_longlong(-1), C.c_longlong(-1)
    n_out = _lib.lib().smi_pitch_layout(L, t[0], t[1], r[0], r[1], n, C.byref(P), C.byref(Q), C.byref(M), C.byref(K), C.byref(up), C.byref(down))
    return dict(n_out=n_out, P=P.value, Q=Q.value, M=M.value, K=K.value, up=up.value, down=down.value)


@pytest.mark.parametrize("n", [16, 64, 512])
def test_layout_against_plan(n):
    H = n // 2
    lengths = sorted({0, 1, 2, H - 1, H, H + 1, n, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 1, 48000})
    for r in ((3, 2), (2, 3), (28, 25), (89, 100), (199, 100), (1, 1), (1, 2), (2, 1)):
        for t in TEMPOS:
            for L in lengths:
                assert _layout(L, t, r, n) == R.plan(L, t, r, n), (L, t, r, n)
    # ratios that are not in lowest terms give the same plan; null out-pointers are allowed
    assert _layout(1000, (10, 8), (6, 4), n) == R.plan(1000, (5, 4), (3, 2), n)
    assert _lib.lib().smi_pitch_layout(1000, 5, 4, 3, 2, n, None, None, None, None, None, None) == 800


def test_layout_bad_arguments():
    f = _lib.lib().smi_pitch_layout
    none = (None,) * 6
    assert f(100, 1, 1, 3, 2, 512, *none) == 100
    for args in ((-1, 1, 1, 3, 2, 512), ((1 << 24) + 1, 1, 1, 3, 2, 512), (100, 0, 1, 3, 2, 512), (100, 1, 0, 3, 2, 512), (100, 1, 1, 0, 2, 512),
                 (100, 1, 1, 3, 0, 512), (100, 1, 1, 3, 2, 14), (100, 1, 1, 3, 2, 511), (100, 1, 1, 3, 2, 2050), (100, 32768, 1, 3, 2, 512),
                 (100, 1, 1, 9, 2, 512),        # a stretch of 2/9: below 1/4
                 (100, 4, 1, 1, 2, 512),        # a stretch of 8
                 (100, 211, 199, 197, 193, 512)):   # lowest terms above 32767
        assert f(*args, *none) == -1, args


def test_the_stretched_span_always_resamples_to_at_least_n_out():
    """ceil(M up / down) >= n_out for every hundredth ratio, with a surplus of 0 .. 2 samples: the claim the cut rests on"""
    lengths = list(range(0, 40)) + [255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096, 4097, 16000, 48000, 48001, 160000, 1 << 20, 1 << 24]
    worst = 0
    for c in range(50, 201):
        g = math.gcd(c, 100)
        r = (c // g, 100 // g)
        for t in TEMPOS:
            for L in lengths:
                pl = R.plan(L, t, r, N)
                assert max(pl["P"], pl["Q"]) <= 20000 and pl["P"] <= 4 * pl["Q"] and pl["Q"] <= 4 * pl["P"]
                surplus = -((-pl["M"] * pl["up"]) // pl["down"]) - pl["n_out"]
                assert 0 <= surplus <= 2, (L, t, r, pl)
                worst = max(worst, surplus)
    assert worst == 2


@functools.lru_cache(maxsize=None)
def _noise(L=3000):
    x = tempo_ref.signal(L, 21)
    x.setflags(write=False)
    return x


def test_identities():
    x = _noise()
    y, s = R.pitch(x, (1, 1), (1, 1), 64, 8)
    assert np.array_equal(y.view(np.uint32), x.view(np.uint32)) and np.array_equal(s, 32 * np.arange(s.size))
    for t in ((5, 4), (2, 3)):
        want, places = tempo_ref.tempo(x, t[0], t[1], 64, 8)
        y, s = R.pitch(x, t, (1, 1), 64, 8)
        assert np.array_equal(y.view(np.uint32), want.view(np.uint32)) and np.array_equal(s, places)


@functools.lru_cache(maxsize=None)
def _tone():
    x = R.tone(16000)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("semitones,want", [(-5, 194), (-2, 163), (2, 130), (4, 115), (7, 97)])
def test_a_tone_keeps_its_length_and_moves_its_period(semitones, want):
    r = pitch_ratio(semitones)
    assert want == round(16000 / 110.0 / (r[0] / r[1]))
    y, _ = R.pitch(_tone(), (1, 1), r, N, D)
    assert y.size == 16000
    assert abs(R.period(y) - want) <= 1, (semitones, R.period(y))
    assert abs(R.period(_tone()) - 145) <= 1


def test_tempo_and_pitch_in_one_pass():
    y, _ = R.pitch(_tone(), tempo_ratio(1.25), pitch_ratio(3), N, D)
    assert y.size == 12800
    assert abs(R.period(y) - 122) <= 1, R.period(y)


def test_the_reference_rejects_the_wrong_variants():
    x = _noise()[:2995]
    t, r = (5, 4), (28, 25)
    pl = R.plan(x.size, t, r, 64)
    assert -((-pl["M"] * pl["up"]) // pl["down"]) > pl["n_out"] and pl["M"] % 32      # a surplus to cut, a last frame cut short
    good, s = R.pitch(x, t, r, 64, 8)
    assert good.size == pl["n_out"] == 2396
    cut, _ = R.pitch(x, t, r, 64, 8, wrong="cut")
    assert cut.size != good.size and np.array_equal(cut[: good.size], good)
    edge, _ = R.pitch(x, t, r, 64, 8, wrong="edge")
    assert edge.size == good.size and not np.array_equal(edge, good)
    first = int(np.flatnonzero(edge != good)[0])
    assert first >= good.size - 2 * (10 * 28 + 32)      # only the sums that reach past M differ
    two, _ = R.pitch(x, t, r, 64, 8, wrong="two_pass")
    assert two.size == good.size and not np.array_equal(two, good)
