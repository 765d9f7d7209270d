"""The tempo arithmetic on the host: sparkmi.audio's helpers, smi_tempo_layout through the library against tests/tempo_ref.py,
and the properties of the reference itself that the GPU tests rely on."""
import ctypes as C
import math

import numpy as np
import pytest

import tempo_ref as R
from sparkmi import _lib
from sparkmi.audio import tempo_frame, tempo_len, tempo_ratio, tempo_window


def test_tempo_ratio_values_and_errors():
    assert tempo_ratio(1.25) == (5, 4) and tempo_ratio(0.8) == (4, 5) and tempo_ratio(1.0) == (1, 1) and tempo_ratio(1) == (1, 1)
    assert tempo_ratio(2.0) == (2, 1) and tempo_ratio(0.5) == (1, 2) and tempo_ratio(1.5) == (3, 2)
    assert tempo_ratio(1.33) == (133, 100) and tempo_ratio(0.999) == (1, 1) and tempo_ratio(np.float32(1.25)) == (5, 4)
    for bad in (0.49, 2.01, 0.0, -1.0, math.nan, math.inf, -math.inf, "1.25", None, True):
        with pytest.raises(ValueError):
            tempo_ratio(bad)


def test_frame_and_window():
    assert tempo_frame(16000) == (512, 240) and tempo_frame(24000) == (768, 360) and tempo_frame(8000) == (256, 120)
    for N in (16, 64, 512, 2048):
        w = tempo_window(N)
        assert w.dtype == np.float64 and np.array_equal(w, R.window(N)) and w[0] == 0.0
        assert np.max(np.abs(w[: N // 2] + w[N // 2:] - 1.0)) < 1e-15
    with pytest.raises(ValueError):
        tempo_window(15)


@pytest.mark.parametrize("N", [16, 64, 512])
def test_layout_matches_the_reference(N):
    l = _lib.lib()
    H = N // 2
    for L in (0, 1, H - 1, H, H + 1, 1000):
        for p, q in ((1, 1), (5, 4), (4, 5), (3, 2), (2, 3), (2, 1), (1, 2), (133, 100), (4, 1), (1, 4)):
            K = C.c_longlong(-7)
            M = l.smi_tempo_layout(L, p, q, N, C.byref(K))
            assert (M, K.value) == R.layout(L, p, q, N), (L, p, q, N)
            assert M == tempo_len(L, p, q) and l.smi_tempo_layout(L, p, q, N, None) == M
    for bad in ((-1, 1, 1, N), ((1 << 24) + 1, 1, 1, N), (10, 0, 1, N), (10, 1, 0, N), (10, 32768, 32767, N), (10, 9, 2, N), (10, 2, 9, N),
                (10, 1, 1, N + 1), (10, 1, 1, 14), (10, 1, 1, 2050)):
        assert l.smi_tempo_layout(*bad, None) == -1, bad


def test_quantise_rounds_half_to_even_and_clamps():
    x = np.array([0.0, 1.0, -1.0, 2.0, -3.0, 0.5 / 32767, 1.5 / 32767, 2.5 / 32767, np.nan, np.inf, -np.inf], dtype=np.float32)
    q = R.quantise(x)
    assert q.dtype == np.int64 and q[:5].tolist() == [0, 32767, -32767, 32767, -32767] and q[8:].tolist() == [0, 32767, -32767]
    # the only exact halves in range are +-0.5 -> +-16383.5, which go to the even +-16384
    assert R.quantise(np.array([0.5, -0.5, 0.25, 2.0 ** -16], dtype=np.float32)).tolist() == [16384, -16384, 8192, 0]


@pytest.mark.parametrize("N,D,L", [(16, 3, 200), (64, 8, 1000), (512, 240, 8000)])
def test_identity_at_one_is_bit_exact(N, D, L):
    x = R.signal(L, seed=L)
    for p, q in ((1, 1), (7, 7)):
        out, s = R.tempo(x, p, q, N, D)
        assert np.array_equal(s, np.arange(s.size) * (N // 2))
        assert np.array_equal(out.view(np.uint32), x.view(np.uint32))


def _period(y, lo, hi):
    """the lag in [lo, hi) at which y's autocorrelation is largest"""
    y = y.astype(np.float64) - np.mean(y)
    ac = [float(np.dot(y[:-lag], y[lag:])) / (y.size - lag) for lag in range(lo, hi)]
    return lo + int(np.argmax(ac))


def test_a_stationary_tone_keeps_its_period():
    sr, f0 = 16000, 110.0
    t = np.arange(sr, dtype=np.float64) / sr
    x = sum(np.sin(2 * np.pi * f0 * h * t) / h for h in range(1, 8))
    x = (0.5 * x / np.max(np.abs(x))).astype(np.float32)
    want = _period(x, 80, 220)
    assert abs(want - sr / f0) <= 1
    for p, q in ((5, 4), (4, 5)):
        out, s = R.tempo(x, p, q, 512, 240)
        assert out.size == R.layout(x.size, p, q, 512)[0]
        body = out[512: out.size - 1024]        # away from the edges, where frames reach past the span
        assert abs(_period(body, 80, 220) - want) <= 1, (p, q)


def test_every_frame_is_searched_at_three_halves_with_a_short_radius():
    """N = 64, D = 8 at 3/2: the nominal step (48) leaves the natural one (32) by 16 = 2 D a frame, so t_k - a_k lies in
    [-3 D, -D] and the shortcut applies only behind a frame that ended at the range's very edge, delta = +D.  On the tests' own
    signal no frame does: every frame k >= 1 takes the search branch, which the GPU shapes rely on.  At N = 16, D = 3 the step
    differs by 4 < 2 D and some frames keep their natural place: most are searched."""
    for N, D, L in ((64, 8, 1000), (16, 3, 200)):
        x = R.signal(L, seed=7)
        searched = []
        _, s = R.tempo(x, 3, 2, N, D, searched)
        if N == 64:
            assert searched == list(range(1, s.size)), (N, searched)
        else:
            assert len(searched) >= (s.size - 1) * 3 // 4
        a = (np.arange(s.size) * (N // 2) * 3) // 2
        assert np.all(np.abs(s - a) <= D)


def test_ties_go_to_the_nearest_then_the_smaller_delta():
    N, D = 16, 3
    z, s = R.tempo(np.zeros(200, dtype=np.float32), 3, 2, N, D)
    assert not z.any()
    # every candidate is at distance 0: the nearest to t_k wins -- delta = -D when t_k lies below a_k - D
    H = N // 2
    for k in range(1, s.size):
        a, t = (k * H * 3) // 2, int(s[k - 1]) + H
        assert s[k] == (t if abs(t - a) <= D else (a - D if t < a else a + D))
