"""Numpy-only restatement of include/sparkmi.h's tempo section (smi_tempo_layout, smi_tempo_rows): WSOLA with an exact integer
search, in int64 and float64 alone.  ``tempo`` returns the frame places as well as the samples, and the tests hold the device
to both bit for bit: the search's distances are integers, so there is no tolerance to derive."""
import numpy as np


def window(N):
    """w[i] = 0.5 - 0.5 cos(2 pi i / N), float64 (sparkmi.audio.tempo_window states the same; the tests compare the two)"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(N), dtype=np.float64) / int(N))


def layout(L, p, q, N):
    """(M, K): the output samples and the frames of a span of L samples at tempo p / q"""
    L, p, q, H = int(L), int(p), int(q), int(N) // 2
    M = -((-L * q) // p)
    return M, ((M - 1) // H + 1 if M else 0)


def quantise(x):
    """int64 [L]: clamp(rint(fl64(x) * 32767), +-32767), half to even; a NaN gives 0"""
    v = np.asarray(x, dtype=np.float32).astype(np.float64) * 32767.0
    nan = np.isnan(v)
    return np.where(nan, 0.0, np.clip(np.rint(np.where(nan, 0.0, v)), -32767.0, 32767.0)).astype(np.int64)


def _take(a, first, count):
    """a[first .. first + count) with zeros outside a's own range"""
    out = np.zeros(count, dtype=a.dtype)
    lo, hi = max(0, first), min(a.size, first + count)
    if hi > lo:
        out[lo - first: hi - first] = a[lo:hi]
    return out


def positions(x, p, q, N, D, searched=None):
    """int64 [K]: s_k.  ``searched`` (a list) receives the k of every frame that took the search branch."""
    x = np.asarray(x, dtype=np.float32)
    p, q, N, D = int(p), int(q), int(N), int(D)
    H = N // 2
    _, K = layout(x.size, p, q, N)
    qx = quantise(x)
    s = np.zeros(K, dtype=np.int64)
    deltas = np.arange(-D, D + 1, dtype=np.int64)
    for k in range(1, K):
        a = (k * H * p) // q
        t = int(s[k - 1]) + H
        if abs(t - a) <= D:
            s[k] = t      # what the search returns: distance 0, nothing closer to t
            continue
        if searched is not None:
            searched.append(k)
        target = _take(qx, t, N)
        cand = _take(qx, a - D, N + 2 * D)
        windows = np.lib.stride_tricks.sliding_window_view(cand, N)      # [2 D + 1][N]
        dist = np.sum((target[None, :] - windows) ** 2, axis=1, dtype=np.int64)
        near = np.abs(a + deltas - t)
        best = np.lexsort((deltas, near, dist))[0]                       # distance, then |a + delta - t|, then delta
        s[k] = a + int(deltas[best])
    return s


def tempo(x, p, q, N, D, searched=None):
    """(out float32 [M], s int64 [K]) of the span ``x`` at tempo p / q"""
    x = np.asarray(x, dtype=np.float32)
    N = int(N)
    H = N // 2
    M, K = layout(x.size, p, q, N)
    s = positions(x, p, q, N, D, searched)
    w = window(N)
    xd = x.astype(np.float64)
    out = np.zeros(M, dtype=np.float32)
    for k in range(K):
        m0, cnt = k * H, min(H, M - k * H)
        if k == 0:
            out[:cnt] = _take(x, 0, cnt)
            continue
        u0 = _take(xd, int(s[k]), cnt) * w[:cnt]
        u1 = _take(xd, int(s[k - 1]) + H, cnt) * w[H: H + cnt]
        out[m0: m0 + cnt] = (u0 + u1).astype(np.float32)
    return out, s


def signal(L, seed, f0=110.0, sr=16000, amp=0.9):
    """seeded noise plus a tone, |x| <= amp: float32 [L]"""
    rng = np.random.default_rng(seed)
    t = np.arange(int(L), dtype=np.float64) / sr
    v = 0.6 * np.sin(2 * np.pi * f0 * t + rng.uniform(0, 2 * np.pi)) + 0.3 * rng.uniform(-1.0, 1.0, int(L))
    return (amp * v).astype(np.float32)
