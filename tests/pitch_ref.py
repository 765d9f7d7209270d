"""Numpy-only restatement of include/sparkmi.h's pitch section (smi_pitch_layout, smi_pitch_rows), built from the two references
the device's halves are already held to: ``tempo_ref.tempo`` (the WSOLA stretch, exact integer search) and
``resample_ref.emulate_fp32`` (the polyphase sum in the device's order), plus the cut.

For a span of L samples, a tempo t = tp / tq and a pitch ratio r = rp / rq:

    P / Q = (tp rq) / (tq rp) in lowest terms;  z = tempo(x, P, Q, N, D), M = ceil(L Q / P) samples
    up / down = rq / rp in lowest terms;        y = emulate_fp32(z, up, down, fl32(resample_taps(up, down)))
    the row is y[0 .. n_out), n_out = ceil(L tq / tp)

The tests hold the device to places and samples bit for bit, so there is no tolerance here.  ``pitch`` also builds the wrong
variants the tests must tell apart (``wrong=``): "cut" keeps the resampler's own length ceil(M up / down) instead of n_out;
"edge" lets the stretched signal run on to the end of its last frame (K H samples) and pads the sums' edge there instead of at
M; "two_pass" applies the tempo and the pitch as two WSOLA passes, one behind the other, instead of one."""
import math

import numpy as np

import resample_ref
import tempo_ref
from sparkmi.audio import resample_taps


def plan(L, t, r, N):
    """dict(n_out, P, Q, M, K, up, down) of a span of L samples at tempo t = (tp, tq) and pitch ratio r = (rp, rq)"""
    L, (tp, tq), (rp, rq) = int(L), (int(t[0]), int(t[1])), (int(r[0]), int(r[1]))
    a, b = tp * rq, tq * rp
    g = math.gcd(a, b)
    P, Q = a // g, b // g
    gr = math.gcd(rp, rq)
    M, K = tempo_ref.layout(L, P, Q, N)
    return dict(n_out=-((-L * tq) // tp), P=P, Q=Q, M=M, K=K, up=rq // gr, down=rp // gr)


def taps32(up, down):
    """the taps as the device gets them: ``resample_taps`` rounded to fp32 once"""
    return resample_taps(up, down).astype(np.float32)


def _resample(z, up, down):
    if z.size == 0:
        return np.zeros(0, np.float32)
    return resample_ref.emulate_fp32(z, up, down, taps32(up, down).astype(np.float64))


def _run_on(x, s, N, K):
    """the stretched signal with its last frame completed: K H samples (the "edge" variant's input)"""
    H = N // 2
    w = tempo_ref.window(N)
    xd = np.asarray(x, np.float32).astype(np.float64)
    out = np.zeros(K * H, dtype=np.float32)
    for k in range(K):
        if k == 0:
            out[:H] = tempo_ref._take(np.asarray(x, np.float32), 0, H)
            continue
        u0 = tempo_ref._take(xd, int(s[k]), H) * w[:H]
        u1 = tempo_ref._take(xd, int(s[k - 1]) + H, H) * w[H:]
        out[k * H: (k + 1) * H] = (u0 + u1).astype(np.float32)
    return out


def pitch(x, t, r, N, D, wrong=None):
    """(y float32 [n_out], s int64 [K]) of the span ``x`` at tempo t = (tp, tq) and pitch ratio r = (rp, rq)"""
    x = np.asarray(x, dtype=np.float32)
    pl = plan(x.size, t, r, N)
    if wrong == "two_pass":
        mid, _ = tempo_ref.tempo(x, int(t[0]), int(t[1]), N, D)
        return pitch(mid, (1, 1), r, N, D)
    z, s = tempo_ref.tempo(x, pl["P"], pl["Q"], N, D)
    assert z.size == pl["M"] and s.size == pl["K"]
    if (pl["up"], pl["down"]) == (1, 1):
        return z, s
    if wrong == "edge":
        z = _run_on(x, s, N, pl["K"])
    y = _resample(z, pl["up"], pl["down"])
    assert y.size >= pl["n_out"], (y.size, pl)
    return (y if wrong == "cut" else y[: pl["n_out"]]), s


def stretched(x, t, r, N, D):
    """z alone: what the device never writes to memory"""
    pl = plan(np.asarray(x).size, t, r, N)
    return tempo_ref.tempo(x, pl["P"], pl["Q"], N, D)[0]


def tone(L, f0=110.0, harmonics=7, sr=16000, amp=0.8):
    """a harmonic tone, float32 [L]: f0 and its first ``harmonics`` multiples at 1 / h"""
    t = np.arange(int(L), dtype=np.float64) / sr
    v = sum(np.sin(2 * np.pi * f0 * h * t + 0.3 * h) / h for h in range(1, harmonics + 1))
    return (amp * v / np.abs(v).max()).astype(np.float32)


def period(y, lo=40, hi=400):
    """the period of the middle of ``y``: the smallest lag in [lo, hi) at which the normalised autocorrelation has a local
    maximum within 3 % of its largest value (a periodic signal correlates as well at every multiple of its period)"""
    y = np.asarray(y, np.float64)
    y = y[y.size // 4: y.size // 4 + min(4096, y.size // 2)]
    y = y - y.mean()
    lags = np.arange(lo, min(hi, y.size // 2))
    c = np.array([float(y[:-g] @ y[g:]) / math.sqrt(float(y[:-g] @ y[:-g]) * float(y[g:] @ y[g:]) + 1e-300) for g in lags])
    for i in range(1, c.size - 1):
        if c[i] >= 0.97 * c.max() and c[i] >= c[i - 1] and c[i] >= c[i + 1]:
            return int(lags[i])
    return int(lags[int(np.argmax(c))])
