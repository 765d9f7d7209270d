"""Numpy-only restatement of include/sparkmi.h's output loudness (smi_loud_rows, smi_gain_rows): BS.1770's K-weighting as a
sequential recurrence, 400 ms blocks of four hops, both gates in the linear domain, and the gain to a target under a peak
ceiling -- in float64 and, for the error bounds, in ``np.longdouble``; the device's own order of operations (segments of
``LD_SEG`` samples, a carry of states, hop parts, strided block sums) in float64; and the cases the tests share.

The tolerance.  ``emulate`` differs from ``loudness(..., dt=np.longdouble)`` by float64 rounding alone; over
all committed cases that difference stays below ``EMU_LU`` in loudness and ``EMU_GAIN`` in relative gain (tests/test_loud_cpu.py
measures it and holds it to these).  The device adds one ``log10`` (OpenCL's bound: 3 ulp, on a value of magnitude < 10, times
10: < 1e-14 LU) and two ``pow`` (16 ulp each: 7e-15 relative), which ``MARGIN`` covers with room."""
import functools
import math

import numpy as np

LD_SEG = 128            # csrc/smi_audio.hip
LD_TILE = 64 * LD_SEG   # samples of one block of k_loud_seg
GATE_LANES = 256        # k_loud_gate's threads
OFFSET = -0.691
EMU_LU = 1e-12          # bound on |emulate - longdouble| in LU over the committed cases
EMU_GAIN = 1.2e-13       # ... and in relative gain
MARGIN = 8.0            # for the device's log10 / pow
TOL_LU = EMU_LU * MARGIN
TOL_GAIN = EMU_GAIN * MARGIN


def k_weighting(sr):
    from sparkmi.audio import k_weighting as kw
    return kw(sr)


def _step(c, s, v):
    """one sample through both biquads in the header's order; ``s`` = [x1, x2, p1, p2, q1, q2] is updated in place"""
    w = ((c[0] * v + c[1] * s[0]) + c[2] * s[1]) - c[4] * s[3]
    y = w - c[3] * s[2]
    u = ((c[5] * y + c[6] * s[2]) + c[7] * s[3]) - c[9] * s[5]
    o = u - c[8] * s[4]
    s[1] = s[0]; s[0] = v
    s[3] = s[2]; s[2] = y
    s[5] = s[4]; s[4] = o
    return o


def _scalars(x, coef, dt):
    if dt is np.float64:   # Python floats: IEEE float64, no FMA
        return [float(v) for v in np.asarray(x, dtype=np.float32)], [float(v) for v in coef], 0.0
    return [dt(v) for v in np.asarray(x, dtype=np.float32)], [dt(v) for v in np.asarray(coef, dtype=np.float64)], dt(0)


def kfilter(x, coef, dt=np.float64):
    """the K-weighted span, sample by sample from zero state"""
    xs, c, zero = _scalars(x, coef, dt)
    s = [zero] * 6
    return [_step(c, s, v) for v in xs]


def _seq_sum(vals, zero):
    t = zero
    for v in vals:
        t = t + v
    return t


def abs_gate(dt=np.float64):
    return dt(10.0) ** ((dt(-70.0) + dt(0.691)) / dt(10.0))


def blocks(x, coef, block, dt=np.float64, hops=4, tail=False):
    """z_j, the mean squares of the blocks (one block, the whole span, where it is shorter than a block)"""
    L = len(x)
    if L == 0:
        return []
    zero = 0.0 if dt is np.float64 else dt(0)
    e = [v * v for v in kfilter(x, coef, dt)]
    if L < block:
        return [_seq_sum(e, zero) / dt(L)]
    hop = block // hops
    H = [_seq_sum(e[h * hop: (h + 1) * hop], zero) for h in range(L // hop)]
    z = [_seq_sum(H[j: j + hops], zero) / dt(block) for j in range((L - block) // hop + 1)]
    if tail and (L - block) % hop:   # (a variant the standard rules out: the last, shorter block counted too)
        a = len(z) * hop
        z.append(_seq_sum(e[a:], zero) / dt(L - a))
    return z


def gates(z, L, block, dt=np.float64, rel=None, use_abs=True):
    """(the mask after the absolute gate, the relative threshold or None, the mask after both)"""
    A = abs_gate(dt)
    m1 = [(zz > A) if use_abs else True for zz in z]
    if L < block or not any(m1):
        return m1, None, list(m1)
    zero = 0.0 if dt is np.float64 else dt(0)
    mean = _seq_sum([zz for zz, k in zip(z, m1) if k], zero) / dt(sum(m1))
    thr = (dt(0.1) if rel is None else dt(10.0) ** (dt(rel) / dt(10.0))) * mean
    return m1, thr, [k and zz > thr for zz, k in zip(z, m1)]


def loudness(x, coef, block, dt=np.float64, hops=4, rel=None, use_abs=True, tail=False, offset=OFFSET):
    """the integrated loudness of the span; the keywords build the wrong variants the tolerance must reject"""
    z = blocks(x, coef, block, dt, hops, tail)
    _, _, m2 = gates(z, len(x), block, dt, rel, use_abs)
    if not any(m2):
        return -math.inf
    zero = 0.0 if dt is np.float64 else dt(0)
    mean = _seq_sum([zz for zz, k in zip(z, m2) if k], zero) / dt(sum(m2))
    return dt(offset) + dt(10.0) * np.log10(dt(mean))


def peak(x):
    x = np.asarray(x, dtype=np.float32)
    return float(np.max(np.abs(x))) if x.size else 0.0


def gain(loud, pk, target, max_gain_db, ceiling, dt=np.float64):
    """(gain, limit) of the header's rule"""
    if target is None or (isinstance(target, float) and math.isnan(target)) or loud == -math.inf:
        return dt(1.0), 0
    g = dt(10.0) ** ((dt(target) - dt(loud)) / dt(20.0))
    gmax = dt(10.0) ** (dt(max_gain_db) / dt(20.0))
    limit = 0
    if g > gmax:
        g, limit = gmax, 1
    if g * dt(pk) > dt(ceiling):
        g, limit = dt(ceiling) / dt(pk), 2
    return g, limit


def apply_gain(x, g):
    """fl32(fl64(x) * g)"""
    return (np.asarray(x, dtype=np.float32).astype(np.float64) * np.float64(g)).astype(np.float32)


# ---- the device's order of operations, in float64
def transition(coef):
    c = [float(v) for v in coef]
    T = [[0.0] * 4 for _ in range(4)]
    for i in range(4):
        s = [0.0, 0.0] + [1.0 if q == i else 0.0 for q in range(4)]
        for _ in range(LD_SEG):
            _step(c, s, 0.0)
        for q in range(4):
            T[q][i] = s[2 + q]
    return T


def _lane_sum(vals):
    """k_loud_gate's sum: lane t adds its values j = t, t + 256, ... in ascending order, then the fixed tree"""
    lanes = [0.0] * GATE_LANES
    for j, v in enumerate(vals):
        if v is not None:
            lanes[j % GATE_LANES] = lanes[j % GATE_LANES] + v
    o = GATE_LANES // 2
    while o:
        for t in range(o):
            lanes[t] = lanes[t] + lanes[t + o]
        o //= 2
    return lanes[0]


def emulate(x, coef, block):
    """the loudness as csrc/smi_audio.hip forms it: segments from zero state, the carry, hop parts, strided sums"""
    xs, c, _ = _scalars(x, coef, np.float64)
    L = len(xs)
    if L == 0:
        return -math.inf
    hop = block // 4
    nseg = (L + LD_SEG - 1) // LD_SEG
    hist = lambda i0: [xs[i0 - 1] if i0 >= 1 else 0.0, xs[i0 - 2] if i0 >= 2 else 0.0]   # noqa: E731
    T = transition(coef)
    S = [[0.0] * 4]
    for k in range(nseg - 1):
        s = hist(k * LD_SEG) + [0.0] * 4
        for v in xs[k * LD_SEG: (k + 1) * LD_SEG]:
            _step(c, s, v)
        p = S[-1]
        S.append([(((T[i][0] * p[0] + T[i][1] * p[1]) + T[i][2] * p[2]) + T[i][3] * p[3]) + s[2 + i] for i in range(4)])
    nh = (L + hop - 1) // hop
    H = [0.0] * nh
    for k in range(nseg):
        s = hist(k * LD_SEG) + list(S[k])
        acc, i = 0.0, k * LD_SEG
        for v in xs[k * LD_SEG: (k + 1) * LD_SEG]:
            o = _step(c, s, v)
            acc = acc + o * o
            i += 1
            if i % hop == 0:
                H[i // hop - 1] = H[i // hop - 1] + acc
                acc = 0.0
        if i % hop:
            H[i // hop] = H[i // hop] + acc
    if L >= block:
        z = [(((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / float(block) for j in range((L - block) // hop + 1)]
    else:
        z = [_seq_sum(H, 0.0) / float(L)]
    A = abs_gate()
    m = [zz > A for zz in z]
    if not any(m):
        return -math.inf
    if L >= block:
        rel = 0.1 * (_lane_sum([zz if k else None for zz, k in zip(z, m)]) / float(sum(m)))
        m = [k and zz > rel for zz, k in zip(z, m)]
    return OFFSET + 10.0 * math.log10(_lane_sum([zz if k else None for zz, k in zip(z, m)]) / float(sum(m)))


# ---- the committed cases
SMALL_BLOCK = 64   # hop 16: rows of a few thousand samples reach every branch


def _tone(n, sr, amps, seed, f=997.0):
    """a sine with a little noise under a piecewise-constant envelope: ``amps`` = [(samples, amplitude)], cut or padded to n"""
    rng = np.random.default_rng(seed)
    env = np.concatenate([np.full(m, a, dtype=np.float64) for m, a in amps])
    env = np.concatenate([env, np.full(max(0, n - env.size), amps[-1][1])])[:n]
    t = np.arange(n, dtype=np.float64)
    return (env * (np.sin(2 * np.pi * f * t / sr) + 0.1 * rng.standard_normal(n))).astype(np.float32)


def cases():
    """[{name, x (the span, float32), sr, block, target, max_gain_db, ceiling}]: every span length and signal the issue lists"""
    out = []
    ceil0 = 10 ** (-1 / 20)

    def add(name, x, sr=16000, block=SMALL_BLOCK, target=-23.0, max_gain_db=20.0, ceiling=ceil0):
        out.append(dict(name=name, x=np.ascontiguousarray(x, dtype=np.float32), sr=sr, block=block, target=target,
                        max_gain_db=max_gain_db, ceiling=ceiling))

    b, h = SMALL_BLOCK, SMALL_BLOCK // 4
    lengths = [0, 1, b - 1, b, b + h - 1, b + 3 * h + 5, LD_SEG - 1, LD_SEG, LD_SEG + 1, 3 * LD_SEG + 5, LD_TILE + 300]
    for q, L in enumerate(lengths):
        sr = 48000 if q % 2 else 16000
        add(f"len{L}", _tone(L, sr, [(max(1, L), 0.2)], 100 + q), sr=sr)
    # loud - quiet - loud: the relative gate drops the quiet blocks; the middle level lies between the -10 and the -8 LU gate
    lql = [(700, 0.5), (600, 0.5 * 10 ** (-11.7 / 20)), (500, 0.5 * 10 ** (-40 / 20)), (700, 0.5)]
    add("loud_quiet_loud", _tone(2500, 16000, lql, 7))
    add("loud_quiet_loud_48k", _tone(2500, 48000, lql, 8), sr=48000)
    add("under_abs_gate", _tone(1500, 16000, [(1500, 1e-5)], 9))
    add("zeros", np.zeros(1000, dtype=np.float32))
    add("max_gain_binds", _tone(2000, 16000, [(2000, 0.003)], 10))
    add("ceiling_binds", _tone(2000, 48000, [(2000, 0.6)], 11), sr=48000, target=-3.0)
    add("measure_only", _tone(1800, 16000, [(900, 0.3), (900, 0.05)], 12), target=math.nan)
    add("real_3s_16k", _tone(48000, 16000, [(16000, 0.3), (9000, 0.004), (23000, 0.12)], 13, f=220.0), block=6400)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """per case, computed once and shared: the coefficients, the longdouble loudness, the peak, and the gain and limit they give"""
    out = []
    for c in cases():
        coef = k_weighting(c["sr"])
        loud = loudness(c["x"], coef, c["block"], np.longdouble)
        pk = peak(c["x"])
        g, limit = gain(loud, pk, c["target"], c["max_gain_db"], c["ceiling"], np.longdouble)
        out.append(dict(c, coef=coef, loudness=loud, peak=pk, gain=g, limit=limit))
    return out
