"""Numpy-only restatement of include/sparkmi.h's loudness of joined streams (smi_louds_*): the running BS.1770 gain, knot by knot
on the stream's absolute hops -- sequentially in float64 and, for the error bounds, in ``np.longdouble``; in the device's own
order of operations (tests/loud_ref.py's segments, carry, hop parts and strided block sums) in float64; the emission
arithmetic (``piece_len``); and the cases the tests share.

By the header's guarantee a stream's result does not depend on its pushes, so everything here takes the WHOLE stream.

The tolerance is the batch stage's construction: ``loud_ref.EMU_LU`` / ``EMU_GAIN`` bound the difference between
the device's order and the longdouble result (tests/test_loud_stream_cpu.py measures it over the cases below and holds it to
them), times ``loud_ref.MARGIN`` for the device's ``log10`` and ``pow``.  The slew clamp and the hold pass an error on without
amplifying it (both are monotone and 1-Lipschitz in the log domain), and a clamped knot adds one rounding (1.1e-16 relative)."""
import functools
import math

import numpy as np

import loud_ref as LR

TOL_LU = LR.TOL_LU
TOL_GAIN = LR.TOL_GAIN
F_MAX_GAIN, F_CEILING, F_SLEW, F_HOLD = 1, 2, 4, 8
CEIL0 = 10 ** (-1 / 20)


# ---- emission
def piece_len(block, n_before, length, last):
    """(piece, n after, knots made after): E(n) = hop max(0, floor(n / hop) - 4) while the stream goes on, L at its end"""
    hop = block // 4
    emitted = lambda n: hop * max(0, n // hop - 4)   # noqa: E731
    n = n_before + length
    if last:
        return n - emitted(n_before), n, ((n - 1) // hop + 2 if n else 0)
    return emitted(n) - emitted(n_before), n, max(0, n // hop - 3)


# ---- hop sums
def hops(x, coef, hop, dt=np.float64):
    """the definition: y^2 of the sequential filter, summed in ascending order per hop (the last one may be short)"""
    zero = 0.0 if dt is np.float64 else dt(0)
    e = [v * v for v in LR.kfilter(x, coef, dt)]
    return [LR._seq_sum(e[h * hop: (h + 1) * hop], zero) for h in range((len(e) + hop - 1) // hop)]


def hops_device(x, coef, hop):
    """the device's order (csrc/smi_audio.hip): segments of LD_SEG from zero state, the carry, each segment again from its true
    state, hop parts added in ascending order -- tests/loud_ref.py's ``emulate`` up to the hop sums"""
    xs, c, _ = LR._scalars(x, coef, np.float64)
    L, S = len(xs), LR.LD_SEG
    nseg = (L + S - 1) // S
    hist = lambda i0: [xs[i0 - 1] if i0 >= 1 else 0.0, xs[i0 - 2] if i0 >= 2 else 0.0]   # noqa: E731
    T = LR.transition(coef)
    st = [[0.0] * 4]
    for k in range(nseg - 1):
        s = hist(k * S) + [0.0] * 4
        for v in xs[k * S: (k + 1) * S]:
            LR._step(c, s, v)
        p = st[-1]
        st.append([(((T[i][0] * p[0] + T[i][1] * p[1]) + T[i][2] * p[2]) + T[i][3] * p[3]) + s[2 + i] for i in range(4)])
    H = [0.0] * ((L + hop - 1) // hop)
    for k in range(nseg):
        s = hist(k * S) + list(st[k])
        acc, i = 0.0, k * S
        for v in xs[k * S: (k + 1) * S]:
            o = LR._step(c, s, v)
            acc = acc + o * o
            i += 1
            if i % hop == 0:
                H[i // hop - 1] = H[i // hop - 1] + acc
                acc = 0.0
        if i % hop:
            H[i // hop] = H[i // hop] + acc
    return H


def _log10(v, dt):
    return math.log10(v) if dt is np.float64 else np.log10(v)


def _running(z, first, j, dt, device, margins):
    """the gated loudness over z[first .. j]: (a block passes, I)"""
    A = LR.abs_gate(dt)
    zz = z[first: j + 1]
    m1 = [v > A for v in zz]
    if margins is not None:
        margins["gate"] = min([margins["gate"]] + [abs(float(v) / float(A) - 1.0) for v in zz if v > 0])
    if not any(m1):
        return False, -math.inf
    zero = 0.0 if dt is np.float64 else dt(0)
    total = (lambda m: LR._lane_sum([v if k else None for v, k in zip(zz, m)])) if device else \
        (lambda m: LR._seq_sum([v for v, k in zip(zz, m) if k], zero))
    rel = dt(0.1) * (total(m1) / dt(sum(m1)))
    if margins is not None:
        margins["gate"] = min([margins["gate"]] + [abs(float(v) / float(rel) - 1.0) for v, k in zip(zz, m1) if k])
    m2 = [k and v > rel for v, k in zip(zz, m1)]
    if not any(m2):
        return False, -math.inf
    return True, dt(LR.OFFSET) + dt(10.0) * _log10(total(m2) / dt(sum(m2)), dt)


def slew_factors(max_slew_db):
    """(s_up, s_dn) as smi_louds_open forms them on the host, in float64: they are data to every version of the arithmetic"""
    up = 10.0 ** (float(max_slew_db) / 20.0)
    return up, 1.0 / up


def stream(x, coef, block, target, max_gain_db=20.0, ceiling=CEIL0, max_slew_db=1.0, dt=np.float64, device=False, variant=None,
           margins=None):
    """The whole definition for one stream: dict(G, flags, I (per knot), loudness (of the whole stream), z).  ``device``: the
    device's order of the sums (float64 only).  ``variant``: a wrong reading the tolerance must reject -- "early" (every knot
    one hop early), "peak1" (the peak over the knot's own hop alone), "slew_after_peak", "rel30" (both gates over the last 30
    blocks only).  ``margins`` (a dict with "gate" and "bound"): receives the smallest relative distance of a block from a gate
    and of a knot from a bound it is compared with."""
    x = np.asarray(x, dtype=np.float32)
    L, hop = len(x), block // 4
    if L == 0:
        return dict(G=[], flags=[], I=[], loudness=-math.inf, z=[])
    H = hops_device(x, coef, hop) if device else hops(x, coef, hop, dt)
    nz = max(0, L // hop - 3)
    z = [(((H[j] + H[j + 1]) + H[j + 2]) + H[j + 3]) / dt(block) for j in range(nz)]
    nk = (L - 1) // hop + 2
    ax = np.abs(x.astype(np.float64))
    measure_only = target is None or (isinstance(target, float) and math.isnan(target))
    s_up, s_dn = slew_factors(max_slew_db)
    s_up, s_dn, ceil_, one = dt(s_up), dt(s_dn), dt(ceiling), dt(1.0)
    gmax = dt(10.0) ** (dt(max_gain_db) / dt(20.0))

    def near(a, b):
        if margins is not None and float(b) > 0:
            margins["bound"] = min(margins["bound"], abs(float(a) / float(b) - 1.0))

    def target_gain(loud):
        A = dt(10.0) ** ((dt(target) - loud) / dt(20.0))
        near(A, gmax)
        return (gmax, F_MAX_GAIN) if A > gmax else (A, 0)

    short = None
    if nz == 0:   # shorter than a block: one block, the whole stream, the absolute gate alone
        zero = 0.0 if dt is np.float64 else dt(0)
        zz = LR._seq_sum(H, zero) / dt(L)
        if margins is not None and zz > 0:
            margins["gate"] = min(margins["gate"], abs(float(zz) / float(LR.abs_gate(dt)) - 1.0))
        if zz > LR.abs_gate(dt):
            short = (True, dt(LR.OFFSET) + dt(10.0) * _log10(zz, dt))
        else:
            short = (False, -math.inf)
    G, flags, Is = [], [], []
    loud = -math.inf
    hold = None   # (A, flags) of the knots behind the last whole block
    for j in range(nk):
        jj = j + 1 if variant == "early" else j
        prev = G[-1] if j else one
        if jj < nz:
            have, I = _running(z, max(0, jj - 29) if variant == "rel30" else 0, jj, dt, device, margins if variant is None else None)
            loud = I
            A, fl = (target_gain(I) if have else (prev, F_HOLD)) if not measure_only else (one, 0)
        else:
            if hold is None:
                if short is not None:
                    loud = short[1]
                    hold = (one, 0) if measure_only else (target_gain(short[1]) if short[0] else (one, F_HOLD))
                else:
                    hold = (prev, F_HOLD)
            A, fl = hold
            I = loud
        lo_i, hi_i = max(0, (j - 1) * hop), min(L, (j + 1) * hop)
        if variant == "peak1" and j * hop < hi_i:
            lo_i = j * hop
        P = dt(float(ax[lo_i:hi_i].max())) if hi_i > lo_i else dt(0.0)

        def slew(A, fl):
            if j == 0:
                return A, fl
            lo, hi = prev * s_dn, prev * s_up
            near(A, lo)
            near(A, hi)
            if A < lo:
                return lo, fl | F_SLEW
            if A > hi:
                return hi, fl | F_SLEW
            return A, fl

        def peak(A, fl):
            near(A * P, ceil_)
            if A * P > ceil_:
                return ceil_ / P, fl | F_CEILING
            return A, fl

        if measure_only:
            g, fl = one, 0
        elif variant == "slew_after_peak":
            g, fl = slew(*peak(A, fl))
        else:
            g, fl = peak(*slew(A, fl))
        G.append(g)
        flags.append(fl)
        Is.append(I)
    return dict(G=G, flags=flags, I=Is, loudness=loud, z=z)


def apply(x, G, hop):
    """out[i] = fl32(fl64(x[i]) * (G_j + fl(fl(G_{j+1} - G_j) * fl(fl64(i - j hop) / fl64(hop))))), float64, every step rounded"""
    x = np.asarray(x, dtype=np.float32)
    if not len(x):
        return x.copy()
    G = np.asarray([float(g) for g in G], dtype=np.float64)
    i = np.arange(len(x), dtype=np.int64)
    j = i // hop
    fr = (i - j * hop).astype(np.float64) / np.float64(hop)
    d = (G[j + 1] - G[j]) * fr
    return (x.astype(np.float64) * (G[j] + d)).astype(np.float32)


# ---- the committed cases
SMALL = 64     # hop 16: many hops a segment
MID = 400      # hop 100: hops straddle segments
REAL = 6400    # hop 1600, the 16 kHz value: segments inside a hop


def _noise(n, amp, seed):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _bursts(parts, seed, sr=16000, f=440.0):
    """[(samples, amplitude)]: a tone with a little noise under a piecewise-constant envelope"""
    n = sum(m for m, _ in parts)
    return LR._tone(n, sr, parts, seed, f=f)


def cases():
    """[{name, x, sr, block, target, max_gain_db, ceiling, max_slew_db}]"""
    out = []

    def add(name, x, block=SMALL, sr=16000, target=-23.0, max_gain_db=20.0, ceiling=CEIL0, max_slew_db=1.0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        x.setflags(write=False)
        out.append(dict(name=name, x=x, sr=sr, block=block, target=target, max_gain_db=max_gain_db, ceiling=ceiling,
                        max_slew_db=max_slew_db))

    for block in (SMALL, MID, REAL):
        hop = block // 4
        for q, L in enumerate([1, block - 1, block, block + hop - 1, 127, 128, 129]):
            add(f"b{block}_len{L}", _bursts([(max(1, L), 0.2)], 300 + q + block), block=block)
    add("b64_len0", np.zeros(0, dtype=np.float32))
    # a silent lead-in (hold), a quiet passage the gain climbs into at the slew rate, a loud one it falls from, a tail
    talk = [(400, 0.0), (900, 0.02), (900, 0.5), (700, 0.05), (437, 0.2)]
    add("b64_talk", _bursts(talk, 21))
    add("b400_talk", _bursts([(m * 4, a) for m, a in talk], 22), block=MID)
    click = _bursts([(2500, 0.05)], 23).copy()
    click[1203] = 0.9
    add("b64_click", click)
    add("b64_max_gain", _bursts([(1500, 0.002)], 24), max_gain_db=12.0)
    add("b64_measure_only", _bursts([(800, 0.3), (800, 0.03)], 25), target=math.nan)
    add("b64_under_gate", _bursts([(1200, 1e-5)], 26))
    add("b400_noise", _noise(5003, 0.1, 27), block=MID, sr=48000)
    add("real_3s", _bursts([(4000, 0.0), (14000, 0.25), (9000, 0.004), (21000, 0.1)], 28, f=220.0), block=REAL)
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """per case, computed once and shared (read only): the coefficients, the longdouble result and its samples"""
    out = []
    for c in cases():
        coef = LR.k_weighting(c["sr"])
        r = stream(c["x"], coef, c["block"], c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"], np.longdouble)
        y = apply(c["x"], r["G"], c["block"] // 4)
        y.setflags(write=False)
        out.append(dict(c, coef=coef, ref=r, y=y))
    return out


def case(name):
    return next(c for c in reference() if c["name"] == name)
