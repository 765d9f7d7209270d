"""The limiter of joined streams (include/sparkmi.h, smi_limits_*) in numpy float64.  Nothing is defined anew: a stream's pieces,
concatenated, are tests/limit_ref.py's ``limit`` of the whole stream at g = 1.  ``stream`` is the host model of the device code:
the carried input, the emission rule E(n) = max(0, n - (A + R + 10)), r computed anew over what a piece can read, the running
stats -- with the same operations in the same order as ``limit`` (numpy fuses nothing), so it is held to it bit for bit.  It
also takes the wrong variants that tests/test_limit_stream_cpu.py shows the committed cases to tell apart.  ``reference()``
generates the cases from limit_ref's own generators with fixed seeds; ``chunkings(case)`` lists the pushes the tests use."""
import functools

import numpy as np

import limit_ref as LR
from sparkmi import audio

HALO = LR.HALO
REACHES = ((0, 0), (3, 5), (40, 400), (256, 2048))
MODES = ("true", "sample")


def edge_of(A, R):
    """the push edge n that chunkings() uses for the "edge" cases (one push of n samples, then the rest): late enough that
    output E(n) reads the whole reach behind it, E(n) - (A + R) >= 0"""
    return 2 * (A + R + HALO) + 7


def emitted(n, A, R):
    """E(n): samples a stream of n samples that goes on has emitted"""
    return max(0, n - (A + R + HALO))


def piece_len(A, R, n_before, length, last):
    """(piece length, n after) of one push"""
    n = n_before + length
    return (n if last else emitted(n, A, R)) - emitted(n_before, A, R), n


def hist_start(n, A, R, keep=None):
    """first sample a stream of n samples that goes on still holds: what output E(n) reads first"""
    return max(0, emitted(n, A, R) - ((A + R) if keep is None else keep) - (HALO - 1))


def _smooth(r_ext, r_own, A, R, w):
    """s of ``piece`` samples from r over those and W = A + R more on either side (1 where there is none): limit_ref.limit's
    minimum (exact in any order) and its window sum, ascending k, every product and sum rounded on its own"""
    W, piece = A + R, r_own.size
    n_m = piece + W                                        # m[j], j from (first sample) - A to (last sample) + R
    m = np.lib.stride_tricks.sliding_window_view(r_ext, W + 1).min(axis=1) if piece else np.zeros(0)
    assert m.size == (n_m if piece else 0)
    acc = np.zeros(piece)
    for k in range(-R, A + 1):
        acc = acc + w[k + R] * (1.0 - m[A - k: A - k + piece])     # m[i - k]
    return np.minimum(1.0 - acc, r_own)


def stream(x, pushes, ceiling, h, A, R, w, variant=None):
    """``x`` float32 pushed in chunks of ``pushes`` samples (the last push is the stream's last; lengths may be 0).  Returns
    dict(out float32 -- the pieces concatenated --, pieces -- their lengths --, s float64, stats [4], stats_after -- the stats
    after every push --, held -- the most input samples held between two pushes).
    ``variant``: "drop_history" (zeros and r = 1 before a push's chunk), "short_history" (only R + 9 samples carried before
    E(n), zeros before them), "early" (E = n - (A + R): the interpolator's reach forgotten), "stats_last" (the stats of the last
    push alone)."""
    x = np.asarray(x, dtype=np.float32)
    w = np.asarray(w, dtype=np.float64)
    W = A + R
    assert w.size == W + 1 and sum(pushes) == x.size and len(pushes) >= 1
    E = (lambda n: max(0, n - W)) if variant == "early" else (lambda n: emitted(n, A, R))
    c32 = LR.c32(ceiling)
    hist, h0, n_old = np.zeros(0, dtype=np.float32), 0, 0
    emax, smin, cnt = 0.0, 1.0, 0.0
    outs, ss, lens, after, held = [], [], [], [], 0
    for t, length in enumerate(pushes):
        last = t == len(pushes) - 1
        chunk = x[n_old: n_old + length]
        n_new = n_old + length
        e_old, e_new = E(n_old), (n_new if last else E(n_new))
        piece = e_new - e_old
        if variant == "stats_last":
            emax, smin, cnt = 0.0, 1.0, 0.0
        if piece > 0:
            seq = np.concatenate([hist, chunk])            # the stream from h0 to n_new

            def at(lo, hi):
                """the stream over [lo, hi) as float32: zero before h0 (and before 0) and from n_new on"""
                v = np.zeros(hi - lo, dtype=np.float32)
                a, b = max(lo, h0), min(hi, n_new)
                if b > a:
                    v[a - lo: b - lo] = seq[a - h0: b - h0]
                return v

            r_lo, r_hi = max(0, e_old - W), min(n_new, e_new + W)
            e = LR.envelope(at(r_lo - HALO, r_hi + HALO), h)[HALO: HALO + r_hi - r_lo]
            v = 1.0 * e
            with np.errstate(divide="ignore"):
                r = np.where(v > ceiling, ceiling / np.where(v > ceiling, v, 1.0), 1.0)
            if variant == "drop_history":
                r[: max(0, min(r_hi, n_old) - r_lo)] = 1.0
            r_ext = np.ones(piece + 2 * W)                 # r over [e_old - W, e_new + W)
            r_ext[r_lo - (e_old - W): r_hi - (e_old - W)] = r
            s = _smooth(r_ext, r[e_old - r_lo: e_new - r_lo], A, R, w)
            o = (at(e_old, e_new).astype(np.float64) * 1.0) * s
            outs.append(np.minimum(np.maximum(o.astype(np.float32), -c32), c32))
            ss.append(s)
            emax = max(emax, float(e[e_old - r_lo: e_new - r_lo].max()))
            smin = min(smin, float(s.min()))
            cnt = cnt + float(np.count_nonzero(s < 1.0))
        lens.append(piece)
        after.append(np.array([emax, 1.0, smin, cnt], dtype=np.float64))
        if not last:
            h0_new = hist_start(n_new, A, R, R if variant == "short_history" else None)
            if variant == "drop_history":
                h0_new = n_new
            seq = np.concatenate([hist, chunk])
            assert h0_new >= h0
            hist, h0 = seq[h0_new - h0:].copy(), h0_new
            held = max(held, hist.size)
        n_old = n_new
    out = np.concatenate(outs) if outs else np.zeros(0, dtype=np.float32)
    return dict(out=out, pieces=lens, s=np.concatenate(ss) if ss else np.zeros(0), stats=after[-1], stats_after=after, held=held)


def taps_of(mode):
    return LR.taps() if mode == "true" else None


def run_stream(c, pushes, variant=None):
    return stream(c["x"], pushes, c["ceiling"], taps_of(c["mode"]), c["A"], c["R"], audio.limiter_window(c["A"], c["R"]), variant)


def _split(L, size):
    """pushes of ``size`` samples, the last one shorter (never empty unless L = 0)"""
    full, rest = divmod(L, size)
    return [size] * full + ([rest] if rest or not full else [])


def chunkings(c):
    """the ways the tests push the case ``c``: name -> push lengths.  Pushes of 1 and of 7 at the small reaches and on short
    streams only (a push is three launches)."""
    L, W = c["x"].size, c["A"] + c["R"]
    out = {"once": [L]}
    small = W <= 8
    if L <= (300 if small else 0):
        out["ones"] = _split(L, 1)
    if L <= (1100 if W <= 440 else 0):
        out["7"] = _split(L, 7)
    for size in (127, 128, 129, W + HALO, 251, 1009):
        if 0 < size < L:
            out[str(size)] = _split(L, size)
    if c["name"].endswith("_edge"):
        out["edge"] = [edge_of(c["A"], c["R"]), L - edge_of(c["A"], c["R"])]
    if L > 2:
        half = _split(L, max(1, L // 3))
        gaps = []
        for p in half:
            gaps += [p, 0]
        out["empties"] = gaps                              # an empty push behind every push, the last one included
    return out


@functools.lru_cache(maxsize=None)
def reference():
    """the committed cases: dict(name, x, ceiling, mode, A, R) with ``want`` = limit_ref.limit of the whole stream at g = 1"""
    rng = np.random.default_rng(20241021)
    cases = []

    def add(name, x, mode, A, R, ceiling=LR.CEILING):
        cases.append(dict(name=f"A{A}_R{R}_{mode}_{name}", x=np.ascontiguousarray(x, dtype=np.float32), g=1.0, ceiling=float(ceiling),
                          mode=mode, A=int(A), R=int(R)))

    for A, R in REACHES:
        W = A + R
        lengths = [0, 1, 2, 10, W + 9, W + 10, W + 11, 2 * W + 18, 2 * W + 19, 2 * W + 20, 1023, 1024, 1025, 4 * LR.TILE + 37]
        for mode in MODES:
            for L in sorted(set(lengths)):
                add(f"len{L}", LR._noise(rng, L, 1.3), mode, A, R)           # (peak 1.3: overs at g = 1)
            L = 2 * LR.TILE + 452
            add("first_last", LR._clicks(rng, L, [0, L - 1]), mode, A, R)
            # overs on both sides of E(n) for the push edge n = edge_of(A, R) and on both sides of the edge itself, and a larger
            # one in the look-ahead part of the carried history, E(n) - R - 12: only the whole history brings it (twelve samples
            # in, since the window's last weights are too small to show in float32)
            n = edge_of(A, R)
            e = emitted(n, A, R)
            x = LR._clicks(rng, max(L, n + W + 700), sorted({e - 1, e, n - 1, n}))
            x[e - R - 12] = 2.0
            add("edge", x, mode, A, R, ceiling=0.8)
            add("hot", LR._noise(rng, 1100 + W, 6.0), mode, A, R)           # most samples limited: every push edge inside a reduction
        quarter = (1.1 * np.sin(0.5 * np.pi * np.arange(600 + 2 * W) + 0.25 * np.pi)).astype(np.float32)
        add("quarter", quarter, "true", A, R)
        add("quarter", quarter, "sample", A, R)
    for c in cases:
        want = LR.run(c)
        for a in want.values():
            a.setflags(write=False)
        c["x"].setflags(write=False)
        c["want"] = want
    return tuple(cases)


def case(name):
    return next(c for c in reference() if c["name"] == name)
