"""The look-ahead true-peak limiter (include/sparkmi.h, smi_limit_rows) restated in numpy float64: vectorised over the sample
index i, the loops over the taps d and over the window k in the header's order, every product and sum an operation of its own
(numpy fuses nothing), so the device is held to it bit for bit.  ``limit`` also takes the wrong variants that
tests/test_limit_cpu.py shows the committed cases to tell apart.  ``reference()`` generates the cases from fixed seeds."""
import functools

import numpy as np

from sparkmi import audio

HALO = 10            # H / P: the interpolator's reach in samples on either side
PHASES = 4
TILE = 1024          # samples a block of the device kernels
A0, R0 = 40, 400     # audio.limiter_reach(16000)
CEILING = audio.PEAK_CEILING


def taps(phases=PHASES):
    return np.ascontiguousarray(audio.resample_taps(phases, 1), dtype=np.float64)


def c32(ceiling):
    """the largest float32 <= ceiling"""
    c = np.float32(ceiling)
    return c if float(c) <= ceiling else np.nextafter(c, np.float32(0))


def envelope(x, h, phases=PHASES, use=None):
    """e[i] = max(|x[i]|, |u_k[i]|): u_k[i] = sum over ascending d of fl(h[P d + k + H] x[i - d]); ``h`` None: |x| alone.
    ``use``: the phases k that take part (a wrong variant drops one)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = np.abs(x)
    if h is None:
        return e
    L, H = x.size, (h.size - 1) // 2
    assert h.size == 2 * HALO * phases + 1
    xp = np.concatenate([np.zeros(HALO), x, np.zeros(HALO)])
    for k in (range(1, phases) if use is None else use):
        u = np.zeros(L)
        for d in range(-HALO, HALO):
            u = u + h[phases * d + k + H] * xp[HALO - d: HALO - d + L]
        e = np.maximum(e, np.abs(u))
    return e


def limit(x, g, ceiling, h, A, R, w, phases=PHASES, use=None, min_lo=0, min_hi=0, shift=0, on_m=False, final_min=True, clamp=True,
          gain_last=False):
    """One span.  Returns dict(out float32, e, r, m, s, stats [4]).  The keywords past ``phases`` are the wrong variants."""
    x = np.asarray(x, dtype=np.float32)
    L, W = x.size, A + R
    w = np.asarray(w, dtype=np.float64)
    assert w.size == W + 1
    x64 = x.astype(np.float64)
    e = envelope(x, h, phases, use)
    v = g * e
    with np.errstate(divide="ignore"):
        r = np.where(v > ceiling, ceiling / np.where(v > ceiling, v, 1.0), 1.0)
    # m[j] = min r[j - R .. j + A] for j in [-(W + 1), L + W + 1), r = 1 outside the span; mm[j + W + 1] holds m[j]
    pad = 2 * W + 2
    rp = np.concatenate([np.ones(pad), r, np.ones(pad)])
    n_m = L + 2 * W + 2
    mm = np.full(n_m, np.inf)
    for t in range(-(R - min_lo), (A - min_hi) + 1):
        lo = pad - (W + 1) + t
        mm = np.minimum(mm, rp[lo: lo + n_m])
    acc = np.zeros(L)
    for k in range(-R + shift, A + shift + 1):
        mk = mm[W + 1 - k: W + 1 - k + L]             # m[i - k]
        acc = acc + w[k + R - shift] * (mk if on_m else 1.0 - mk)
    s = acc if on_m else 1.0 - acc
    if final_min:
        s = np.minimum(s, r)
    o = (x64 * s) * g if gain_last else (x64 * g) * s
    out = o.astype(np.float32)
    if clamp:
        c = c32(ceiling)
        out = np.minimum(np.maximum(out, -c), c)
    stats = np.array([g * (e.max() if L else 0.0), g, s.min() if L else 1.0, float(np.count_nonzero(s < 1.0))], dtype=np.float64)
    return dict(out=out, e=e, r=r, m=mm[W + 1: W + 1 + L], s=s, stats=stats)


def gain_only(x, g):
    """smi_gain_rows' arithmetic: fl32(fl64(x) g)"""
    return (np.asarray(x, dtype=np.float32).astype(np.float64) * g).astype(np.float32)


def run(c, **variant):
    """the case ``c`` through ``limit`` (its own mode, reach and window)"""
    return limit(c["x"], c["g"], c["ceiling"], taps() if c["mode"] == "true" else None, c["A"], c["R"], audio.limiter_window(c["A"], c["R"]),
                 **variant)


def true_peak(y):
    """the 4x oversampled peak of a float32 row, with the limiter's own taps"""
    e = envelope(y, taps())
    return float(e.max()) if e.size else 0.0


def _noise(rng, L, amp):
    """speech-like: white noise through a short moving average and a slow envelope, peak ``amp``"""
    if L == 0:
        return np.zeros(0, dtype=np.float32)
    z = np.convolve(rng.standard_normal(L + 4), np.ones(5) / 5.0, mode="valid")
    z = z * (0.55 + 0.45 * np.sin(2 * np.pi * np.arange(L) / 1700.0 + 0.3))
    return (z * (amp / max(1e-30, float(np.max(np.abs(z)))))).astype(np.float32)


def _clicks(rng, L, at, amp=1.5, floor=0.2):
    x = _noise(rng, L, floor)
    for n, i in enumerate(at):
        x[i] = amp if n % 2 == 0 else -amp
    return x


@functools.lru_cache(maxsize=None)
def reference():
    """the committed cases: dict(name, x, g, ceiling, mode, A, R) with ``want`` = run(case)"""
    rng = np.random.default_rng(20240917)
    cases = []

    def add(name, x, g=1.0, ceiling=CEILING, mode="true", A=A0, R=R0):
        cases.append(dict(name=name, x=np.ascontiguousarray(x, dtype=np.float32), g=float(g), ceiling=float(ceiling), mode=mode,
                          A=int(A), R=int(R)))

    # span lengths: nothing, less than the interpolator's reach, the look-ahead, the whole reach, around one tile, four tiles
    for L in (0, 1, 2, HALO, A0, A0 + R0, TILE - 1, TILE, TILE + 1, 3 * TILE + A0 + R0 + 1):
        add(f"len{L}", _noise(rng, L, 0.5), g=2.5)
    # where the overs lie
    L = 2 * TILE + 452
    add("first_last", _clicks(rng, L, [0, L - 1]))
    add("tile_edge", _clicks(rng, L, [TILE - 1, TILE, 2 * TILE - 1, 2 * TILE]))
    add("two_close", _clicks(rng, L, [600, 900]))
    add("dist_A", _clicks(rng, L, [1000, 1000 + A0]))
    add("dist_R", _clicks(rng, L, [1000, 1000 + R0]))
    add("dist_A_R", _clicks(rng, L, [700, 700 + A0 + R0, 700 + 2 * (A0 + R0) + 1]))
    # an inter-sample over: a quarter-rate sine sampled at 45 degrees, |samples| = 0.778 under the ceiling, true peak 1.1 over it
    quarter = (1.1 * np.sin(0.5 * np.pi * np.arange(600) + 0.25 * np.pi)).astype(np.float32)
    add("quarter_true", quarter)
    add("quarter_sample", quarter, mode="sample")
    # the reach
    for A, R in ((0, 0), (3, 5), (256, 2048)):
        add(f"A{A}_R{R}_short", _noise(rng, 700, 0.5), g=2.5, A=A, R=R)
        add(f"A{A}_R{R}_clicks", _clicks(rng, 1500, [0, 1, 740, 1023, 1024, 1499]), g=1.25, A=A, R=R)
        add(f"A{A}_R{R}_hot", _noise(rng, 1100, 0.5), g=12.0, A=A, R=R)
    add("A256_R2048_long", _noise(rng, 3 * TILE + 256 + 2048 + 1, 0.5), g=2.5, A=256, R=2048)
    # gains; no over at all; the sample-peak mode; another ceiling (its float32 neighbour lies above it)
    add("no_over", _noise(rng, 1500, 0.3), g=2.0)
    add("no_over_unit", _noise(rng, 1500, 0.5))
    add("sample_mode", _noise(rng, 1500, 0.5), g=2.5, mode="sample")
    add("ceiling_0p8", _clicks(rng, 900, [5, 450, 899]), g=1.0, ceiling=0.8, mode="sample", A=0, R=0)
    add("ceiling_0p8_true", _noise(rng, 1300, 0.5), g=3.0, ceiling=0.8)
    # The float32 rounding of the row hides a float64 rounding unless a product falls within an ulp of the middle between two
    # float32 values.  These samples do (found by a search over the float32 values under the ceiling, beside a click, for this
    # gain): fl32(fl(fl(x g) s)) and fl32(fl(fl(x s) g)) differ there, which tells the order of the two products.
    x = np.zeros(64, dtype=np.float32)
    x[20] = 1.5
    x[23], x[17] = float.fromhex("0x1.d04c2p-2"), float.fromhex("0x1.d04c2p-4")
    add("order_of_g", x, g=1.21 + 0.013 * 28, mode="sample", A=3, R=5)
    # three seconds at 16 kHz with a click, hot
    x = _noise(rng, 48000, 0.12)
    x[20000] = 0.9
    add("speech_3s", x, g=6.0)
    for c in cases:
        w = run(c)
        for a in w.values():
            a.setflags(write=False)
        c["x"].setflags(write=False)
        c["want"] = w
    return tuple(cases)
