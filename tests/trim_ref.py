"""numpy restatements of include/sparkmi.h's long-form audio edge (smi_trim_rows, smi_concat_rows), in float64, and the inputs
the GPU tests run, so that the CPU tests can check those inputs themselves.

``bounds`` is the header's formula.  ``bounds_reference_style`` evaluates the same windows the way the reference's
``detect_speech_boundaries`` does (sparktts/utils/audio.py:186-225) -- fp32 ``sliding_window_view``, ``mean``, ``sqrt``, ``>=`` --
restated from those lines, not imported: the reference module imports torchaudio and soxr."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def energies(x, window, step):
    """float64 sums of the exact squares of the fp32 samples, one per window x[i s .. i s + W)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if x.size < window:
        return np.zeros(0)
    return np.array([np.sum(np.square(x[i: i + window])) for i in range(0, x.size - window + 1, step)])


def level(window, threshold):
    return float(threshold) * float(threshold) * float(window)


def _from_mask(mask, n, step, margin):
    if not mask.any():
        return (0, 0)
    first = int(np.argmax(mask))
    last = int(len(mask) - 1 - np.argmax(mask[::-1]))
    return (max(0, first * step - margin), min(n, last * step + margin))


def bounds(x, window, step, threshold, margin):
    n = len(x)
    if n < window:
        return (0, n)
    return _from_mask(energies(x, window, step) >= level(window, threshold), n, step, margin)


def bounds_reference_style(x, window, step, threshold, margin):
    """the reference's evaluation; its two ValueError cases (a row shorter than the window, no speech) take the header's values"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    if n < window:
        return (0, n)
    windows = sliding_window_view(x, window)[::step]
    energy = np.sqrt(np.mean(windows ** 2, axis=1))
    return _from_mask(energy >= threshold, n, step, margin)


def closest_to_level(x, window, step, threshold):
    """min over windows of |S_i - level| / level (inf without windows or with a zero level)"""
    e, lv = energies(x, window, step), level(window, threshold)
    if not e.size or lv == 0:
        return np.inf
    return float(np.min(np.abs(e - lv)) / lv)


def faded(piece, fade):
    p = np.asarray(piece, dtype=np.float32).copy()
    L = p.size
    f = min(int(fade), L // 2)
    if f:
        w = np.arange(1, f + 1, dtype=np.float64) / np.float64(f + 1)
        p[:f] = (p[:f].astype(np.float64) * w).astype(np.float32)
        p[L - f:] = (p[L - f:].astype(np.float64) * w[::-1]).astype(np.float32)
    return p


def layout(bounds_, gaps):
    """(offset of every piece, total): an empty piece drops its gap"""
    offs, total = [], 0
    for (a, b), g in zip(bounds_, gaps):
        if b > a:
            total += g
        offs.append(total)
        total += b - a
    return offs, total


def concat(rows, bounds_, gaps, fade, cap=None):
    offs, total = layout(bounds_, gaps)
    out = np.zeros(total if cap is None else cap, dtype=np.float32)
    for x, (a, b), o in zip(rows, bounds_, offs):
        out[o: o + b - a] = faded(np.asarray(x, dtype=np.float32)[a:b], fade)
    return out, offs, total


# ---- the inputs of tests/test_trim_gpu.py
TILE = 64                    # windows a block of k_trim_scan (csrc/smi_audio.hip: TR_TILE)
PARAMS = {"small": (20, 2, 40, 0.05), "odd": (25, 2, 40, 0.05), "default": (1600, 160, 3200, 0.01)}   # W, s, m, thr


def _noise(rng, n, amp):
    return (amp * rng.standard_normal(n)).astype(np.float32)


def trim_cases(name):
    """[(label, row)] for one parameter set: rows of quiet noise (rms = thr / 10) with loud stretches (rms = 4 thr)"""
    W, s, m, thr = PARAMS[name]
    rng = np.random.default_rng({"small": 11, "odd": 12, "default": 13}[name])
    quiet, loud = thr / 10, 4 * thr
    cases = [("n=0", np.zeros(0, np.float32))]
    for label, n in (("n=W-1", W - 1), ("n=W", W), ("one window", W + s - 1), ("two windows", W + s)):
        cases.append((label, _noise(rng, n, loud)))
    for label, nwin in (("tile+1 windows", TILE + 1), ("tile-1 windows", TILE - 1), ("2 tiles+1 windows", 2 * TILE + 1)):
        n = (nwin - 1) * s + W + (s - 1)
        x = _noise(rng, n, quiet)
        x[n - W:] = _noise(rng, W, loud)            # speech at the very end: the last window, in the last tile, decides
        x[: W // 2] = _noise(rng, W // 2, loud)     # and a loud half window at the start, to see what the first windows do
        cases.append((label, x))
    n = 6 * W + 3 * s + 1
    nwin = (n - W) // s + 1
    x = _noise(rng, n, quiet); x[:W] = _noise(rng, W, loud * 3)
    cases.append(("speech in the first window", x))
    x = _noise(rng, n, quiet); x[(nwin - 1) * s:] = _noise(rng, n - (nwin - 1) * s, loud * 3)
    cases.append(("speech in the last window", x))
    x = _noise(rng, n, quiet); x[3 * W: 4 * W] = _noise(rng, W, loud * 3)
    cases.append(("speech in the middle", x))
    cases.append(("silent", _noise(rng, n, quiet)))
    cases.append(("zeros", np.zeros(n, np.float32)))
    return cases


def equality_case(name):
    """(row, thr, the window that sits exactly on the level): samples +-2^-k with thr = 2^-k sum exactly in any order, so a full
    window of them has S = W 2^-2k = the level, bit for bit; the rest of the row is zero"""
    W, s, m, _ = PARAMS[name]
    k = 5
    n = 5 * W + s
    x = np.zeros(n, np.float32)
    i = (2 * W) // s
    sign = np.where(np.arange(W) % 3 == 0, -1.0, 1.0)
    x[i * s: i * s + W] = (sign * 2.0 ** -k).astype(np.float32)
    return x, 2.0 ** -k, i


CONCAT_FADE = 8
CONCAT_LENGTHS = [0, 1, 2, 3, 2 * CONCAT_FADE - 1, 2 * CONCAT_FADE, 2 * CONCAT_FADE + 1, 0, 2500]


def concat_case(seed=5):
    """(rows [B][stride] float32, n, bounds): pieces of CONCAT_LENGTHS somewhere inside rows of different lengths"""
    rng = np.random.default_rng(seed)
    stride = 2600
    rows = rng.standard_normal((len(CONCAT_LENGTHS), stride)).astype(np.float32)
    n, bounds_ = [], []
    for b, L in enumerate(CONCAT_LENGTHS):
        a = 0 if b % 2 else 7 * b
        bounds_.append((a, a + L))
        n.append(min(stride, a + L + 3 * (b % 3)))
    return rows, n, bounds_
