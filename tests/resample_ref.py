"""Float64 references of the device audio path (``smi_rs_*``, sparkmi/audio.py) and the bounds its tests hold it to.

Resampling.  For a row x[0 .. n), up/down in lowest terms and taps h[0 .. 2H]:

    n_out = ceil(n up / down),    y[k] = sum_j x[j] h[H + k down - j up]   (0 <= j < n, tap index in [0, 2H])

``direct`` evaluates that in float64 and returns, per output sample, the value, sum_j |h x| and the number of terms N.  The device
sums in fp32, ascending j, one accumulator, with taps rounded to fp32 once: N products, N - 1 additions and one tap rounding a
term, so by the standard running-error bound

    |y - y_ref| <= gamma_{N+1} sum_j |h x|,   gamma_m = m u / (1 - m u),  u = 2^-24,

with y_ref the float64 formula on the fp32 input with float64 taps (``bound``).  ``emulate_fp32`` is that order in numpy.

Prompt stages.  ``normalize_ref`` is ``audio_volume_normalize`` (sparktts/utils/audio.py:34-75) in float64, stage by stage, and
also returns the combined gain; its keyword arguments build the deliberately wrong variants the tests must tell apart.
``GAIN_RTOL`` = 1e-12: the device forms the statistic exactly (fixed point) and the gain in float64, numpy's pairwise mean of at
most 2^19 values errs by about 2e-15 relative.
"""
import math

import numpy as np

U = 2.0 ** -24
GAIN_RTOL = 1e-12
# (input rate, output rate): into the model's 16 kHz, and out of it
PAIRS = ((48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 8000), (16000, 24000), (16000, 44100), (16000, 48000))


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n, up, down):
    return -((-n * up) // down)


def _index(n, up, down, half, tap_shift=0, drop_last=False, phase_shift=0):
    """[n_out][M] input indices J, tap indices T and the validity mask of every term, ascending j along axis 1"""
    k = np.arange(out_len(n, up, down), dtype=np.int64)
    c = k * down + phase_shift
    jlo = np.maximum(0, -((-(c - half)) // up))
    jhi = np.minimum(n - 1, (c + half) // up)
    M = int(max(1, (jhi - jlo).max() + 1))
    J = jlo[:, None] + np.arange(M, dtype=np.int64)[None, :]
    valid = J <= jhi[:, None]
    if drop_last:
        valid &= J < jhi[:, None]
    T = half + c[:, None] - J * up + tap_shift
    valid &= (T >= 0) & (T <= 2 * half)
    return np.where(valid, J, 0), np.where(valid, T, 0), valid


def direct(x, up, down, h, **wrong):
    """(y, sum |h x|, N) per output sample, float64.  ``wrong``: tap_shift=1, drop_last=True or phase_shift=1 give the three
    wrong results the bound must reject."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    J, T, valid = _index(x.size, up, down, (h.size - 1) // 2, **wrong)
    terms = np.where(valid, x[J] * h[T], 0.0)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1), valid.sum(axis=1)


def emulate_fp32(x, up, down, h):
    """the device's order: fp32 taps, fp32 products, one fp32 accumulator, ascending j"""
    x = np.asarray(x, np.float32)
    h = np.asarray(h, np.float64).astype(np.float32)
    J, T, valid = _index(x.size, up, down, (h.size - 1) // 2)
    acc = np.zeros(J.shape[0], np.float32)
    for m in range(J.shape[1]):
        acc = np.where(valid[:, m], acc + x[J[:, m]] * h[T[:, m]], acc).astype(np.float32)
    return acc


def bound(absum, N):
    m = (np.asarray(N, np.float64) + 1.0) * U
    return m / (1.0 - m) * absum


def normalize_ref(audio, coeff=0.2, lo_shift=0, hi_shift=0, inclusive=False):
    """(normalized samples, combined gain), float64.  lo_shift / hi_shift move a rank by that much, inclusive=True turns the
    ``> 0.01`` filter into ``>=``: the wrong variants."""
    audio = np.asarray(audio, np.float64)
    gain = 1.0
    temp = np.sort(np.abs(audio))
    if temp[-1] < 0.1:
        scale = max(temp[-1], 1e-3)
        audio = audio / scale * 0.1
        gain = gain / scale * 0.1
    temp = temp[temp >= 0.01] if inclusive else temp[temp > 0.01]
    n = temp.shape[0]
    if n <= 10:
        return audio, gain
    volume = np.mean(temp[int(0.9 * n) + lo_shift: int(0.99 * n) + hi_shift])
    g = np.clip(coeff / volume, a_min=0.1, a_max=10)
    audio = audio * g
    gain = gain * g
    peak = np.max(np.abs(audio))
    if peak > 1:
        audio = audio / peak
        gain = gain / peak
    return audio, float(gain)


def fixed_point_gain(y32):
    """The device's way to the gain, in integers: ranks selected on the bit patterns of |y|, the range summed as multiples of
    2^-30 (Python integers: exact), one division, the gain in float64."""
    a = np.abs(np.asarray(y32, np.float32))
    bits = np.sort(a.view(np.uint32))
    peak = float(bits[-1:].view(np.float32)[0])
    gain = 1.0
    if peak < 0.1:
        gain = 0.1 / max(peak, 1e-3)
    cnt = bits[bits.view(np.float32).astype(np.float64) > 0.01]
    n = cnt.size
    if n <= 10:
        return gain
    lo, hi = int(0.9 * n), int(0.99 * n)
    fixed = [int(float(v) * 2.0 ** 30) for v in cnt[lo:hi].view(np.float32)]
    assert all(f / 2.0 ** 30 == float(v) for f, v in zip(fixed, cnt[lo:hi].view(np.float32)))   # multiples of 2^-30
    volume = float(sum(fixed)) / 2.0 ** 30 / float(hi - lo)
    gain = gain * min(max(0.2 / volume, 0.1), 10.0)
    if peak * gain > 1.0:
        gain = gain / (peak * gain)
    return gain


def gain_inputs():
    """name -> fp32 row; every branch of the normalisation and ties at both ranks"""
    rng = np.random.default_rng(11)
    noise = (0.2 * rng.standard_normal(20000)).astype(np.float32)
    quiet = (0.02 * rng.standard_normal(5000)).astype(np.float32)
    quiet *= np.float32(0.08) / np.abs(quiet).max()
    sparse = np.zeros(3000, np.float32)
    sparse[::400] = 0.5                                    # 8 samples above 0.01
    q8 = (np.round(np.clip(0.25 * rng.standard_normal(20000), -1, 1) * 127) / 127).astype(np.float32)
    loud = (0.004 * rng.standard_normal(8000)).astype(np.float32)
    loud[::9] = 0.011 * np.sign(rng.standard_normal(loud[::9].size)).astype(np.float32)
    loud[100] = 0.9                                        # gain 10 drives the peak over 1
    edge = noise.copy()
    edge[:50] = np.float32(0.01)                           # fp32(0.01) < 0.01: not counted
    return dict(noise=noise, quiet=quiet, sparse=sparse, q8=q8, loud=loud, edge=edge)


def ref_clip(wav, n):
    """get_ref_clip's tiling: ref[i] = wav[i mod len(wav)], i < n"""
    wav = np.asarray(wav)
    return wav[np.arange(n) % wav.size]
