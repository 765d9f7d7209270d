"""smi_rs_*: the device resampler and the prompt preparation, through the C ABI, against tests/resample_ref.py.

Resampled rows are held to the running-error bound of the float64 direct formula; rows of one call are bit-equal to their solo
calls and to the reversed call; everything past a row's length is zero; the normalisation's gain is within 1e-12 of the float64
restatement and its samples within 2 fp32 ulps of that restatement applied to the device's own un-normalised rows; the reference
clip is get_ref_clip of the device's own row; bad arguments are refused by name and leave the handle usable."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import resample_ref as rr
from sparkmi import _lib, audio
from sparkmi.encoder import get_ref_clip

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 65, 333, 4097)          # shorter than the filter's half length, no multiple of the 1024 tile, just over a tile
RATIOS = [rr.ratio(a, b) for a, b in rr.PAIRS]
GARBAGE = 7.5e8


class _Handle:
    def __init__(self, rows=8, n_in=70000, n_out=70000, ratios=RATIOS):
        self.l = _lib.lib()
        self.h = C.c_void_p()
        self.l.check(self.l.smi_rs_create(rows, n_in, n_out, C.byref(self.h)), "smi_rs_create")
        for up, down in ratios:
            t = np.ascontiguousarray(audio.resample_taps(up, down))
            self.l.check(self.l.smi_rs_register(self.h, up, down, t.ctypes.data_as(C.POINTER(C.c_double)), t.size), "smi_rs_register")

    def __del__(self):
        self.l.smi_rs_destroy(self.h)

    @staticmethod
    def _pack(rows, stride, fill=0.0):
        a = np.full((len(rows), stride), fill, np.float32)
        for b, r in enumerate(rows):
            a[b, : r.size] = r
        return torch.from_numpy(a).cuda()

    def raw_resample(self, x_dev, in_stride, n_in, ups, downs, out_dev, out_stride):
        B = len(n_in)
        i32 = lambda v: (C.c_int32 * B)(*v)   # noqa: E731
        return self.l.smi_rs_resample_rows(self.h, C.c_void_p(x_dev.data_ptr()), in_stride, i32(n_in), i32(ups), i32(downs), B,
                                           C.c_void_p(out_dev.data_ptr()), out_stride, None)

    def resample(self, rows, ratios, in_stride=None, out_stride=None):
        """[B] numpy rows through one call: ([B][out_stride] numpy, n_out)"""
        n_in = [r.size for r in rows]
        n_out = [rr.out_len(n, u, d) for n, (u, d) in zip(n_in, ratios)]
        in_stride, out_stride = in_stride or max(n_in), out_stride or max(n_out)
        x = self._pack(rows, in_stride, GARBAGE)
        y = torch.full((len(rows), out_stride), GARBAGE, dtype=torch.float32, device="cuda")
        self.l.check(self.raw_resample(x, in_stride, n_in, [u for u, _ in ratios], [d for _, d in ratios], y, out_stride),
                     "smi_rs_resample_rows")
        return y.cpu().numpy(), n_out

    def prompt(self, rows, ratios, ref_len, normalize=1, wav_stride=None, ref_stride=None):
        """(wav [B][wav_stride], ref [B][ref_stride], gain [B], n_out), numpy"""
        B = len(rows)
        n_in = [r.size for r in rows]
        n_out = [rr.out_len(n, u, d) for n, (u, d) in zip(n_in, ratios)]
        wav_stride, ref_stride = wav_stride or max(n_out), ref_stride or max(ref_len)
        x = self._pack(rows, max(n_in), GARBAGE)
        wav = torch.full((B, wav_stride), GARBAGE, dtype=torch.float32, device="cuda")
        ref = torch.full((B, ref_stride), GARBAGE, dtype=torch.float32, device="cuda")
        gain = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        i32 = lambda v: (C.c_int32 * B)(*v)   # noqa: E731
        got = (C.c_int32 * B)()
        self.l.check(self.l.smi_rs_prompt_rows(self.h, C.c_void_p(x.data_ptr()), max(n_in), i32(n_in), i32([u for u, _ in ratios]),
                                               i32([d for _, d in ratios]), B, normalize, C.c_void_p(wav.data_ptr()), wav_stride,
                                               i32(ref_len), C.c_void_p(ref.data_ptr()), ref_stride, C.c_void_p(gain.data_ptr()), got, None),
                     "smi_rs_prompt_rows")
        assert list(got) == n_out
        return wav.cpu().numpy(), ref.cpu().numpy(), gain.cpu().numpy(), n_out


@functools.lru_cache(maxsize=None)
def _handle():
    return _Handle()


def _signal(seed, n):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.3 * np.sin(2 * np.pi * 0.013 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_rows_within_the_bound(up, down):
    h = _handle()
    rows = [_signal(100 + n, n) for n in LENGTHS]
    y, n_out = h.resample(rows, [(up, down)] * len(rows))
    taps = audio.resample_taps(up, down)
    for b, x in enumerate(rows):
        want, absum, N = rr.direct(x, up, down, taps)
        assert n_out[b] == want.size == _lib.lib().smi_rs_out_len(x.size, up, down)
        err = np.abs(y[b, : n_out[b]].astype(np.float64) - want)
        bound = rr.bound(absum, N)
        print(f"{up}/{down} n={x.size}: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
        assert (err <= bound).all(), (x.size, float((err / np.maximum(bound, 1e-300)).max()))
        assert not y[b, n_out[b]:].any()


def test_ratio_one_is_a_copy():
    rows = [_signal(200 + n, n) for n in LENGTHS]
    y, n_out = _handle().resample(rows, [(1, 1)] * len(rows), out_stride=5000)
    for b, x in enumerate(rows):
        assert n_out[b] == x.size and np.array_equal(y[b, : x.size].view(np.uint32), x.view(np.uint32)) and not y[b, x.size:].any()


MIXED = ((4097, (1, 3)), (333, (160, 441)), (1, (441, 160)), (2500, (3, 2)), (65, (1, 1)))


def test_rows_are_independent_of_the_call():
    h = _handle()
    rows = [_signal(300 + i, n) for i, (n, _) in enumerate(MIXED)]
    ratios = [r for _, r in MIXED]
    y, n_out = h.resample(rows, ratios, in_stride=6000, out_stride=7001)       # padded strides, larger than any row
    yr, _ = h.resample(rows[::-1], ratios[::-1])
    for b, x in enumerate(rows):
        solo, n1 = h.resample([x], [ratios[b]])
        assert n1 == [n_out[b]]
        assert np.array_equal(y[b, : n_out[b]].view(np.uint32), solo[0].view(np.uint32)), b
        assert np.array_equal(yr[len(rows) - 1 - b, : n_out[b]].view(np.uint32), solo[0].view(np.uint32)), b
        assert not y[b, n_out[b]:].any(), b          # the buffer held garbage before the call


def test_padding_is_zeroed_up_to_the_stride():
    h = _handle()
    rows = [_signal(400, 3000), _signal(401, 10)]
    for stride in (1000, 1024, 1025, 2049, 5000):
        y, n_out = h.resample(rows, [(1, 3), (1, 3)], out_stride=stride)
        assert n_out == [1000, 4]
        for b in range(2):
            assert np.isfinite(y[b]).all() and np.abs(y[b, : n_out[b]]).max() < 10 and not y[b, n_out[b]:].any()


# ---- normalisation
@functools.lru_cache(maxsize=None)
def _norm_run():
    """the rows of rr.gain_inputs() (as they are: ratio 1/1) and a 48 kHz noise row, in ONE call with and without normalize"""
    x = rr.gain_inputs()
    names = sorted(x)
    rows = [x[k] for k in names] + [_signal(500, 60000)]
    ratios = [(1, 1)] * len(names) + [(1, 3)]
    names = names + ["noise48k"]
    h = _handle()
    ref_len = [1600] * len(rows)
    plain = h.prompt(rows, ratios, ref_len, normalize=0)
    norm = h.prompt(rows, ratios, ref_len, normalize=1)
    return names, rows, ratios, plain, norm


@pytest.mark.parametrize("i", range(7))
def test_normalize(i):
    names, rows, ratios, plain, norm = _norm_run()
    n = plain[3][i]
    raw = plain[0][i, :n]
    assert plain[2][i] == 1.0
    if ratios[i] == (1, 1):
        assert np.array_equal(raw.view(np.uint32), rows[i].view(np.uint32))
    want, gain = rr.normalize_ref(raw)
    got, g = norm[0][i, :n], float(norm[2][i])
    print(f"{names[i]}: gain {g!r} against {gain!r}, relative difference {abs(g - gain) / abs(gain):.2e}")
    assert abs(g - gain) <= rr.GAIN_RTOL * abs(gain), (names[i], g, gain)
    assert (np.abs(got.astype(np.float64) - want) <= 2.0 ** -22 * np.abs(want)).all(), names[i]
    assert not norm[0][i, n:].any()
    # the row alone: the same bits in samples, reference clip and gain
    w1, r1, g1, _ = _handle().prompt([rows[i]], [ratios[i]], [1600], normalize=1)
    assert np.array_equal(w1[0].view(np.uint32), got.view(np.uint32)) and g1[0] == norm[2][i]
    assert np.array_equal(r1[0].view(np.uint32), norm[1][i].view(np.uint32))


def test_normalize_takes_every_branch():
    names, _, _, plain, norm = _norm_run()
    g = dict(zip(names, norm[2]))
    assert g["sparse"] == 1.0 and 1.0 < g["loud"] < 10.0 and g["quiet"] > 1.25 and g["noise"] != g["edge"]


# ---- reference clip
@pytest.mark.parametrize("normalize", [0, 1])
def test_reference_clip_is_get_ref_clip_of_the_device_row(normalize):
    lens = (999, 700, 220, 5000, 1600)        # tiled once, twice and 7 times with a remainder; longer than the clip; exactly the clip
    rows = [_signal(600 + n, n) for n in lens]
    wav, ref, _, n_out = _handle().prompt(rows, [(1, 1)] * len(rows), [1600] * len(rows), normalize=normalize, ref_stride=1700)
    for b, n in enumerate(lens):
        want = get_ref_clip(wav[b, :n], 16000, 0.1, 1)
        assert want.size == 1600 and np.array_equal(ref[b, :1600].view(np.uint32), want.view(np.uint32)), n
        assert not ref[b, 1600:].any()
    # rows with reference lengths of their own, after a resampling stage
    rows = [_signal(700, 3000), _signal(701, 900)]
    wav, ref, _, n_out = _handle().prompt(rows, [(1, 3), (160, 441)], [2500, 64], normalize=normalize)
    for b, rl in enumerate((2500, 64)):
        assert np.array_equal(ref[b, :rl].view(np.uint32), rr.ref_clip(wav[b, : n_out[b]], rl).view(np.uint32)) and not ref[b, rl:].any()


# ---- validation
def test_bad_arguments_are_refused_by_name_and_nothing_breaks():
    l = _lib.lib()
    h = _Handle(rows=2, n_in=5000, n_out=5000, ratios=[(1, 3)])
    x = torch.zeros((3, 5000), dtype=torch.float32, device="cuda")
    y = torch.full((3, 5000), GARBAGE, dtype=torch.float32, device="cuda")

    def refused(word, n_in, ups, downs, out_stride=5000):
        assert h.raw_resample(x, 5000, n_in, ups, downs, y, out_stride) == -1
        msg = l.smi_last_error().decode()
        assert word in msg, msg

    refused("not registered", [100], [160], [441])                 # an unregistered ratio
    refused("n_in[1]", [100, 5001], [1, 1], [3, 3])                # a row longer than the reservation
    refused("out_stride", [5000], [1], [1], out_stride=4000)            # ... and one longer than its stride
    refused("B=3", [10, 10, 10], [1, 1, 1], [3, 3, 3])             # B over the reservation
    refused("up[0]", [10], [0], [3])
    taps = np.ones(4)
    assert l.smi_rs_register(h.h, 2, 3, taps.ctypes.data_as(C.POINTER(C.c_double)), 4) == -1 and b"n_taps" in l.smi_last_error()
    big = _Handle(rows=1, n_in=1 << 24, n_out=1 << 24, ratios=[])
    assert big.raw_resample(x, 1 << 24, [1 << 23], [441], [160], y, 1 << 24) == -1 and b"2^31" in l.smi_last_error()
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == np.float32(GARBAGE)).all()           # nothing was launched
    # a valid call still works
    row = _signal(800, 3000)
    got, n_out = h.resample([row], [(1, 3)])
    want, absum, N = rr.direct(row, 1, 3, audio.resample_taps(1, 3))
    assert n_out == [1000] and (np.abs(got[0].astype(np.float64) - want) <= rr.bound(absum, N)).all()
