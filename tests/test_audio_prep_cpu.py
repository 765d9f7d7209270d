"""The device audio path's arithmetic, pinned on the host: the numpy-only taps against scipy's firwin, the direct formula of
tests/resample_ref.py against scipy.signal.resample_poly, the resampling bound (an fp32 emulation in the device's order stays
inside, three wrong results fall outside), the gain bound (the device's integer route to the statistic stays inside 1e-12, three
wrong restatements fall outside) and DeviceAudio's bookkeeping on a stand-in library."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as rr
from sparkmi import audio
from sparkmi.encoder import audio_volume_normalize, get_ref_clip

LENGTHS = (1, 7, 333, 1500)


def _ratios():
    return [rr.ratio(a, b) for a, b in rr.PAIRS]


def test_ratio_reduces_to_lowest_terms():
    assert audio.ratio(48000, 16000) == (1, 3) and audio.ratio(44100, 16000) == (160, 441)
    assert audio.ratio(16000, 44100) == (441, 160) and audio.ratio(16000, 16000) == (1, 1)
    assert audio.ratio(22050, 16000) == (320, 441) and audio.ratio(16000, 24000) == (3, 2)
    assert [audio.ratio(a, b) for a, b in rr.PAIRS] == _ratios()
    with pytest.raises(ValueError):
        audio.ratio(0, 16000)
    with pytest.raises(ValueError):
        audio.resample_taps(2, 4)


@pytest.mark.parametrize("up,down", _ratios())
def test_taps_equal_firwin(up, down):
    signal = pytest.importorskip("scipy.signal")
    half = 10 * max(up, down)
    want = signal.firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    got = audio.resample_taps(up, down)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-15


@pytest.mark.parametrize("up,down", _ratios())
def test_direct_formula_equals_resample_poly(up, down):
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(up * 1000 + down)
    h = signal.firwin(2 * 10 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    for n in LENGTHS:
        x = rng.standard_normal(n)
        want = signal.resample_poly(x, up, down)
        got, _, _ = rr.direct(x, up, down, h)
        assert got.shape == want.shape == (audio.out_len(n, up, down),) == (rr.out_len(n, up, down),)
        assert np.abs(got - want).max() <= 1e-13


def test_out_len_of_the_library_agrees():
    from sparkmi import _lib
    l = _lib.lib()
    for up, down in _ratios() + [(1, 1)]:
        for n in (0, 1, 7, 333, 1500, 480000):
            assert l.smi_rs_out_len(n, up, down) == audio.out_len(n, up, down)
    assert l.smi_rs_out_len(-1, 1, 3) == -1 and l.smi_rs_out_len(5, 0, 3) == -1


def _signal(rng, n):
    t = np.arange(n)
    return (0.3 * np.sin(2 * np.pi * 0.013 * t) + 0.1 * rng.standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("up,down", _ratios())
def test_resampling_bound_holds_for_the_device_order_and_rejects_wrong_results(up, down):
    rng = np.random.default_rng(7 + up + down)
    h = audio.resample_taps(up, down)
    x = _signal(rng, 1500)
    y_ref, absum, N = rr.direct(x, up, down, h)
    b = rr.bound(absum, N)
    err = np.abs(rr.emulate_fp32(x, up, down, h).astype(np.float64) - y_ref)
    assert (err <= b).all(), float((err / np.maximum(b, 1e-300)).max())
    for wrong in (dict(tap_shift=1), dict(drop_last=True), dict(phase_shift=1)):
        y_bad = rr.direct(x, up, down, h, **wrong)[0]
        outside = np.abs(y_bad - y_ref) > b
        assert outside.mean() > 0.01, (wrong, float(outside.mean()))


_gain_inputs = rr.gain_inputs


def test_restatement_is_audio_volume_normalize():
    for name, y in _gain_inputs().items():
        got, gain = rr.normalize_ref(y)
        want = audio_volume_normalize(y.astype(np.float64))
        assert np.array_equal(got, want), name
        nz = y != 0
        assert np.allclose(got[nz] / y[nz].astype(np.float64), gain, rtol=1e-14, atol=0), name


def test_gain_inputs_take_every_branch():
    g = {k: rr.normalize_ref(v)[1] for k, v in _gain_inputs().items()}
    x = _gain_inputs()
    assert np.abs(x["quiet"]).max() < 0.1 and (np.abs(x["sparse"]) > 0.01).sum() <= 10 and g["sparse"] == 1.0
    assert np.abs(x["loud"]).max() * g["loud"] == pytest.approx(1.0, abs=1e-12) and g["loud"] < 10
    assert np.unique(np.abs(x["q8"])).size <= 128


@pytest.mark.parametrize("name", ["noise", "quiet", "q8", "loud", "edge", "sparse"])
def test_gain_bound_holds_for_the_fixed_point_route(name):
    y = _gain_inputs()[name]
    want = rr.normalize_ref(y)[1]
    got = rr.fixed_point_gain(y)
    assert abs(got - want) <= rr.GAIN_RTOL * abs(want), (got, want)


def test_gain_bound_rejects_wrong_restatements():
    """either rank off by one, or the filter made >=, moves the gain by more than 1e-12 on these rows (the filter needs samples
    that are exactly 0.01, which only a float64 row can hold)"""
    rng = np.random.default_rng(5)
    y = 0.2 * rng.standard_normal(20000)
    y[:300] = 0.01
    want = rr.normalize_ref(y)[1]
    for wrong in (dict(lo_shift=1), dict(lo_shift=-1), dict(hi_shift=1), dict(hi_shift=-1), dict(inclusive=True)):
        bad = rr.normalize_ref(y, **wrong)[1]
        assert abs(bad - want) > rr.GAIN_RTOL * abs(want), wrong
    for name in ("noise", "q8"):
        y32 = _gain_inputs()[name]
        want = rr.normalize_ref(y32)[1]
        for wrong in (dict(lo_shift=1), dict(lo_shift=-1), dict(hi_shift=1), dict(hi_shift=-1)):
            assert abs(rr.normalize_ref(y32, **wrong)[1] - want) > rr.GAIN_RTOL * abs(want), (name, wrong)


def test_ref_clip_restatement_is_get_ref_clip():
    rng = np.random.default_rng(3)
    for n_wav, n_ref in ((1000, 1000), (999, 1600), (700, 1600), (220, 1600), (5000, 1600)):
        w = rng.standard_normal(n_wav).astype(np.float32)
        assert np.array_equal(rr.ref_clip(w, n_ref), get_ref_clip(w, 16000, n_ref / 16000.0, 1)), (n_wav, n_ref)


class _FakeLib:
    """the four host-side entry points DeviceAudio's bookkeeping uses"""

    def __init__(self):
        self.created, self.destroyed, self.registered = [], 0, []

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_rs_create(self, rows, n_in, n_out, out):
        self.created.append((rows, n_in, n_out))
        out._obj.value = len(self.created)
        return 0

    def smi_rs_destroy(self, h):
        self.destroyed += 1
        return 0

    def smi_rs_register(self, h, up, down, taps, n):
        assert n == 2 * 10 * max(up, down) + 1
        self.registered.append((h.value, up, down))
        return 0


def test_device_audio_bookkeeping():
    lib = _FakeLib()
    a = audio.DeviceAudio("cuda:0", lib=lib)
    a.reserve(2, 1000, 400)
    assert a.reserved == (2, 1000, 400) and lib.created == [(2, 1000, 400)]
    a.register(1, 3)
    a.register(1, 3)          # once a ratio
    a.register(1, 1)          # a copy needs no filter
    assert lib.registered == [(1, 1, 3)] and a.registered == {(1, 3)}
    a.reserve(1, 500, 400)    # fits: nothing happens
    assert len(lib.created) == 1 and lib.destroyed == 0 and a.registered == {(1, 3)}
    a.reserve(3, 800, 900)    # grows in every dimension that needs it, never shrinks; a new handle forgets the ratios
    assert a.reserved == (3, 1000, 900) and lib.created[-1] == (3, 1000, 900) and lib.destroyed == 1 and a.registered == set()
    assert a._prepare([300, 441], [1, 160], [3, 441]) == [100, 160]
    assert lib.registered[1:] == [(2, 1, 3), (2, 160, 441)] and len(lib.created) == 2
    with pytest.raises(ValueError, match="at most"):
        a.reserve(audio.MAX_ROWS + 1, 10, 10)
    with pytest.raises(ValueError):
        a._prepare([10], [1, 1], [1])
    a.close()
    assert lib.destroyed == 2 and not a._h
