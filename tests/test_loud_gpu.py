"""smi_loud_rows and smi_gain_rows through the C ABI against tests/loud_ref.py: loudness and gain within the tolerance derived
in tests/test_loud_cpu.py, peak and limit exactly, the scaled samples bit for bit, and a row's stats as its own."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import loud_ref as R
from sparkmi import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GARBAGE = 7.5e8
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _f64(v):
    v = [float(a) for a in v]
    return (C.c_double * len(v))(*v)


def _groups():
    g = {}
    for c in R.reference():
        g.setdefault((c["sr"], c["block"]), []).append(c)
    return g


GROUPS = sorted(_groups())


def _pack(cs, lead=0, trail=0, extra=0, fill=0.0):
    """rows [fill * lead | span | fill * trail], then `extra` more columns of fill past the longest row"""
    n = [lead + c["x"].size + trail for c in cs]
    x = np.full((len(cs), max(n + [1]) + extra), fill, dtype=np.float32)
    for b, c in enumerate(cs):
        x[b, lead: lead + c["x"].size] = c["x"]
    spans = [(lead, lead + c["x"].size) for c in cs]
    return x, n, spans


def loud(x_dev, n, spans, coef, block, targets, max_gain_db, ceiling, B=None, work_len=None, rc_only=False):
    l = _lib.lib()
    B = len(n) if B is None else B
    need = l.smi_loud_work_len(max([v for v in n if v >= 0] + [0]), block if block >= 4 and block % 4 == 0 else 4, max(1, min(B, 64)))
    work = torch.full((max(1, need if work_len is None else work_len),), math.nan, dtype=torch.float64, device=DEV)
    stats = torch.full((max(1, B), 4), SENTINEL, dtype=torch.float64, device=DEV)
    st = None if spans is None else _i32(s[0] for s in spans)
    en = None if spans is None else _i32(s[1] for s in spans)
    rc = l.smi_loud_rows(C.c_void_p(x_dev.data_ptr()), x_dev.shape[1], _i32(n), st, en, B, _f64(coef), block, _f64(targets), float(max_gain_db),
                         float(ceiling), C.c_void_p(work.data_ptr()), work.numel() if work_len is None else work_len,
                         C.c_void_p(stats.data_ptr()), None)
    if rc_only:
        torch.cuda.synchronize()
        return rc, l.smi_last_error().decode(), stats.cpu().numpy()
    l.check(rc, "smi_loud_rows")
    return stats


def measure(cs, **pack):
    """the stats of the cases `cs` (one coefficient set, block and limits) as one call"""
    x, n, spans = _pack(cs, **pack)
    xd = torch.from_numpy(x).to(DEV)
    c0 = cs[0]
    whole = not pack.get("lead") and not pack.get("trail")
    stats = loud(xd, n, None if whole else spans, c0["coef"], c0["block"], [c["target"] for c in cs], c0["max_gain_db"], c0["ceiling"])
    return stats, xd, x, n, spans


def gain_rows(xd, n, spans, stats, out=None, out_stride=None, B=None, rc_only=False):
    l = _lib.lib()
    B = len(n) if B is None else B
    if out is None:
        out = torch.full((max(1, B), xd.shape[1] if out_stride is None else out_stride), 9.0, dtype=torch.float32, device=DEV)
    st = None if spans is None else _i32(s[0] for s in spans)
    en = None if spans is None else _i32(s[1] for s in spans)
    rc = l.smi_gain_rows(C.c_void_p(xd.data_ptr()), xd.shape[1], _i32(n), st, en, B, C.c_void_p(stats.data_ptr()), C.c_void_p(out.data_ptr()),
                         out.shape[1] if out.dim() == 2 else out_stride, None)
    if rc_only:
        torch.cuda.synchronize()
        return rc, l.smi_last_error().decode()
    l.check(rc, "smi_gain_rows")
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("key", GROUPS, ids=[f"{sr}Hz-block{b}" for sr, b in GROUPS])
def test_stats_match_the_reference(key):
    cs = _groups()[key]
    got = measure(cs)[0].cpu().numpy()
    for c, (loudness, peak, g, limit) in zip(cs, got):
        print(f"{c['name']}: L={c['x'].size} loudness {loudness!r} (ref {float(c['loudness'])!r}) peak {peak!r} gain {g!r} limit {limit}")
        if c["loudness"] == -math.inf:
            assert loudness == -math.inf and g == 1.0 and limit == 0.0
        else:
            assert abs(np.longdouble(loudness) - c["loudness"]) <= R.TOL_LU, c["name"]
            assert abs(np.longdouble(g) / c["gain"] - 1) <= R.TOL_GAIN, c["name"]
            assert limit == c["limit"], c["name"]
        assert peak == c["peak"], c["name"]
    # what lies outside the span is never read: garbage before start, after end, past n and in a longer stride changes no bit
    dirty = measure(cs, lead=37, trail=11, extra=333, fill=GARBAGE)[0].cpu().numpy()
    assert np.array_equal(_bits(dirty), _bits(got))
    # a row's stats are its own: alone, among five, in the reversed call
    pick = [i % len(cs) for i in (2, 5, len(cs) - 1, 8, 0)]
    pick = pick if len(cs) >= 5 else list(range(len(cs)))
    some = measure([cs[i] for i in pick])[0].cpu().numpy()
    assert np.array_equal(_bits(some), _bits(got[pick]))
    assert np.array_equal(_bits(measure([cs[i] for i in pick[::-1]])[0].cpu().numpy()), _bits(some[::-1]))
    for i in pick[:3]:
        assert np.array_equal(_bits(measure([cs[i]])[0].cpu().numpy()), _bits(got[i: i + 1]))


@pytest.mark.parametrize("key", GROUPS[:2], ids=[f"{sr}Hz-block{b}" for sr, b in GROUPS[:2]])
def test_gain_rows_scales_the_span_bit_for_bit(key):
    cs = _groups()[key]
    stats, xd, x, n, spans = measure(cs, lead=5, trail=9, extra=13, fill=0.25)
    g = stats.cpu().numpy()[:, 2]
    want = np.zeros_like(x)
    for b, (a, e) in enumerate(spans):
        want[b, : n[b]] = x[b, : n[b]]
        want[b, a:e] = R.apply_gain(x[b, a:e], g[b])
    out = gain_rows(xd, n, spans, stats)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))        # the span scaled, the rest copied, zeros past n
    wide = gain_rows(xd, n, spans, stats, out_stride=x.shape[1] + 1029).cpu().numpy()
    assert np.array_equal(_bits(wide[:, : x.shape[1]]), _bits(want)) and not wide[:, x.shape[1]:].any()
    inplace = xd.clone()
    assert gain_rows(inplace, n, spans, stats, out=inplace) is inplace
    assert np.array_equal(_bits(inplace.cpu().numpy()), _bits(want))
    # null spans: the whole row is the span
    whole = gain_rows(xd, n, None, stats).cpu().numpy()
    for b in range(len(cs)):
        assert np.array_equal(_bits(whole[b, : n[b]]), _bits(R.apply_gain(x[b, : n[b]], g[b]))) and not whole[b, n[b]:].any()


def test_refusals_name_their_argument_and_launch_nothing():
    cs = [c for c in R.reference() if c["name"] in ("loud_quiet_loud", "len129")]
    x, n, spans = _pack(cs, lead=3, trail=2)
    xd = torch.from_numpy(x).to(DEV)
    c0 = cs[0]
    ok = dict(coef=c0["coef"], block=c0["block"], targets=[-23.0, -23.0], max_gain_db=20.0, ceiling=0.9)

    def refused(word, n=n, spans=spans, **kw):
        a = dict(ok, **kw)
        rc, err, stats = loud(xd, n, spans, a["coef"], a["block"], a["targets"], a["max_gain_db"], a["ceiling"], B=a.get("B"),
                              work_len=a.get("work_len"), rc_only=True)
        assert rc == EINVAL and word in err, (word, rc, err)
        assert (stats == SENTINEL).all(), word      # nothing was launched

    refused("B=0", B=0)
    refused("B=65", B=65)
    refused("n[1]", n=[n[0], -1])
    refused("end[0]", spans=[(spans[0][1], spans[0][0]), spans[1]])
    refused("end[1]", spans=[spans[0], (0, n[1] + 1)])
    refused("block", block=66)
    refused("block", block=0)
    refused("work_len", work_len=7)
    bad = np.array(c0["coef"])
    bad[3] = math.inf
    refused("coef[3]", coef=bad)
    bad[3] = math.nan
    refused("coef[3]", coef=bad)
    refused("ceiling", ceiling=0.0)
    refused("ceiling", ceiling=-1.0)
    refused("max_gain_db", max_gain_db=-0.5)
    refused("target[1]", targets=[-23.0, math.inf])
    # the next valid call works
    stats = loud(xd, n, spans, ok["coef"], ok["block"], ok["targets"], ok["max_gain_db"], ok["ceiling"])
    assert [c["sr"] for c in cs] == [16000, 16000]
    for b, c in enumerate(cs):
        assert abs(np.longdouble(stats.cpu().numpy()[b, 0]) - c["loudness"]) <= R.TOL_LU, c["name"]
    # smi_gain_rows: an output that overlaps the input other than row on row
    flat = torch.zeros(4 * x.shape[1] + 8, dtype=torch.float32, device=DEV)
    src = flat[: 2 * x.shape[1]].view(2, -1)
    src.copy_(xd)
    for off in (1, x.shape[1]):
        rc, err = gain_rows(src, n, spans, stats, out=flat[off: off + 2 * x.shape[1]].view(2, -1), rc_only=True)
        assert rc == EINVAL and "out_dev" in err
    rc, err = gain_rows(src, n, spans, stats, out=flat[: 2 * x.shape[1] + 2].view(2, -1), rc_only=True)   # same start, another stride
    assert rc == EINVAL and "out_dev" in err
    rc, err = gain_rows(src, n, spans, stats, B=0, rc_only=True)
    assert rc == EINVAL and "B=0" in err
    assert np.array_equal(src.cpu().numpy(), x)     # none of them wrote
    assert _lib.lib().smi_loud_work_len(1000, 66, 1) == -1 and _lib.lib().smi_loud_work_len(-1, 64, 1) == -1
    assert _lib.lib().smi_loud_work_len(1000, 64, 65) == -1 and _lib.lib().smi_loud_work_len(0, 64, 1) >= 1


def test_device_audio_gives_the_raw_calls_results():
    from sparkmi.audio import DeviceAudio, k_weighting
    cs = _groups()[(16000, R.SMALL_BLOCK)]
    stats, xd, x, n, spans = measure(cs, lead=4, trail=4)
    da = DeviceAudio(DEV)
    mine = da.loudness_rows(xd, n, spans=spans, targets=[None if math.isnan(c["target"]) else c["target"] for c in cs],
                            max_gain_db=cs[0]["max_gain_db"], ceiling=cs[0]["ceiling"], sr=16000, block=R.SMALL_BLOCK)
    assert np.array_equal(_bits(mine.cpu().numpy()), _bits(stats.cpu().numpy()))
    want = gain_rows(xd, n, spans, stats).cpu().numpy()
    assert np.array_equal(_bits(da.gain_rows(xd, n, mine, spans=spans).cpu().numpy()), _bits(want))
    y = xd.clone()
    assert da.gain_rows(y, n, mine, spans=spans, out=y) is y and np.array_equal(_bits(y.cpu().numpy()), _bits(want))
    # the defaults: sr gives the coefficients and the block; no targets: measure only
    real = _groups()[(16000, 6400)]
    ref = measure(real)
    only = da.loudness_rows(ref[1], ref[3], sr=16000).cpu().numpy()
    assert np.array_equal(_bits(only[:, :2]), _bits(ref[0].cpu().numpy()[:, :2])) and only[0, 2] == 1.0 and only[0, 3] == 0.0
    assert np.array_equal(k_weighting(16000), real[0]["coef"])
