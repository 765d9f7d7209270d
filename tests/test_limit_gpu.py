"""smi_limit_rows through the C ABI against tests/limit_ref.py: the limited rows and the four stats bit for bit, for every
committed case; a row's bits as its own (alone, among five, reversed, garbage outside the span, a longer stride); in place; the
three ways a gain arrives; a NaN-filled work buffer; zeros past n; and refusals that launch nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import limit_ref as R
from sparkmi import _lib, audio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GARBAGE = 7.5e8
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _f64(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return (C.c_double * v.size)(*v.tolist())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _groups():
    g = {}
    for c in R.reference():
        g.setdefault((c["ceiling"], c["mode"], c["A"], c["R"]), []).append(c)
    return g


GROUPS = sorted(_groups())
IDS = [f"{m}-A{a}-R{r}-c{c:.3f}" for c, m, a, r in GROUPS]


def _pack(cs, lead=0, trail=0, extra=0, fill=0.0):
    """rows [fill * lead | span | fill * trail], then `extra` more columns of fill past the longest row; the rows expected back"""
    n = [lead + c["x"].size + trail for c in cs]
    x = np.full((len(cs), max(n + [1]) + extra), fill, dtype=np.float32)
    want = np.zeros_like(x)
    for b, c in enumerate(cs):
        x[b, lead: lead + c["x"].size] = c["x"]
        want[b, : n[b]] = x[b, : n[b]]
        want[b, lead: lead + c["x"].size] = c["want"]["out"]
    spans = [(lead, lead + c["x"].size) for c in cs]
    return x, n, spans, want


def limit(xd, n, spans, key, gains="plain", g=None, out=None, out_stride=None, B=None, work_len=None, rc_only=False, **bad):
    """one smi_limit_rows call for rows of one (ceiling, mode, A, R); gains: "plain" [B] float64, "stats" (the loudness layout:
    [B][4], the gain third), or None (the rows' gain is 1)"""
    l = _lib.lib()
    ceiling, mode, A, Rr = key
    B = len(n) if B is None else B
    h = R.taps() if mode == "true" else None
    w = bad.get("win", audio.limiter_window(A, Rr))
    need = l.smi_limit_work_len(max([v for v in n if v >= 0] + [0]), max(1, min(B, 64)))
    work = torch.full((max(1, need),), math.nan, dtype=torch.float64, device=DEV)
    stats = torch.full((max(1, B), 4), SENTINEL, dtype=torch.float64, device=DEV)
    if out is None:
        out = torch.full((max(1, len(n)), xd.shape[1] if out_stride is None else out_stride), 9.0, dtype=torch.float32, device=DEV)
    gp, gs, keep = C.c_void_p(0), 0, None
    if gains == "plain":
        keep = torch.tensor([float(v) for v in g], dtype=torch.float64, device=DEV)
        gp, gs = C.c_void_p(keep.data_ptr()), 1
    elif gains == "stats":
        keep = torch.full((len(g), 4), GARBAGE, dtype=torch.float64, device=DEV)
        keep[:, 2] = torch.tensor([float(v) for v in g], dtype=torch.float64, device=DEV)
        gp, gs = C.c_void_p(keep.data_ptr() + 16), 4
    st = None if spans is None else _i32(s[0] for s in spans)
    en = None if spans is None else _i32(s[1] for s in spans)
    rc = l.smi_limit_rows(C.c_void_p(xd.data_ptr()), xd.shape[1], _i32(n), st, en, B, gp, bad.get("gain_stride", gs), float(bad.get("ceiling", ceiling)),
                          None if h is None else _f64(h), bad.get("n_taps", 0 if h is None else h.size), bad.get("phases", R.PHASES),
                          bad.get("A", A), bad.get("R", Rr), _f64(w), C.c_void_p(work.data_ptr()), work.numel() if work_len is None else work_len,
                          C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(stats.data_ptr()), None)
    if rc_only:
        torch.cuda.synchronize()
        return rc, l.smi_last_error().decode(), out, stats.cpu().numpy()
    l.check(rc, "smi_limit_rows")
    return out, stats


def run(cs, key, gains="plain", **pack):
    x, n, spans, want = _pack(cs, **pack)
    xd = torch.from_numpy(x).to(DEV)
    whole = not pack.get("lead") and not pack.get("trail")
    out, stats = limit(xd, n, None if whole else spans, key, gains=gains, g=[c["g"] for c in cs])
    return out.cpu().numpy(), stats.cpu().numpy(), want, xd, n, spans


def _same(got, want, what):
    bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
    assert bad.size == 0, f"{what}: {bad.size} values differ, the first at {bad[:5]}: {got.ravel()[bad[:5]]!r} for {want.ravel()[bad[:5]]!r}"


@pytest.mark.parametrize("key", GROUPS, ids=IDS)
def test_rows_and_stats_match_the_reference_bit_for_bit(key):
    cs = _groups()[key]
    out, stats, want, *_ = run(cs, key)
    for b, c in enumerate(cs):
        print(f"{c['name']}: L={c['x'].size} g={c['g']} stats {stats[b].tolist()} (ref {c['want']['stats'].tolist()})")
    for b, c in enumerate(cs):
        _same(stats[b], c["want"]["stats"], f"{c['name']}: stats")
        _same(out[b], want[b], f"{c['name']}: row")           # (the columns past n are zeros: the output was filled with 9)
    assert (np.abs(out.astype(np.float64)) <= key[0]).all()


@pytest.mark.parametrize("key", GROUPS, ids=IDS)
def test_a_rows_bits_are_its_own(key):
    cs = _groups()[key]
    out, stats, want, *_ = run(cs, key)
    # garbage before the span, behind it, past n and in a longer stride: never read, and copied through; the span starts off a tile
    for lead, trail, extra in ((37, 11, 333), (R.TILE - 1, 1, 0), (R.TILE + 1, 0, 1029)):
        o2, s2, w2, *_ = run(cs, key, lead=lead, trail=trail, extra=extra, fill=GARBAGE)
        _same(s2, stats, f"stats with garbage around, lead {lead}")
        _same(o2, w2, f"rows with garbage around, lead {lead}")
    # alone, among five, in the reversed call
    pick = [i % len(cs) for i in (2, 5, len(cs) - 1, 8, 0)]
    pick = pick if len(cs) >= 5 else list(range(len(cs)))
    o5, s5, w5, *_ = run([cs[i] for i in pick], key)
    _same(s5, stats[pick], "stats among five")
    _same(o5, w5, "rows among five")
    o5r, s5r, w5r, *_ = run([cs[i] for i in pick[::-1]], key)
    _same(s5r, s5[::-1], "stats reversed")
    _same(o5r, w5r, "rows reversed")
    for i in pick[:3]:
        o1, s1, w1, *_ = run([cs[i]], key)
        _same(s1[0], stats[i], "stats alone")
        _same(o1, w1, "row alone")


@pytest.mark.parametrize("key", GROUPS[:3], ids=IDS[:3])
def test_in_place_wide_output_and_the_ways_a_gain_arrives(key):
    cs = _groups()[key]
    out, stats, want, xd, n, spans = run(cs, key, lead=5, trail=9, extra=13, fill=0.25)
    _same(out, want, "rows")
    g = [c["g"] for c in cs]
    inplace = xd.clone()
    o, s = limit(inplace, n, spans, key, g=g, out=inplace)
    assert o is inplace
    _same(inplace.cpu().numpy(), want, "in place")
    _same(s.cpu().numpy(), stats, "stats in place")
    wide, s = limit(xd, n, spans, key, g=g, out_stride=xd.shape[1] + 1029)
    wide = wide.cpu().numpy()
    _same(wide[:, : xd.shape[1]], want, "wide")
    assert not wide[:, xd.shape[1]:].any()
    # the gain read from a loudness-stats layout gives the same bits as from a plain array
    o, s = limit(xd, n, spans, key, gains="stats", g=g)
    _same(o.cpu().numpy(), want, "gain from stats")
    _same(s.cpu().numpy(), stats, "stats, gain from stats")
    # a null gain is g = 1
    unit = [i for i, c in enumerate(cs) if c["g"] == 1.0]
    if unit:
        x1, n1, sp1, w1 = _pack([cs[i] for i in unit], lead=5, trail=9)
        o, s = limit(torch.from_numpy(x1).to(DEV), n1, sp1, key, gains=None)
        _same(o.cpu().numpy(), w1, "null gain")
        _same(s.cpu().numpy(), stats[unit], "stats, null gain")


def test_the_inter_sample_over_is_limited_in_true_mode_only():
    ref = {c["name"]: c for c in R.reference()}
    t, s = ref["quarter_true"], ref["quarter_sample"]
    ot, st, *_ = run([t], (t["ceiling"], "true", t["A"], t["R"]))
    os_, ss, *_ = run([s], (s["ceiling"], "sample", s["A"], s["R"]))
    assert st[0, 0] > t["ceiling"] > np.abs(t["x"]).max() and st[0, 2] < 1 and st[0, 3] > 500
    assert np.abs(ot[0]).max() < np.abs(t["x"]).max()
    assert ss[0, 2] == 1.0 and ss[0, 3] == 0.0
    _same(os_[0, : s["x"].size], s["x"], "sample mode leaves the row as it is")


def test_null_spans_are_the_whole_rows():
    key = GROUPS[0]
    cs = _groups()[key][:4]
    x, n, spans, want = _pack(cs)
    o, s = limit(torch.from_numpy(x).to(DEV), n, None, key, g=[c["g"] for c in cs])
    _same(o.cpu().numpy(), want, "null spans")


def test_refusals_name_their_argument_and_launch_nothing():
    key = (R.CEILING, "true", R.A0, R.R0)
    cs = [c for c in R.reference() if c["name"] in ("two_close", "len1025")]
    x, n, spans, want = _pack(cs, lead=3, trail=2)
    xd = torch.from_numpy(x).to(DEV)
    g = [c["g"] for c in cs]

    def refused(word, n=n, spans=spans, **kw):
        rc, err, out, stats = limit(xd, n, spans, key, g=g, rc_only=True, **kw)
        assert rc == EINVAL and word in err, (word, rc, err)
        assert (stats == SENTINEL).all() and (out.cpu().numpy() == 9.0).all(), word      # nothing was launched

    refused("B=0", B=0)
    refused("B=65", B=65)
    refused("n[1]", n=[n[0], -1])
    refused("end[0]", spans=[(spans[0][1], spans[0][0]), spans[1]])
    refused("lookahead", A=-1)
    refused("release", R=2049)
    refused("win sums", win=audio.limiter_window(R.A0, R.R0) * 1.001)
    refused("n_taps", phases=5)
    refused("ceiling", ceiling=0.0)
    refused("work_len", work_len=7)
    flat = torch.zeros(4 * x.shape[1] + 8, dtype=torch.float32, device=DEV)
    src = flat[: 2 * x.shape[1]].view(2, -1)
    src.copy_(xd)
    for off in (1, x.shape[1]):
        rc, err, _, stats = limit(src, n, spans, key, g=g, out=flat[off: off + 2 * x.shape[1]].view(2, -1), rc_only=True)
        assert rc == EINVAL and "out_dev" in err and (stats == SENTINEL).all()
    assert np.array_equal(src.cpu().numpy(), x)     # none of them wrote
    out, stats = limit(xd, n, spans, key, g=g)        # the next valid call works
    _same(out.cpu().numpy(), want, "after the refusals")


def test_device_audio_gives_the_raw_calls_results():
    key = (R.CEILING, "true", R.A0, R.R0)
    cs = _groups()[key][:12]
    out, stats, want, xd, n, spans = run(cs, key, lead=4, trail=4)
    da = audio.DeviceAudio(DEV)
    gains = torch.tensor([c["g"] for c in cs], dtype=torch.float64, device=DEV)
    o, s = da.limit_rows(xd, n, gains=gains, spans=spans)
    _same(o.cpu().numpy(), want, "DeviceAudio.limit_rows")
    _same(s.cpu().numpy(), stats, "DeviceAudio.limit_rows stats")
    four = torch.zeros((len(cs), 4), dtype=torch.float64, device=DEV)
    four[:, 2] = gains
    y = xd.clone()
    o, s = da.limit_rows(y, n, gains=four, spans=spans, out=y)
    assert o is y
    _same(y.cpu().numpy(), want, "in place, gains from a stats tensor")
    sm = [c for c in R.reference() if c["name"] == "sample_mode"]
    x1, n1, sp1, w1 = _pack(sm)
    o, s = da.limit_rows(torch.from_numpy(x1).to(DEV), n1, gains=torch.tensor([sm[0]["g"]], dtype=torch.float64, device=DEV), mode="sample")
    _same(o.cpu().numpy(), w1, "sample mode")
    with pytest.raises(ValueError):
        da.limit_rows(xd, n, mode="peak")
