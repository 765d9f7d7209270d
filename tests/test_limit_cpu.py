"""The limiter on the host: tests/limit_ref.py held to the claims of include/sparkmi.h (s <= r, the ceiling exactly, gain_rows'
bits away from the overs, nothing outside the span matters), the true peak of its output re-measured, the wrong variants the
committed cases must tell apart, the window and reach helpers, and every argument smi_limit_rows refuses (host only: a refused
call launches nothing)."""
import ctypes as C
import math

import numpy as np
import pytest

import limit_ref as R
from sparkmi import _lib, audio

EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
# the largest true peak of a limited output over the ceiling, relative, over the "true" cases of each reach (A, R), as
# test_true_peak_of_the_output_is_remeasured prints it; DESIGN.md 4.1.7 records the same figures
OVERSHOOT = {(0, 0): 4.330e-01, (3, 5): 8.913e-03, (40, 400): 1.496e-08, (256, 2048): 3.752e-08}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def test_window_and_reach():
    assert audio.limiter_reach(16000) == (40, 400) and audio.limiter_reach(24000) == (60, 600)
    assert audio.limiter_reach(16000, 0, 0) == (0, 0)
    for A, Rr in ((0, 0), (3, 5), (40, 400), (256, 2048)):
        w = audio.limiter_window(A, Rr)
        assert w.dtype == np.float64 and w.shape == (A + Rr + 1,) and (w > 0).all()
        acc = 0.0
        for v in w:
            acc = acc + v
        assert abs(acc - 1.0) <= 1e-13
        assert np.allclose(w, w[::-1], rtol=0, atol=1e-15)
    assert audio.limiter_window(0, 0).tolist() == [1.0]
    for bad in ((-1, 0), (0, -1), (257, 0), (0, 2049)):
        with pytest.raises(ValueError):
            audio.limiter_window(*bad)
    for bad in (dict(sr=0), dict(sr=16000, lookahead_ms=-1), dict(sr=16000, release_ms=math.nan), dict(sr=16000, lookahead_ms=17),
                dict(sr=96000, release_ms=25.0), dict(sr=16000, lookahead_ms=True)):
        with pytest.raises(ValueError):
            audio.limiter_reach(**bad)
    assert audio.check_limiter(None) == (40, 400) and audio.check_limiter("sample", 0.5, 1.0, 10.0, 16000) == (16, 160)
    for bad in (("peak",), (True,), ("true", 0.0), ("true", math.inf), ("true", 0.9, -1.0)):
        with pytest.raises(ValueError):
            audio.check_limiter(*bad)


def test_the_taps_interpolate():
    """phase k of resample_taps(4, 1) reads a slow sine at i + k / 4"""
    h, P = R.taps(), R.PHASES
    assert h.size == 2 * R.HALO * P + 1
    i = np.arange(400)
    x = np.sin(2 * np.pi * 0.01 * i).astype(np.float32)
    for k in range(1, P):
        u = np.zeros(x.size)
        xp = np.concatenate([np.zeros(R.HALO), x.astype(np.float64), np.zeros(R.HALO)])
        for d in range(-R.HALO, R.HALO):
            u = u + h[P * d + k + (h.size - 1) // 2] * xp[R.HALO - d: R.HALO - d + x.size]
        assert np.max(np.abs(u[20:-20] - np.sin(2 * np.pi * 0.01 * (i[20:-20] + k / P)))) < 2e-3


def test_s_never_above_r_and_the_ceiling_holds_exactly():
    for c in R.reference():
        w = c["want"]
        assert (w["s"] <= w["r"]).all() and (w["s"] >= 0).all() and (w["m"] <= w["r"]).all(), c["name"]
        assert (np.abs(w["out"].astype(np.float64)) <= c["ceiling"]).all(), c["name"]
        assert w["out"].dtype == np.float32 and w["out"].size == c["x"].size
        # the stats are what they say
        assert w["stats"][1] == c["g"] and w["stats"][3] == np.count_nonzero(w["s"] < 1)
        if c["x"].size:
            assert w["stats"][0] == (c["g"] * w["e"]).max() and w["stats"][2] == w["s"].min()
        else:
            assert w["stats"].tolist() == [0.0, c["g"], 1.0, 0.0]


def test_gain_rows_bits_away_from_the_overs():
    """out is fl32(fl64(x) g) wherever no over lies within A + R samples on either side; s is exactly 1 there"""
    far = near = 0
    for c in R.reference():
        w, W = c["want"], c["A"] + c["R"]
        over = np.flatnonzero(w["r"] < 1)
        i = np.arange(c["x"].size)
        clear = np.ones(i.size, dtype=bool)
        for j in over:
            clear &= np.abs(i - j) > W
        plain = R.gain_only(c["x"], c["g"])
        assert (w["s"][clear] == 1.0).all(), c["name"]
        assert np.array_equal(_bits(w["out"][clear]), _bits(plain[clear])), c["name"]
        far += int(clear.sum())
        near += int((w["s"] < 1).sum())
    assert far > 10000 and near > 10000


def test_a_row_without_an_over_is_gain_rows():
    seen = 0
    for c in R.reference():
        w = c["want"]
        if c["x"].size and (w["r"] == 1).all():
            assert (w["s"] == 1.0).all() and w["stats"][2] == 1.0 and w["stats"][3] == 0.0
            assert np.array_equal(_bits(w["out"]), _bits(R.gain_only(c["x"], c["g"]))), c["name"]
            seen += c["g"] != 1.0
    assert seen >= 1
    ref = {c["name"]: c for c in R.reference()}
    # the inter-sample over: samples under the ceiling, the true peak over it
    q = ref["quarter_true"]
    assert np.abs(q["x"]).max() < q["ceiling"] < q["want"]["stats"][0] and q["want"]["stats"][3] > 500
    assert (ref["quarter_sample"]["want"]["s"] == 1.0).all()
    assert np.array_equal(_bits(ref["quarter_sample"]["want"]["out"]), _bits(q["x"]))


def test_nothing_outside_the_span_matters():
    """the span inside a longer row of garbage is limited as the span alone: the reference takes the span and nothing else, and
    a span cut from a longer signal differs from that signal's limiter only within reach of the cut"""
    ref = {c["name"]: c for c in R.reference()}
    c = ref["two_close"]
    cut = dict(c, x=c["x"][500:1700])
    got = R.run(cut)
    whole = c["want"]
    W = c["A"] + c["R"]
    inner = slice(W + R.HALO, 1200 - W - R.HALO)
    assert np.array_equal(_bits(got["s"][inner]), _bits(whole["s"][500:1700][inner]))
    assert got["s"].size == 1200


def test_true_peak_of_the_output_is_remeasured():
    """The limiter bounds the samples exactly and the true peak going IN; the true peak of what comes out is held only as far
    as a gain that moves between samples allows, so it is measured, per reach: with a smoothing window of 2.5 + 25 ms or more it
    stays within float32 rounding of the ceiling; with none at all (A = R = 0 is a per-sample clipper) it does not."""
    worst = {}
    for c in R.reference():
        if c["mode"] != "true" or not c["x"].size:
            continue
        tp = R.true_peak(c["want"]["out"])
        over = tp / c["ceiling"] - 1.0
        print(f"{c['name']}: true peak in {c['want']['stats'][0]:.4f}, out {tp:.6f}, over the ceiling by {over:+.3e}")
        key = (c["A"], c["R"])
        if over > worst.get(key, (0.0, None))[0]:
            worst[key] = (over, c["name"])
    assert set(worst) == set(OVERSHOOT)
    for key in sorted(worst):
        print(f"(A, R) = {key}: largest overshoot {worst[key][0]:.4e} ({worst[key][1]}); recorded {OVERSHOOT[key]:.4e}")
    for key in sorted(worst):
        assert worst[key][0] <= 2 * OVERSHOOT[key], key
        assert worst[key][0] >= OVERSHOOT[key] / 2, key      # the recorded figure is the measured one


VARIANTS = {
    "no oversampling": dict(_h=None),
    "phase 1 dropped": dict(use=(2, 3)),
    "phase 2 dropped": dict(use=(1, 3)),
    "phase 3 dropped": dict(use=(1, 2)),
    "min window short by one behind": dict(min_lo=1),
    "min window short by one ahead": dict(min_hi=1),
    "smoothing support shifted by one": dict(shift=1),
    "smoothing on m": dict(on_m=True),
    "no final min with r": dict(final_min=False),
    "no float32 clamp": dict(clamp=False),
    "g applied after s": dict(gain_last=True),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_the_cases_tell_wrong_variants_apart(name):
    """Every wrong variant changes a bit of what the call returns -- the float32 row or the four float64 stats -- in at least one
    case.  "smoothing on m" and "no final min with r" differ from the definition by float64 roundings of s, which the float32
    rounding of the row hides but the stat min s (float64, exact) shows."""
    kw = dict(VARIANTS[name])
    changed = []
    for c in R.reference():
        if "_h" in kw and c["mode"] != "true":
            continue
        if ("min_lo" in kw and c["R"] == 0) or ("min_hi" in kw and c["A"] == 0):
            continue
        if "_h" in kw:
            got = R.limit(c["x"], c["g"], c["ceiling"], None, c["A"], c["R"], audio.limiter_window(c["A"], c["R"]))
        else:
            got = R.run(c, **kw)
        row = not np.array_equal(_bits(got["out"]), _bits(c["want"]["out"]))
        if row or not np.array_equal(_bits(got["stats"]), _bits(c["want"]["stats"])):
            changed.append(c["name"] + (" (row)" if row else " (stats)"))
    print(f"{name}: changes {len(changed)} cases: {changed[:8]}")
    assert changed
    if name not in ("smoothing on m", "no final min with r"):
        assert any(n.endswith("(row)") for n in changed)


def test_cases_cover_the_lengths_and_placements():
    ref = {c["name"]: c for c in R.reference()}
    for L in (0, 1, 2, R.HALO, R.A0, R.A0 + R.R0, R.TILE - 1, R.TILE, R.TILE + 1, 3 * R.TILE + R.A0 + R.R0 + 1):
        assert ref[f"len{L}"]["x"].size == L
    assert {(c["A"], c["R"]) for c in ref.values()} == {(0, 0), (3, 5), (40, 400), (256, 2048)}
    assert {c["mode"] for c in ref.values()} == {"true", "sample"}
    r = ref["first_last"]["want"]["r"]
    assert r[0] < 1 and r[-1] < 1
    r = ref["tile_edge"]["want"]["r"]
    assert r[R.TILE - 1] < 1 and r[R.TILE] < 1
    assert ref["dist_A"]["want"]["r"][1000] < 1 and ref["dist_A"]["want"]["r"][1000 + R.A0] < 1
    assert ref["dist_R"]["want"]["r"][1000 + R.R0] < 1
    assert any(c["want"]["stats"][2] < 0.5 for c in ref.values())   # 1 - (1 - r) is not r there


# ---- the C ABI's host side
def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _f64(v):
    v = [float(a) for a in v]
    return (C.c_double * len(v))(*v)


def test_work_len():
    l = _lib.lib()
    assert l.smi_limit_work_len(-1, 1) == -1 and l.smi_limit_work_len((1 << 24) + 1, 1) == -1
    assert l.smi_limit_work_len(100, 0) == -1 and l.smi_limit_work_len(100, 65) == -1
    a, b, c = l.smi_limit_work_len(0, 1), l.smi_limit_work_len(5000, 1), l.smi_limit_work_len(5000, 3)
    window = 2 * a - l.smi_limit_work_len(0, 2)
    assert window >= 256 + 2048 + 1 and a >= window + 3 and b >= window + 5000 + 3 * 5
    assert c - b == 2 * (b - window)                                    # a window, then equal parts a row
    assert l.smi_limit_work_len(1 << 24, 64) > 64 * (1 << 24)


def test_refusals_name_their_argument_on_the_host():
    """every check comes before the first launch, so the refusals need no device: the pointers are never followed"""
    l = _lib.lib()
    fake = 1 << 20                      # "device" addresses: refused calls read none of them
    n, stride, A, Rr = [900, 1000], 1024, 3, 5
    h, w = R.taps(), audio.limiter_window(A, Rr)
    ok = dict(inp=fake, in_stride=stride, n=n, st=[0, 10], en=[900, 990], B=2, gain=fake + (1 << 22), gain_stride=4, ceiling=0.9, taps=h,
              n_taps=h.size, phases=4, A=A, R=Rr, win=w, work=fake + (1 << 23), work_len=1 << 20, out=fake + (1 << 24), out_stride=stride,
              stats=fake + (1 << 25))

    def refused(word, **kw):
        a = dict(ok, **kw)
        rc = l.smi_limit_rows(C.c_void_p(a["inp"]), a["in_stride"], _i32(a["n"]), _i32(a["st"]), _i32(a["en"]), a["B"], C.c_void_p(a["gain"]),
                              a["gain_stride"], float(a["ceiling"]), None if a["taps"] is None else _f64(a["taps"]), a["n_taps"], a["phases"],
                              a["A"], a["R"], None if a["win"] is None else _f64(a["win"]), C.c_void_p(a["work"]), a["work_len"],
                              C.c_void_p(a["out"]), a["out_stride"], C.c_void_p(a["stats"]), None)
        err = l.smi_last_error().decode()
        assert rc == EINVAL and word in err, (word, rc, err)

    refused("lookahead=-1", A=-1, win=audio.limiter_window(0, Rr))
    refused("lookahead=257", A=257, win=np.full(257 + Rr + 1, 1.0 / (257 + Rr + 1)))
    refused("release=2049", R=2049, win=np.full(A + 2049 + 1, 1.0 / (A + 2049 + 1)))
    refused("release=-2", R=-2)
    refused("win sums", win=w * (1 + 1e-9))
    refused("win sums", win=w * 0.5)
    neg = w.copy()
    neg[2], neg[3] = -neg[2], neg[3] + 2 * neg[2]
    refused("win[2]", win=neg)
    nan = w.copy()
    nan[1] = math.nan
    refused("win[1]", win=nan)
    refused("n_taps=81", phases=5)
    refused("n_taps=80", n_taps=80)
    refused("n_taps=81", phases=3)
    refused("phases=0", phases=0, n_taps=0)
    refused("phases=9", phases=9, n_taps=0)
    bad = h.copy()
    bad[7] = math.inf
    refused("taps[7]", taps=bad)
    refused("taps_host", taps=None)
    refused("ceiling", ceiling=0.0)
    refused("ceiling", ceiling=-0.5)
    refused("ceiling", ceiling=math.nan)
    refused("B=65", B=65)
    refused("B=0", B=0)
    refused("n[1]", n=[900, -1])
    refused("n[0]", n=[1025, 1000])
    refused("end[0]", en=[901, 990])
    refused("end[1]", st=[0, 991])
    refused("gain_stride", gain_stride=-1)
    refused("work_len", work_len=100)
    refused("out_stride", out_stride=999)
    refused("out_dev", out=fake + 4)                                   # partial overlap: one sample on
    refused("out_dev", out=fake + 4 * stride)                          # row 0 of out on row 1 of in
    refused("out_dev", out=fake, out_stride=stride + 8)                # same start, another stride
    refused("stats_dev", stats=fake + (1 << 22) + 8)
    refused("null", inp=0)
    refused("null", win=None)
    refused("null", stats=0)
