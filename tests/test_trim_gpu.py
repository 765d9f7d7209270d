"""smi_trim_rows and smi_concat_rows through the C ABI against tests/trim_ref.py: bounds exactly, assembled samples bit for bit.
tests/test_longform_cpu.py checks the inputs themselves (no window near the threshold; both restatements agree)."""
import ctypes as C

import numpy as np
import pytest
import torch

import trim_ref as tr
from sparkmi import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GARBAGE = 7.5e8


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _pack(rows, stride=None, fill=0.0):
    stride = max([len(r) for r in rows] + [1]) if stride is None else stride
    x = np.full((len(rows), stride), fill, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    return x


def trim(rows, W, s, thr, m, stride=None, fill=0.0, n=None, B=None, rc_only=False):
    l = _lib.lib()
    x = torch.from_numpy(_pack(rows, stride, fill)).to(DEV)
    n = [len(r) for r in rows] if n is None else n
    B = len(rows) if B is None else B
    need = l.smi_trim_work_len(max([v for v in n if v >= 0] + [0]), max(W, 1), max(s, 1), max(1, min(B, 64)))
    work = torch.full((max(2, need),), -77, dtype=torch.int32, device=DEV)
    bounds = torch.full((max(1, B), 2), -5, dtype=torch.int32, device=DEV)
    rc = l.smi_trim_rows(C.c_void_p(x.data_ptr()), x.shape[1], _i32(n), B, W, s, float(thr), m, C.c_void_p(work.data_ptr()), work.numel(),
                         C.c_void_p(bounds.data_ptr()), None)
    if rc_only:
        return rc, l.smi_last_error().decode()
    l.check(rc, "smi_trim_rows")
    return [tuple(b) for b in bounds.cpu().tolist()]


@pytest.mark.parametrize("name", sorted(tr.PARAMS))
def test_bounds_equal_the_reference_formula(name):
    W, s, m, thr = tr.PARAMS[name]
    cases = tr.trim_cases(name)
    rows = [x for _, x in cases]
    want = [tr.bounds(x, W, s, thr, m) for x in rows]
    got = trim(rows, W, s, thr, m)
    for (label, x), g, w in zip(cases, got, want):
        print(f"{name}: {label}: n={len(x)} bounds {g}")
        assert g == w, (name, label, g, w)
    # what lies past n is never read: garbage there, and a longer stride, change nothing
    assert trim(rows, W, s, thr, m, stride=max(len(r) for r in rows) + 333, fill=GARBAGE) == want
    # a row's bounds are its own: alone, among five, and in the reversed call
    pick = [2, 5, len(rows) - 3, 8, 0]
    five = trim([rows[i] for i in pick], W, s, thr, m)
    assert five == [want[i] for i in pick]
    assert trim([rows[i] for i in pick[::-1]], W, s, thr, m) == five[::-1]
    for i in pick:
        assert trim([rows[i]], W, s, thr, m) == [want[i]]


@pytest.mark.parametrize("name", sorted(tr.PARAMS))
def test_a_window_exactly_on_the_threshold_is_speech(name):
    W, s, m, _ = tr.PARAMS[name]
    x, thr, i = tr.equality_case(name)
    want = (max(0, i * s - m), min(len(x), i * s + m))
    assert trim([x, x[::-1].copy()], W, s, thr, m, fill=GARBAGE, stride=len(x) + 5)[0] == want
    assert trim([x], W, s, np.nextafter(thr, 1.0), m) == [(0, 0)]      # one ulp above: silence
    assert trim([x], W, s, 0.0, m) == [(0, len(x))]                    # thr = 0: every window is speech


def concat(rows_np, n, bounds, gaps, fade, cap, rc_only=False, B=None):
    l = _lib.lib()
    x = torch.from_numpy(np.ascontiguousarray(rows_np)).to(DEV)
    B = len(bounds) if B is None else B
    out = torch.full((max(1, cap),), 9.0, dtype=torch.float32, device=DEV)
    offs, total = (C.c_longlong * max(1, B))(), C.c_longlong(-1)
    rc = l.smi_concat_rows(C.c_void_p(x.data_ptr()), x.shape[1], _i32(n), _i32(b[0] for b in bounds), _i32(b[1] for b in bounds), _i32(gaps),
                           B, fade, C.c_void_p(out.data_ptr()), cap, offs, C.byref(total), None)
    if rc_only:
        return rc, l.smi_last_error().decode()
    l.check(rc, "smi_concat_rows")
    return out.cpu().numpy(), list(offs)[:B], total.value


@pytest.mark.parametrize("fade", [0, tr.CONCAT_FADE])
@pytest.mark.parametrize("gap", [0, 5])
def test_concat_bits_equal_the_reference_formula(fade, gap):
    rows, n, bounds = tr.concat_case()
    gaps = [gap] * len(bounds)
    want, offs, total = tr.concat(rows, bounds, gaps, fade)
    for cap in (total, total + 1500):
        got, goff, gtotal = concat(rows, n, bounds, gaps, fade, cap)
        assert gtotal == total and goff == offs
        assert np.array_equal(got[:total].view(np.uint32), want.view(np.uint32))
        assert got.size == cap and not got[total:].any()
    # the two empty pieces dropped their gaps: only the non-empty ones count
    assert total == sum(tr.CONCAT_LENGTHS) + gap * sum(1 for v in tr.CONCAT_LENGTHS if v)
    # a piece's bits are its own: the same pieces in another order and with other neighbours
    order = [8, 3, 0, 6]
    got, goff, gtotal = concat(rows[order], [n[i] for i in order], [bounds[i] for i in order], [gap + 1] * 4, fade, 4000)
    for j, i in enumerate(order):
        a, b = bounds[i]
        assert np.array_equal(got[goff[j]: goff[j] + b - a], tr.faded(rows[i, a:b], fade))
    # all pieces empty: nothing but zeros
    got, _, gtotal = concat(rows[:2], [10, 0], [(3, 3), (0, 0)], [5, 5], fade, 10)
    assert gtotal == 0 and not got.any()


def test_refusals_name_the_argument_and_leave_the_library_working():
    x = [np.ones(100, np.float32)] * 2
    for kw, word in ((dict(B=0), "B=0"), (dict(B=65), "B=65"), (dict(n=[100, -1]), "n[1]=-1"), (dict(n=[101, 3]), "n[0]=101")):
        rc, msg = trim(x, 20, 2, 0.01, 40, rc_only=True, **kw)
        assert rc == -1 and word in msg and "smi_trim_rows" in msg, msg
    for (W, s, m, thr), word in (((0, 2, 40, 0.01), "window=0"), ((20, 0, 40, 0.01), "step=0"), ((20, 2, -1, 0.01), "margin=-1"),
                                 ((20, 2, 40, -0.5), "threshold"), ((20, 2, 40, float("nan")), "threshold"), ((16000, 160, 0, 0.01), "LDS")):
        rc, msg = trim(x, W, s, thr, m, rc_only=True)
        assert rc == -1 and word in msg, msg
    rows = np.ones((2, 100), np.float32)
    ok = dict(n=[100, 50], bounds=[(0, 10), (5, 50)], gaps=[0, 3], fade=4, cap=100)
    for change, word in ((dict(B=0), "B=0"), (dict(B=65), "B=65"), (dict(n=[100, -2]), "n[1]=-2"), (dict(bounds=[(0, 10), (9, 5)]), "end[1]=5 below"),
                         (dict(bounds=[(0, 10), (5, 51)]), "end[1]=51 above"), (dict(bounds=[(-1, 10), (5, 50)]), "start[0]=-1"),
                         (dict(cap=57), "cap=57"), (dict(gaps=[0, -3]), "gap[1]=-3"), (dict(fade=-1), "fade=-1")):
        kw = dict(ok, **change)
        rc, msg = concat(rows, kw["n"], kw["bounds"], kw["gaps"], kw["fade"], kw["cap"], rc_only=True, B=kw.get("B"))
        assert rc == -1 and word in msg and "smi_concat_rows" in msg, msg
    # nothing was launched by any of them, and the next calls work
    got, offs, total = concat(rows, ok["n"], ok["bounds"], ok["gaps"], ok["fade"], 58)
    assert total == 58 and offs == [0, 13] and got[10:13].tolist() == [0, 0, 0] and got[0] == np.float32(0.2)
    assert trim(x, 20, 2, 0.01, 40) == [(0, 100), (0, 100)]


def test_device_audio_surface():
    from sparkmi.audio import DeviceAudio
    W, s, m, thr = tr.PARAMS["small"]
    cases = tr.trim_cases("small")[5:11]
    rows = [x for _, x in cases]
    n = [len(r) for r in rows]
    da = DeviceAudio(DEV)
    x = torch.from_numpy(_pack(rows)).to(DEV)
    bounds = da.trim_rows(x, n, W, s, thr, m)
    assert bounds == [tr.bounds(r, W, s, thr, m) for r in rows]
    gaps = [0] + [7] * (len(rows) - 1)
    want, offs, total = tr.concat(rows, bounds, gaps, 8)
    assert da.concat_layout(bounds, gaps) == (offs, total)
    out, got_total = da.concat_rows(x, bounds, gaps, 8, n=n)
    assert got_total == total == out.numel() and np.array_equal(out.cpu().numpy(), want)
    buf = torch.full((total + 40,), 3.0, dtype=torch.float32, device=DEV)
    out2, _ = da.concat_rows(x, bounds, gaps, 8, out=buf)
    assert out2 is buf and np.array_equal(buf.cpu().numpy()[:total], want) and not buf.cpu().numpy()[total:].any()
    with pytest.raises(_lib.SparkMIError, match="end\\[0\\]"):
        da.concat_rows(x, [(0, n[0] + 1)] + bounds[1:], gaps, 8, n=n)
    with pytest.raises(ValueError):
        da.concat_rows(x, bounds[:-1], gaps, 8)
    assert da.trim_rows(x, n, W, s, thr, m) == bounds
