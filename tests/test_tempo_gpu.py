"""smi_tempo_rows through the C ABI against tests/tempo_ref.py: the frame places and the samples bit for bit, a row's results
as its own, nothing outside a span read, and every refusal before any launch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tempo_ref as R
from sparkmi import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _ref(key, p, q, N, D):
    """the reference of one span, computed once and shared (read only)"""
    searched = []
    out, s = R.tempo(SPANS[key], p, q, N, D, searched)
    out.setflags(write=False)
    s.setflags(write=False)
    return out, s, tuple(searched)


def _square(L, period=8, amp=0.25):
    return np.where((np.arange(L) % period) < period // 2, amp, -amp).astype(np.float32)


SPANS = {
    "a200": R.signal(200, 1), "b0": R.signal(0, 2), "b1": R.signal(1, 3), "b63": R.signal(63, 4), "b64": R.signal(64, 5),
    "b1000": R.signal(1000, 6), "c8000": R.signal(8000, 7), "e6000": R.signal(6000, 8),
    "zero": np.zeros(300, dtype=np.float32), "half": np.full(300, 0.5, dtype=np.float32), "square": _square(300),
}


def tempo(x, n, spans, pq, N, D, B=None, out=None, out_stride=None, pos_stride=None, win=None, rc_only=False):
    """one smi_tempo_rows call on host rows x [B][stride]; returns (out, m, pos) as numpy, or (rc, error, out) for rc_only"""
    l = _lib.lib()
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    B = len(n) if B is None else B
    lens = [e - s for s, e in spans] if spans is not None else list(n)
    lay = [R.layout(max(0, L), p, q, N if N % 2 == 0 and N >= 2 else 16) if p >= 1 and q >= 1 else (1, 1) for L, (p, q) in zip(lens, pq)]
    ms = max([1] + [m for m, _ in lay]) if out_stride is None else out_stride
    ks = max([1] + [k for _, k in lay]) if pos_stride is None else pos_stride
    if out is None:
        out = torch.full((max(1, B), ms), SENTINEL, dtype=torch.float32, device=DEV)
    pos = torch.full((max(1, B), ks), -7, dtype=torch.int32, device=DEV)
    wd = torch.from_numpy(R.window(N) if win is None else win).to(DEV)
    got = (C.c_int32 * max(1, B))()
    st = None if spans is None else _i32(s[0] for s in spans)
    en = None if spans is None else _i32(s[1] for s in spans)
    rc = l.smi_tempo_rows(C.c_void_p(xd.data_ptr()), xd.shape[1], _i32(n), st, en, B, _i32(a[0] for a in pq), _i32(a[1] for a in pq), N, D,
                          C.c_void_p(wd.data_ptr()), C.c_void_p(pos.data_ptr()), pos.shape[1], C.c_void_p(out.data_ptr()), out.shape[1],
                          got, None)
    torch.cuda.synchronize()
    if rc_only:
        return rc, l.smi_last_error().decode(), out.cpu().numpy()
    l.check(rc, "smi_tempo_rows")
    return out.cpu().numpy(), list(got)[:B], pos.cpu().numpy()


def _pack(keys, lead=0, trail=0, extra=0, fill=0.0):
    n = [lead + SPANS[k].size + trail for k in keys]
    x = np.full((len(keys), max(n + [1]) + extra), fill, dtype=np.float32)
    for b, k in enumerate(keys):
        x[b, lead: lead + SPANS[k].size] = SPANS[k]
    return x, n, [(lead, lead + SPANS[k].size) for k in keys]


def _check(keys, pq, N, D, got):
    out, m, pos = got
    for b, (k, (p, q)) in enumerate(zip(keys, pq)):
        want, s, _ = _ref(k, p, q, N, D)
        assert m[b] == want.size == R.layout(SPANS[k].size, p, q, N)[0], (k, p, q)
        assert np.array_equal(pos[b, : s.size], s.astype(np.int32)), (k, p, q)
        assert not pos[b, s.size:].any()
        assert np.array_equal(_bits(out[b, : want.size]), _bits(want)), (k, p, q)
        assert not _bits(out[b, want.size:]).any(), (k, p, q)       # zeros from M to the stride


def test_a_every_frame_searched():
    x, n, _ = _pack(["a200"])
    assert len(_ref("a200", 3, 2, 16, 3)[2]) >= 12      # (of 16: at this radius a frame behind delta >= 1 keeps its natural place)
    _check(["a200"], [(3, 2)], 16, 3, tempo(x, n, None, [(3, 2)], 16, 3))


def test_b_ragged_rows_spans_and_per_row_tempos():
    keys = ["b0", "b1", "b63", "b64", "b1000"]
    pq = [(2, 3), (3, 2), (5, 4), (1, 1), (2, 1)]
    x, n, spans = _pack(keys, lead=5, trail=3, extra=9, fill=0.75)
    got = tempo(x, n, spans, pq, 64, 8)
    _check(keys, pq, 64, 8, got)
    assert np.array_equal(_bits(got[0][3, :64]), _bits(SPANS["b64"]))      # 1/1: the span itself
    # the longest row at every tempo, whole rows (null spans)
    x, n, _ = _pack(["b1000"] * 5)
    _check(["b1000"] * 5, pq, 64, 8, tempo(x, n, None, pq, 64, 8))


@pytest.mark.parametrize("p,q", [(5, 4), (2, 1), (1, 2)])
def test_c_the_production_frame(p, q):
    x, n, _ = _pack(["c8000"])
    _check(["c8000"], [(p, q)], 512, 240, tempo(x, n, None, [(p, q)], 512, 240))


def test_d_ties():
    keys = ["zero", "half", "square"]
    for pq in ((3, 2), (2, 3)):
        x, n, _ = _pack(keys)
        _check(keys, [pq] * 3, 16, 3, tempo(x, n, None, [pq] * 3, 16, 3))
        _check(keys, [pq] * 3, 64, 8, tempo(x, n, None, [pq] * 3, 64, 8))


def test_e_the_limits():
    # with H = D = 1024 only a tempo beyond 2 or below 1/2 drifts past the radius: the C ABI's range is 1/4 .. 4
    x, n, _ = _pack(["e6000"] * 2)
    pq = [(4, 1), (2, 5)]
    for p, q in pq:
        assert _ref("e6000", p, q, 2048, 1024)[2], (p, q)      # frames were searched
    _check(["e6000"] * 2, pq, 2048, 1024, tempo(x, n, None, pq, 2048, 1024))


def test_f_a_row_is_its_own_and_nothing_outside_its_span_is_read():
    key, pq, N, D = "b1000", (3, 2), 64, 8
    x, n, _ = _pack([key])
    alone = tempo(x, n, None, [pq], N, D)
    _check([key], [pq], N, D, alone)
    L = SPANS[key].size
    lead, stride = 41, L + 41 + 77
    big = np.full((64, stride), np.nan, dtype=np.float32)
    big[37, lead: lead + L] = SPANS[key]
    spans = [(3, 3 + (b % 7)) for b in range(64)]
    spans[37] = (lead, lead + L)
    ns = [stride - (b % 5) for b in range(64)]
    pqs = [((5, 4), (2, 3), (1, 1), (2, 1))[b % 4] for b in range(64)]
    pqs[37] = pq
    out, m, pos = tempo(big, ns, spans, pqs, N, D, out_stride=alone[0].shape[1] + 333, pos_stride=alone[2].shape[1] + 5)
    M, K = alone[1][0], alone[2].shape[1]
    assert m[37] == M
    assert np.array_equal(_bits(out[37, :M]), _bits(alone[0][0, :M])) and not _bits(out[37, M:]).any()
    assert np.array_equal(pos[37, :K], alone[2][0]) and not pos[37, K:].any()
    assert not np.isnan(out[37]).any()


def test_g_refusals_name_their_argument_and_launch_nothing():
    x, n, spans = _pack(["b1000", "b64"], lead=2, trail=2)
    xd = torch.from_numpy(x).to(DEV)
    ok = dict(n=n, spans=spans, pq=[(5, 4), (4, 5)], N=64, D=8)

    def refused(word, **kw):
        a = dict(ok, **kw)
        rc, err, out = tempo(xd, a["n"], a["spans"], a["pq"], a["N"], a["D"], B=a.get("B"), out_stride=a.get("out_stride"),
                             pos_stride=a.get("pos_stride"), win=a.get("win"), rc_only=True)
        assert rc == EINVAL and word in err, (word, rc, err)
        assert (out == SENTINEL).all(), word      # nothing was launched

    refused("N=63", N=63, win=R.window(64))
    refused("N=14", N=14, win=R.window(16))
    refused("N=2050", N=2050, win=R.window(2048))
    refused("D=1025", D=1025)
    refused("D=-1", D=-1)
    refused("p[1]/q[1]", pq=[(5, 4), (9, 2)])
    refused("p[0]/q[0]", pq=[(2, 9), (4, 5)])
    refused("p[0]", pq=[(0, 4), (4, 5)])
    refused("q[1]", pq=[(5, 4), (4, 32768)])
    refused("end[1]", spans=[spans[0], (0, n[1] + 1)])
    refused("end[0]", spans=[(spans[0][1], spans[0][0]), spans[1]])
    refused("n[0]", n=[-1, n[1]])
    refused("B=0", B=0)
    refused("B=65", B=65)
    refused("out_stride", out_stride=100)
    refused("pos_stride", pos_stride=2)
    # an output that overlaps the input
    flat = torch.zeros(4 * x.shape[1], dtype=torch.float32, device=DEV)
    src = flat[: 2 * x.shape[1]].view(2, -1)
    src.copy_(xd)
    for off in (0, 1, 2 * x.shape[1] - 1):
        rc, err, _ = tempo(src, n, spans, ok["pq"], 64, 8, out=flat[off: off + 2 * x.shape[1]].view(2, -1), rc_only=True)
        assert rc == EINVAL and "out_dev" in err, (off, err)
    assert np.array_equal(src.cpu().numpy(), x)
    # the next valid call works
    _check(["b1000", "b64"], ok["pq"], 64, 8, tempo(xd, n, spans, ok["pq"], 64, 8))


def test_device_audio_gives_the_raw_calls_results():
    from sparkmi.audio import DeviceAudio, tempo_window
    keys = ["b1000", "b63", "a200"]
    x, n, spans = _pack(keys, lead=4, trail=4)
    xd = torch.from_numpy(x).to(DEV)
    da = DeviceAudio(DEV)
    y, m, pos = da.tempo_rows(xd, n, [1.5, 0.8, (2, 3)], spans=spans, frame=(64, 8))
    pq = [(3, 2), (4, 5), (2, 3)]
    _check(keys, pq, 64, 8, (y.cpu().numpy(), m, pos.cpu().numpy()))
    # the defaults: the rate gives the frame and the radius; whole rows
    x, n, _ = _pack(["c8000"])
    y, m, pos = da.tempo_rows(torch.from_numpy(x).to(DEV), n, [1.25])
    _check(["c8000"], [(5, 4)], 512, 240, (y.cpu().numpy(), m, pos.cpu().numpy()))
    assert np.array_equal(tempo_window(512), R.window(512))
