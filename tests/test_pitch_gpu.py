"""smi_pitch_rows through the C ABI against tests/pitch_ref.py: the frame places and the samples bit for bit, equal as well to the
device's own smi_tempo_rows followed by smi_rs_resample_rows and the cut, within the resampler's float64 bound of the stretched
reference, a row's results as its own, nothing outside a span read, and every refusal before any launch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pitch_ref as R
import resample_ref
import tempo_ref
from sparkmi import _lib
from sparkmi.audio import resample_taps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
FRAMES = ((16, 3), (64, 8), (512, 240))
RATIOS = ((3, 2), (2, 3), (28, 25), (89, 100), (199, 100))      # 199/100: the longest filter of a hundredth ratio
TEMPOS = ((1, 1), (5, 4), (4, 5))


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _square(L, period=8, amp=0.25):
    return np.where((np.arange(L) % period) < period // 2, amp, -amp).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _span(L, seed=0):
    """a span of L samples, computed once and shared (read only): seed -1 silence, -2 a constant, -3 a square wave, else noise + tone"""
    x = {-1: np.zeros(L, np.float32), -2: np.full(L, 0.5, np.float32), -3: _square(L)}.get(seed)
    if x is None:
        x = tempo_ref.signal(L, 100 + seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(L, seed, t, r, N, D):
    y, s = R.pitch(_span(L, seed), t, r, N, D)
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


def _length(n_out, t):
    """the shortest span whose output at tempo t has at least n_out samples (exactly n_out wherever a span has)"""
    L = (n_out * t[0]) // t[1]
    while -((-L * t[1]) // t[0]) < n_out:
        L += 1
    while L and -((-(L - 1) * t[1]) // t[0]) >= n_out:
        L -= 1
    return L


def _pool(rr):
    """(taps [total] fp32, {(up, down): (offset, count)}) for the pitch ratios rr"""
    where, parts, used = {}, [], 0
    for rp, rq in rr:
        g = np.gcd(rp, rq)
        k = (rq // g, rp // g)
        if k != (1, 1) and k not in where:
            h = R.taps32(*k)
            where[k] = (used, h.size)
            parts.append(h)
            used += h.size
    return (np.concatenate(parts) if parts else np.zeros(1, np.float32)), where


def pitch(x, n, spans, tt, rr, N, D, B=None, out=None, out_stride=None, pos_stride=None, taps=None, offs=None, counts=None, taps_len=None,
          rc_only=False):
    """one smi_pitch_rows call on host rows x [B][stride]; returns (out, m, pos) as numpy, or (rc, error, out) for rc_only"""
    l = _lib.lib()
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    B = len(n) if B is None else B
    lens = [e - s for s, e in spans] if spans is not None else list(n)
    plans = []
    for L, t, r in zip(lens, tt, rr):
        try:
            plans.append(R.plan(max(0, L), t, r, N if N % 2 == 0 and N >= 2 else 16))
        except (ZeroDivisionError, ValueError):
            plans.append(dict(n_out=1, K=1))
    ms = max([1] + [p["n_out"] for p in plans]) if out_stride is None else out_stride
    ks = max([1] + [p["K"] for p in plans]) if pos_stride is None else pos_stride
    if out is None:
        out = torch.full((max(1, B), ms), SENTINEL, dtype=torch.float32, device=DEV)
    pos = torch.full((max(1, B), ks), -7, dtype=torch.int32, device=DEV)
    wd = torch.from_numpy(tempo_ref.window(N if N % 2 == 0 and N >= 2 else 16)).to(DEV)
    pool, where = _pool([r for r in rr if r[0] >= 1 and r[1] >= 1]) if taps is None else (taps, {})
    key = lambda r: (r[1] // np.gcd(r[0], r[1]), r[0] // np.gcd(r[0], r[1])) if r[0] >= 1 and r[1] >= 1 else (1, 1)   # noqa: E731
    if offs is None:
        offs = [where.get(key(r), (0, 0))[0] for r in rr]
    if counts is None:
        counts = [where.get(key(r), (0, 0))[1] for r in rr]
    td = pool if isinstance(pool, torch.Tensor) else torch.from_numpy(pool).to(DEV)      # (a device tensor: the caller's own memory)
    got = (C.c_int32 * max(1, B))()
    st = None if spans is None else _i32(s[0] for s in spans)
    en = None if spans is None else _i32(s[1] for s in spans)
    rc = l.smi_pitch_rows(C.c_void_p(xd.data_ptr()), xd.shape[1], _i32(n), st, en, B, _i32(a[0] for a in tt), _i32(a[1] for a in tt),
                          _i32(a[0] for a in rr), _i32(a[1] for a in rr), N, D, C.c_void_p(wd.data_ptr()), C.c_void_p(td.data_ptr()),
                          td.numel() if taps_len is None else taps_len, _i32(offs), _i32(counts), C.c_void_p(pos.data_ptr()), pos.shape[1],
                          C.c_void_p(out.data_ptr()), out.shape[1], got, None)
    torch.cuda.synchronize()
    if rc_only:
        return rc, l.smi_last_error().decode(), out.cpu().numpy()
    l.check(rc, "smi_pitch_rows")
    return out.cpu().numpy(), list(got)[:B], pos.cpu().numpy()


def _pack(rows, lead=0, trail=0, extra=0, fill=0.0):
    """rows: (L, seed); the spans packed into [B][stride] with `lead` / `trail` samples of `fill` around each"""
    n = [lead + L + trail for L, _ in rows]
    x = np.full((len(rows), max(n + [1]) + extra), fill, dtype=np.float32)
    for b, (L, seed) in enumerate(rows):
        x[b, lead: lead + L] = _span(L, seed)
    return x, n, [(lead, lead + L) for L, _ in rows]


def _check(rows, tt, rr, N, D, got):
    out, m, pos = got
    for b, ((L, seed), t, r) in enumerate(zip(rows, tt, rr)):
        want, s = _ref(L, seed, t, r, N, D)
        pl = R.plan(L, t, r, N)
        assert m[b] == want.size == pl["n_out"], (L, t, r)
        assert np.array_equal(pos[b, : s.size], s.astype(np.int32)), (L, t, r)
        assert not pos[b, s.size:].any()
        assert np.array_equal(_bits(out[b, : want.size]), _bits(want)), (L, t, r, N, D)
        assert not _bits(out[b, want.size:]).any(), (L, t, r)       # zeros from n_out to the stride
        if want.size and (pl["up"], pl["down"]) != (1, 1):          # independently: the float64 sum over the stretched reference
            y, absum, terms = resample_ref.direct(R.stretched(_span(L, seed), t, r, N, D), pl["up"], pl["down"], resample_taps(pl["up"], pl["down"]))
            err = np.abs(out[b, : want.size].astype(np.float64) - y[: want.size])
            assert (err <= resample_ref.bound(absum, terms)[: want.size]).all(), (L, t, r)


def _grid(N):
    """(rows, tempos) whose outputs have 0, 1, H - 1, 1023, 1024, 1025 and 2049 samples at every tempo (the next length where
    a tempo gives none of exactly that many)"""
    rows, tt = [], []
    for t in TEMPOS:
        for i, n_out in enumerate((0, 1, N // 2 - 1, 1023, 1024, 1025, 2049)):
            rows.append((_length(n_out, t), i))
            tt.append(t)
    return rows, tt


@pytest.mark.parametrize("N,D", FRAMES)
@pytest.mark.parametrize("r", RATIOS)
def test_a_bits_at_every_edge_length(N, D, r):
    rows, tt = _grid(N)
    assert {R.plan(L, t, r, N)["n_out"] for (L, _), t in zip(rows, tt) if t == (1, 1)} == {0, 1, N // 2 - 1, 1023, 1024, 1025, 2049}
    x, n, spans = _pack(rows, lead=3, trail=2, extra=5, fill=0.75)
    _check(rows, tt, [r] * len(rows), N, D, pitch(x, n, spans, tt, [r] * len(rows), N, D))


def test_b_ragged_rows_per_row_ratios_pitched_and_unpitched():
    rows = [(0, 1), (1, 2), (63, 3), (64, 4), (1000, 5), (2500, 6), (1000, 5), (777, 7)]
    tt = [(2, 3), (3, 2), (5, 4), (1, 1), (2, 1), (1, 1), (5, 4), (4, 5)]
    rr = [(3, 2), (1, 1), (89, 100), (1, 1), (2, 1), (28, 25), (1, 1), (1, 2)]
    x, n, spans = _pack(rows, lead=5, trail=3, extra=9, fill=0.75)
    got = pitch(x, n, spans, tt, rr, 64, 8)
    _check(rows, tt, rr, 64, 8, got)
    assert np.array_equal(_bits(got[0][3, :64]), _bits(_span(64, 4)))      # r = 1 and t = 1: the span itself
    want, s = tempo_ref.tempo(_span(1000, 5), 5, 4, 64, 8)                 # r = 1: smi_tempo_rows' row
    assert np.array_equal(_bits(got[0][6, :800]), _bits(want)) and np.array_equal(got[2][6, : s.size], s.astype(np.int32))
    # whole rows (null spans)
    x, n, _ = _pack(rows)
    _check(rows, tt, rr, 64, 8, pitch(x, n, None, tt, rr, 64, 8))


@pytest.mark.parametrize("N,D", FRAMES)
@pytest.mark.parametrize("r", RATIOS)
def test_c_equal_to_the_two_existing_device_calls_and_the_cut(N, D, r):
    """test_a's rows through smi_tempo_rows at P / Q, smi_rs_resample_rows at up / down and the cut.  The empty spans are left
    out of the two calls (the resampler takes no row of 0 samples): their n_out = 0 is checked alone."""
    from sparkmi.audio import DeviceAudio
    grid, gt = _grid(N)
    assert all(pitch(np.zeros((1, 1), np.float32), [0], None, [t], [r], N, D)[1] == [0] for t in TEMPOS)
    rows = [row for row in grid if row[0]]
    tt = [t for row, t in zip(grid, gt) if row[0]]
    rr = [r] * len(rows)
    x, n, spans = _pack(rows, lead=2, trail=1)
    xd = torch.from_numpy(x).to(DEV)
    out, m, pos = pitch(xd, n, spans, tt, rr, N, D)
    plans = [R.plan(L, t, r, N) for (L, _), t in zip(rows, tt)]
    assert {p["n_out"] for p, t in zip(plans, tt) if t == (1, 1)} == {1, N // 2 - 1, 1023, 1024, 1025, 2049}
    da = DeviceAudio(DEV)
    z, zm, zpos = da.tempo_rows(xd, n, [(p["P"], p["Q"]) for p in plans], spans=spans, frame=(N, D))
    assert zm == [p["M"] for p in plans] and min(zm) >= 1
    y, yn = da.resample_rows(z.contiguous(), zm, [p["up"] for p in plans], [p["down"] for p in plans])
    y, zpos = y.cpu().numpy(), zpos.cpu().numpy()
    for b, p in enumerate(plans):
        assert yn[b] >= p["n_out"] == m[b]
        assert np.array_equal(_bits(out[b, : m[b]]), _bits(y[b, : m[b]])), (rows[b], tt[b], rr[b])
        assert np.array_equal(pos[b, : p["K"]], zpos[b, : p["K"]])


def test_d_ties():
    rows = [(300, -1), (300, -2), (300, -3)]
    for t, r in (((1, 1), (3, 2)), ((5, 4), (89, 100)), ((4, 5), (2, 3))):
        for N, D in ((16, 3), (64, 8)):
            x, n, _ = _pack(rows)
            _check(rows, [t] * 3, [r] * 3, N, D, pitch(x, n, None, [t] * 3, [r] * 3, N, D))


def test_e_a_row_is_its_own_and_nothing_outside_its_span_is_read():
    row, t, r, N, D = (1500, 11), (5, 4), (28, 25), 64, 8
    x, n, _ = _pack([row])
    alone = pitch(x, n, None, [t], [r], N, D)
    _check([row], [t], [r], N, D, alone)
    L = row[0]
    lead, stride = 41, L + 41 + 77
    big = np.full((64, stride), np.nan, dtype=np.float32)
    big[37, lead: lead + L] = _span(*row)
    spans = [(3, 3 + (b % 7)) for b in range(64)]
    spans[37] = (lead, lead + L)
    ns = [stride - (b % 5) for b in range(64)]
    tts = [((5, 4), (2, 3), (1, 1), (2, 1))[b % 4] for b in range(64)]
    rrs = [((1, 1), (3, 2), (89, 100), (1, 2), (199, 100))[b % 5] for b in range(64)]
    tts[37], rrs[37] = t, r
    out, m, pos = pitch(big, ns, spans, tts, rrs, N, D, out_stride=alone[0].shape[1] + 333, pos_stride=alone[2].shape[1] + 5)
    M, K = alone[1][0], alone[2].shape[1]
    assert m[37] == M == 1200
    assert np.array_equal(_bits(out[37, :M]), _bits(alone[0][0, :M])) and not _bits(out[37, M:]).any()
    assert np.array_equal(pos[37, :K], alone[2][0]) and not pos[37, K:].any()
    assert not np.isnan(out[37]).any()


def test_f_refusals_name_their_argument_and_launch_nothing():
    rows = [(1000, 5), (64, 4)]
    x, n, spans = _pack(rows, lead=2, trail=2)
    xd = torch.from_numpy(x).to(DEV)
    ok = dict(n=n, spans=spans, tt=[(5, 4), (1, 1)], rr=[(3, 2), (1, 1)], N=64, D=8)

    def refused(word, **kw):
        a = dict(ok, **kw)
        rc, err, out = pitch(xd, a["n"], a["spans"], a["tt"], a["rr"], a["N"], a["D"], B=a.get("B"), out_stride=a.get("out_stride"),
                             pos_stride=a.get("pos_stride"), taps=a.get("taps"), offs=a.get("offs"), counts=a.get("counts"),
                             taps_len=a.get("taps_len"), rc_only=True)
        assert rc == EINVAL and word in err, (word, rc, err)
        assert (out == SENTINEL).all(), word      # nothing was launched

    refused("N=63", N=63)
    refused("N=2050", N=2050)
    refused("D=1025", D=1025)
    refused("rp[0]", rr=[(0, 2), (1, 1)])
    refused("rq[1]", rr=[(3, 2), (1, 0)])
    refused("tp[0]", tt=[(0, 4), (1, 1)])
    refused("tq[1]", tt=[(5, 4), (1, -1)])
    refused("row 0 has no layout", rr=[(9, 1), (1, 1)])                      # a stretch of 5/36
    refused("row 1 has no layout", tt=[(5, 4), (4, 1)], rr=[(3, 2), (1, 2)])  # a stretch of 8
    refused("n_taps[0]=0", counts=[0, 0])                                    # a pitched row without taps
    refused("n_taps[0]=30", counts=[30, 0])                                  # an even count
    refused("n_taps[0]=1", counts=[1, 0])                                    # one tap is H = 0: no filter
    refused("n_taps[0]=1", rr=[(1, 2), (1, 1)], counts=[1, 0])               # (r < 1: M < n_out, frames past K would be read)
    refused("n_taps[1]=61", counts=[61, 61])                                 # taps for a row at 1/1
    refused("tap_off[0]=1", offs=[1, 0])                                     # the taps leave the pool
    refused("tap_off[0]=-1", offs=[-1, 0])
    refused("taps_len=60", taps_len=60)                                      # a pool shorter than the row's taps
    refused("floats of LDS", taps=np.zeros(20000, np.float32), counts=[16001, 0])
    refused("floats of LDS", rr=[(1999, 1000), (1, 1)], taps=np.zeros(40000, np.float32), counts=[39981, 0], offs=[0, 0])
    refused("end[1]", spans=[spans[0], (0, n[1] + 1)])
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
        rc, err, _ = pitch(src, n, spans, ok["tt"], ok["rr"], 64, 8, out=flat[off: off + 2 * x.shape[1]].view(2, -1), rc_only=True)
        assert rc == EINVAL and "out_dev" in err, (off, err)
    assert np.array_equal(src.cpu().numpy(), x)
    # an output that overlaps the taps: one buffer holds the rows' output and, from its last float on, the 61 taps of row 0
    size = 2 * 800
    h = torch.from_numpy(R.taps32(2, 3)).to(DEV)
    for first in (size - 1, 0, size - 61):
        both = torch.full((size + 61,), SENTINEL, dtype=torch.float32, device=DEV)
        both[first: first + 61] = h
        before = both.cpu().numpy()
        rc, err, _ = pitch(xd, n, spans, ok["tt"], ok["rr"], 64, 8, out=both[:size].view(2, -1), taps=both[first: first + 61], offs=[0, 0],
                           counts=[61, 0], rc_only=True)
        assert rc == EINVAL and "out_dev overlaps taps_dev" in err, (first, rc, err)
        assert np.array_equal(_bits(both.cpu().numpy()), _bits(before)), first      # nothing was launched
    # the taps right behind the output do not overlap it: the same call is taken
    both = torch.full((size + 61,), SENTINEL, dtype=torch.float32, device=DEV)
    both[size:] = h
    got = pitch(xd, n, spans, ok["tt"], ok["rr"], 64, 8, out=both[:size].view(2, -1), taps=both[size:], offs=[0, 0], counts=[61, 0])
    _check(rows, ok["tt"], ok["rr"], 64, 8, got)
    # the next valid call works
    _check(rows, ok["tt"], ok["rr"], 64, 8, pitch(xd, n, spans, ok["tt"], ok["rr"], 64, 8))


def test_g_device_audio_gives_the_raw_calls_results():
    from sparkmi.audio import PITCH_TAP_CACHE, DeviceAudio, pitch_ratio
    rows = [(1000, 5), (63, 3), (777, 7), (1000, 5)]
    x, n, spans = _pack(rows, lead=4, trail=4)
    xd = torch.from_numpy(x).to(DEV)
    da = DeviceAudio(DEV)
    y, m, pos = da.pitch_rows(xd, n, [1.25, None, (4, 5), 0.8], [7, -2, None, (28, 25)], spans=spans, frame=(64, 8))
    tt, rr = [(5, 4), (1, 1), (4, 5), (4, 5)], [(3, 2), (89, 100), (1, 1), (28, 25)]
    _check(rows, tt, rr, 64, 8, (y.cpu().numpy(), m, pos.cpu().numpy()))
    assert da.registered == set()      # the taps are the object's own cache, not the resampler handle's registrations
    # the defaults: the rate gives the frame and the radius; whole rows; semitones
    x, n, _ = _pack([(2049, 6)])
    y, m, pos = da.pitch_rows(torch.from_numpy(x).to(DEV), n, [None], [2.0])
    assert pitch_ratio(2.0) == (28, 25)
    _check([(2049, 6)], [(1, 1)], [(28, 25)], 512, 240, (y.cpu().numpy(), m, pos.cpu().numpy()))
    # more ratios than the cache holds: the slots unused the longest are taken over in the one pool, the results stay
    small = torch.from_numpy(_pack([(300, 6)])[0]).to(DEV)
    pool = da._pitch_cache["pool"]
    for c in range(101, 101 + PITCH_TAP_CACHE + 2):
        da.pitch_rows(small, [300], [None], [(c, 100)], frame=(16, 3))
    assert len(da._pitch_cache["where"]) == PITCH_TAP_CACHE and da._pitch_cache["pool"] is pool
    # +7 and -2 semitones (2/3, 100/89), unused the longest, were evicted; 25/28 was used again by 112/100 and stayed
    assert (2, 3) not in da._pitch_cache["where"] and (100, 89) not in da._pitch_cache["where"] and (25, 28) in da._pitch_cache["where"]
    y, m, pos = da.pitch_rows(small, [300], [None], [7], frame=(16, 3))      # an evicted ratio comes back: its taps are copied again
    _check([(300, 6)], [(1, 1)], [(3, 2)], 16, 3, (y.cpu().numpy(), m, pos.cpu().numpy()))
    assert (2, 3) in da._pitch_cache["where"] and len(da._pitch_cache["where"]) == PITCH_TAP_CACHE and da._pitch_cache["pool"] is pool
    y, m, pos = da.pitch_rows(small, [300], [0.8], [(133, 100)], frame=(16, 3))      # a ratio that stayed
    _check([(300, 6)], [(4, 5)], [(133, 100)], 16, 3, (y.cpu().numpy(), m, pos.cpu().numpy()))
    y, m, pos = da.pitch_rows(torch.from_numpy(x).to(DEV), n, [None], [2.0])
    _check([(2049, 6)], [(1, 1)], [(28, 25)], 512, 240, (y.cpu().numpy(), m, pos.cpu().numpy()))
    with pytest.raises(ValueError, match="taps"):
        da.pitch_rows(small, [300], [None], [(1999, 1000)], frame=(16, 3))
