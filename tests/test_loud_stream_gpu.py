"""smi_louds_* through the C ABI (and audio.StreamLoudness) against tests/loud_stream_ref.py of the WHOLE stream: knot gains within
the tolerance of the longdouble reference, flags equal, the final loudness bit-equal to smi_loud_rows of the whole stream, the
samples bit-equal to the header's sample formula on the device's own knot gains -- and everything bit for bit against the
one-push run, whatever the pushes, the slot, the row and the other rows; every refusal before anything changes."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import loud_stream_ref as S
from sparkmi import _lib, audio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
NAMES = [c["name"] for c in S.cases()]
PRIMES = [7, 13, 31, 61, 127, 251, 509, 1021]


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Handle:
    """one smi_louds handle and the host's own count of every stream"""

    def __init__(self, max_streams, max_chunk, block, coef, max_blocks=4096):
        self.l, self.block = _lib.lib(), block
        self.h = C.c_void_p()
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        self.l.check(self.l.smi_louds_create(max_streams, max_chunk, block, coef.ctypes.data_as(C.POINTER(C.c_double)), max_blocks,
                                             C.byref(self.h)), "smi_louds_create")
        self.n = {}

    def close(self):
        self.l.smi_louds_destroy(self.h)

    def open(self, slot, c):
        self.l.check(self.l.smi_louds_open(self.h, slot, c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"]), "smi_louds_open")
        self.n[slot] = 0

    def raw(self, x, slots, lens, lasts, B, out, gain=None, stats=None):
        got = (C.c_int32 * max(1, len(slots)))(*([-9] * max(1, len(slots))))
        rc = self.l.smi_louds_push_rows(self.h, C.c_void_p(x.data_ptr()), x.shape[1], _i32(slots), _i32(lens), _i32(lasts), B,
                                        None if gain is None else C.c_void_p(gain.data_ptr()), 0 if gain is None else gain.shape[1],
                                        C.c_void_p(out.data_ptr()), out.shape[1], got,
                                        None if stats is None else C.c_void_p(stats.data_ptr()), None)
        return rc, self.l.smi_last_error().decode(), list(got)

    def push(self, rows, pad=3, extra=0):
        """rows [(slot, chunk, last)]: one call; NaN fills the input past every chunk's length.  Returns per row (piece row,
        piece length, gain row, knots, stats row) as device tensors, after checking the lengths."""
        B = len(rows)
        want, nk = [], []
        for slot, c, last in rows:
            k0 = max(0, self.n[slot] // (self.block // 4) - 3)
            piece, self.n[slot], k1 = S.piece_len(self.block, self.n[slot], len(c), last)
            want.append(piece)
            nk.append(k1 - k0)
        x = np.full((B, max([1] + [len(c) for _, c, _ in rows]) + extra), np.nan, dtype=np.float32)
        for b, (_, c, _) in enumerate(rows):
            x[b, : len(c)] = c
        xd = torch.from_numpy(x).to(DEV)
        out = torch.full((B, max([1] + want) + pad), SENTINEL, dtype=torch.float32, device=DEV)
        gain = torch.full((B, 2 * max([1] + nk) + pad), -7.0, dtype=torch.float64, device=DEV)
        stats = torch.full((B, 4), -7.0, dtype=torch.float64, device=DEV)
        rc, err, got = self.raw(xd, [r[0] for r in rows], [len(r[1]) for r in rows], [r[2] for r in rows], B, out, gain, stats)
        assert rc == 0, err
        assert got[:B] == want
        return [(out[b], want[b], gain[b], nk[b], stats[b]) for b in range(B)]


def _gather(parts):
    """parts of one stream in order -> (samples, G, flags, the last push's stats); the fill behind every piece and behind every
    push's knots must be zeros"""
    ys, gs, fs = [], [], []
    for o, m, g, k, _ in parts:
        o, g = o.cpu().numpy(), g.cpu().numpy()
        assert not o[m:].any() and not g[2 * k:].any()
        ys.append(o[:m])
        gs.append(g[0: 2 * k: 2])
        fs.append(g[1: 2 * k: 2])
    return np.concatenate(ys), np.concatenate(gs), np.concatenate(fs).astype(np.int64), parts[-1][4].cpu().numpy()


def _cuts(style, L):
    if style == "ones":
        return [1] * L
    if style in ("127", "128", "129"):
        step = [int(style)]
    else:
        step = PRIMES
    out, i = [], 0
    while sum(out) < L:
        out.append(min(step[i % len(step)], L - sum(out)))
        i += 1
        if style == "primes" and i % 3 == 0:
            out.append(0)                       # empty pushes among them
    return out + ([0] if style == "primes" else [])   # and an empty last push


def _stream(c, cuts, slot=0, max_streams=2, handle=None):
    """one stream pushed alone in pieces of ``cuts`` (they sum to its length; the last one carries last = 1)"""
    h = handle or Handle(max_streams, max([1] + cuts), c["block"], c["coef"])
    h.open(slot, c)
    parts, at = [], 0
    cuts = cuts or [0]
    for i, m in enumerate(cuts):
        parts += h.push([(slot, c["x"][at: at + m], i == len(cuts) - 1)])
        at += m
    assert at == len(c["x"])
    got = _gather(parts)
    if handle is None:
        h.close()
    return got


@functools.lru_cache(maxsize=None)
def _one_push(name):
    """the stream pushed at once with last = 1, run once and shared (read only)"""
    c = S.case(name)
    got = _stream(c, [len(c["x"])])
    for a in got:
        a.setflags(write=False)
    return got


@functools.lru_cache(maxsize=None)
def _batch_loudness(name):
    c = S.case(name)
    x = c["x"]
    da = audio.DeviceAudio(DEV)
    xd = torch.zeros((1, max(1, len(x))), dtype=torch.float32, device=DEV)
    xd[0, : len(x)] = torch.from_numpy(np.array(x))
    st = da.loudness_rows(xd, [len(x)], coef=c["coef"], block=c["block"]).cpu().numpy()
    da.close()
    return st[0]


@pytest.mark.parametrize("name", NAMES)
def test_one_push_against_the_reference(name):
    c = S.case(name)
    y, G, F, st = _one_push(name)
    r = c["ref"]
    hop = c["block"] // 4
    L = len(c["x"])
    assert len(G) == len(r["G"]) == ((L - 1) // hop + 2 if L else 0) and len(y) == L
    worst = max([abs(float(np.longdouble(a) / b - 1)) for a, b in zip(G, r["G"])] + [0.0])
    print(f"{name}: {len(G)} knots, largest gain difference {worst:.3e} relative (tolerance {S.TOL_GAIN:.1e})")
    assert worst <= S.TOL_GAIN
    assert F.tolist() == r["flags"]
    # the final loudness and the peak: smi_loud_rows of the whole stream, bit for bit
    want = _batch_loudness(name)
    assert _bits64(st[0]) == _bits64(want[0]) and _bits64(st[1]) == _bits64(want[1])
    if math.isfinite(float(r["loudness"])):
        assert abs(float(st[0] - r["loudness"])) <= S.TOL_LU
    else:
        assert st[0] == -math.inf
    if L:
        assert _bits64(st[2]) == _bits64(G[-1]) and int(st[3]) == int(np.bitwise_or.reduce(F))
    # the samples: the header's formula on the device's own knot gains, bit for bit
    assert np.array_equal(_bits(y), _bits(S.apply(c["x"], G, hop)))
    if c["target"] == c["target"]:
        assert float(np.abs(y).max(initial=0.0)) <= c["ceiling"] * (1 + 2.0 ** -23)
    else:
        assert np.array_equal(_bits(y), _bits(c["x"]))


def _same(a, b):
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    assert np.array_equal(_bits64(a[1]), _bits64(b[1])) and np.array_equal(a[2], b[2])
    assert np.array_equal(_bits64(a[3]), _bits64(b[3]))


@pytest.mark.parametrize("name", [n for n in NAMES if len(S.case(n)["x"]) <= 499 and not n.endswith("len0")])
def test_pushes_of_one_sample(name):
    c = S.case(name)
    _same(_stream(c, _cuts("ones", len(c["x"]))), _one_push(name))


@pytest.mark.parametrize("style", ["127", "128", "129", "primes"])
@pytest.mark.parametrize("name", NAMES)
def test_any_pushes_give_the_one_push_run(name, style):
    c = S.case(name)
    _same(_stream(c, _cuts(style, len(c["x"]))), _one_push(name))


def test_a_row_among_64_in_another_slot_with_other_strides():
    c = S.case("b64_talk")
    others = [S.case(n) for n in ("b64_click", "b64_max_gain", "b64_measure_only", "b64_under_gate")]
    h = Handle(80, 700, 64, c["coef"])
    slots = list(range(79, 15, -1))             # 64 slots, the stream under test in slot 42 as row 37
    for b, s in enumerate(slots):
        h.open(s, c if b == 37 else others[b % 4])
    rng = np.random.default_rng(5)
    L = len(c["x"])
    parts, at = [], 0
    sizes = [233, 0, 512, 129, 700, 61]
    i = 0
    while True:
        m = min(sizes[i % len(sizes)], L - at)
        last = at + m == L
        rows = []
        for b, s in enumerate(slots):
            if b == 37:
                rows.append((s, c["x"][at: at + m], last))
            else:
                o = others[b % 4]["x"]
                k = int(rng.integers(0, 700))
                rows.append((s, o[(i * 97 + b) % 500:][:k], False))
        parts.append(h.push(rows, pad=11, extra=29)[37])
        at += m
        i += 1
        if last:
            break
    h.close()
    _same(_gather(parts), _one_push("b64_talk"))


def test_two_handles_interleaved():
    a, b = S.case("b64_talk"), S.case("b400_talk")
    ha, hb = Handle(2, 600, a["block"], a["coef"]), Handle(3, 2100, b["block"], b["coef"])
    ha.open(1, a)
    hb.open(2, b)
    pa, pb, ia, ib = [], [], 0, 0
    while ia < len(a["x"]) or ib < len(b["x"]):
        if ia < len(a["x"]):
            m = min(600, len(a["x"]) - ia)
            pa += ha.push([(1, a["x"][ia: ia + m], ia + m == len(a["x"]))])
            ia += m
        if ib < len(b["x"]):
            m = min(2100, len(b["x"]) - ib)
            pb += hb.push([(2, b["x"][ib: ib + m], ib + m == len(b["x"]))])
            ib += m
    ha.close()
    hb.close()
    _same(_gather(pa), _one_push("b64_talk"))
    _same(_gather(pb), _one_push("b400_talk"))


def test_every_refusal_leaves_the_stream_untouched():
    c = S.case("b64_talk")
    x, L = c["x"], len(c["x"])
    nblk = L // 16 - 3
    h = Handle(4, 2500, 64, c["coef"], max_blocks=nblk)
    h.open(0, c)
    h.open(1, c)
    parts = h.push([(0, x[:900], False)])
    xd = torch.zeros((2, 1200), dtype=torch.float32, device=DEV)
    out = torch.full((2, 1300), SENTINEL, dtype=torch.float32, device=DEV)
    stats = torch.full((2, 4), -7.0, dtype=torch.float64, device=DEV)

    def refused(slots, lens, lasts, B, o=out, x_=xd, word=""):
        rc, err, got = h.raw(x_, slots, lens, lasts, B, o, None, stats)
        assert rc == EINVAL and word in err, (rc, err)
        assert got[0] == -9                     # nothing was filled in
        assert bool((out == SENTINEL).all()) and bool((stats == -7.0).all())

    refused([0, 0], [10, 10], [0, 0], 2, word="stream too")             # a stream given twice in a call
    refused([0, 3], [10, 10], [0, 0], 2, word="not open")               # a stream that is not open
    refused([0], [2501], [0], 1, word="max_chunk")                      # len > max_chunk
    refused([0, 1], [10, 10], [0, 2], 2, word="last")
    flat = torch.zeros(4000, dtype=torch.float32, device=DEV)
    ov_in, ov_out = flat[:2000].view(2, 1000), flat[1500:3500].view(2, 1000)
    rc, err, got = h.raw(ov_in, [0, 1], [10, 10], [0, 0], 2, ov_out, None, None)
    assert rc == EINVAL and "overlaps" in err and got[0] == -9          # out_dev overlapping in_dev
    # passing max_blocks: a handle that holds exactly the stream's blocks refuses one hop more
    long = np.concatenate([x[900:], np.zeros(16, dtype=np.float32)])
    xl = torch.from_numpy(np.stack([long, long])).to(DEV)
    big = torch.full((2, len(long) + 200), SENTINEL, dtype=torch.float32, device=DEV)
    rc, err, got = h.raw(xl, [0, 1], [len(long), 3], [1, 0], 2, big, None, stats)
    assert rc == EINVAL and "max_blocks" in err and got[0] == -9
    assert bool((big == SENTINEL).all()) and bool((stats == -7.0).all())
    # the streams go on as if nothing had been asked: stream 0 from where it was, stream 1 from its start
    parts += h.push([(0, x[900:1500], False)])
    both = h.push([(0, x[1500:], True), (1, x[:1000], False)])
    parts.append(both[0])
    _same(_gather(parts), _one_push("b64_talk"))
    p1 = [both[1]]
    at = 1000
    while at < L:
        m = min(1000, L - at)
        p1 += h.push([(1, x[at: at + m], at + m == L)])
        at += m
    _same(_gather(p1), _one_push("b64_talk"))
    rc, err, _ = h.raw(xd, [0], [10], [0], 1, out, None, None)          # a stream closes with its last push
    assert rc == EINVAL and "not open" in err
    h.close()


def test_stream_loudness_object():
    """audio.StreamLoudness: keys to slots, an unopened key copies, a slot is free again after the last push"""
    c = S.case("b400_talk")
    x, L = c["x"], len(c["x"])
    sl = audio.StreamLoudness(2, 3000, block=c["block"], coef=c["coef"], max_blocks=600, device=DEV)
    sl.open("a", c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"])
    ya, yb, G, F = [], [], [], []
    at = 0
    stats = None
    while at < L:
        m = min(3000, L - at)
        last = at + m == L
        xd = torch.from_numpy(np.stack([np.pad(x[at: at + m], (0, 3000 - m))] * 2)).to(DEV)
        rows = [("a", m, last), ("b", m, last)]
        want = sl.piece_lengths(rows)
        out, lens, gains, nk, stats = sl.push(xd, rows, return_gains=True)
        assert lens == want and sl.last_stats is stats
        o, g = out.cpu().numpy(), gains.cpu().numpy()
        ya.append(o[0, : lens[0]])
        yb.append(o[1, : lens[1]])
        G.append(g[0, : nk[0], 0])
        F.append(g[0, : nk[0], 1])
        at += m
    assert sl.slot("a") is None and sorted(sl._free) == [0, 1] and sl.calls == math.ceil(L / 3000)
    sl.close()
    ref = _one_push("b400_talk")
    assert np.array_equal(_bits(np.concatenate(ya)), _bits(ref[0]))
    assert np.array_equal(_bits64(np.concatenate(G)), _bits64(ref[1])) and np.array_equal(np.concatenate(F).astype(np.int64), ref[2])
    assert np.array_equal(_bits(np.concatenate(yb)), _bits(x))          # no target: measured and copied
    st = stats.cpu().numpy()
    assert np.array_equal(_bits64(st[0]), _bits64(ref[3])) and _bits64(st[1, 0]) == _bits64(ref[3][0]) and st[1, 2] == 1.0
