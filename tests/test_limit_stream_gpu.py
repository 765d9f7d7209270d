"""smi_limits_* through the C ABI (and audio.StreamLimiter) against tests/limit_ref.py of the WHOLE stream at g = 1: the pieces
concatenated and the stats bit for bit, whatever the pushes, the slot, the row, the strides and the other rows; the stats after
every push are those of the samples emitted so far; every refusal before anything changes, checked by taking the stream to a
correct end."""
import ctypes as C

import numpy as np
import pytest
import torch

import limit_ref as LR
import limit_stream_ref as S
from sparkmi import _lib, audio

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
MAX_CHUNK = 8192


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Handle:
    """one smi_limits handle and the host's own count of every stream"""

    def __init__(self, A, R, max_streams=80, max_chunk=MAX_CHUNK, n_taps=None):
        self.l, self.A, self.R = _lib.lib(), A, R
        self.h = C.c_void_p()
        self.win = np.ascontiguousarray(audio.limiter_window(A, R), dtype=np.float64)
        self.taps = LR.taps()
        self.l.check(self.l.smi_limits_create(max_streams, max_chunk, A, R, _dp(self.win), _dp(self.taps),
                                              self.taps.size if n_taps is None else n_taps, LR.PHASES, C.byref(self.h)), "smi_limits_create")
        self.n = {}

    def close(self):
        self.l.smi_limits_destroy(self.h)

    def open(self, slot, mode, ceiling):
        self.l.check(self.l.smi_limits_open(self.h, slot, int(mode == "true"), ceiling), "smi_limits_open")
        self.n[slot] = 0

    def raw(self, x_ptr, stride, slots, lens, lasts, B, out_ptr, out_stride, stats_ptr=None):
        got = (C.c_int32 * max(1, len(slots)))(*([-9] * max(1, len(slots))))
        rc = self.l.smi_limits_push_rows(self.h, C.c_void_p(x_ptr), stride, _i32(slots), _i32(lens), _i32(lasts), B, C.c_void_p(out_ptr),
                                         out_stride, got, None if stats_ptr is None else C.c_void_p(stats_ptr), None)
        return rc, self.l.smi_last_error().decode(), list(got)

    def push(self, rows, pad=3, extra=0):
        """rows [(slot, chunk, last)]: one call; NaN fills the input past every chunk's length.  Returns per row (piece row,
        piece length, stats row) as device tensors, after checking the lengths."""
        B = len(rows)
        want = []
        for slot, c, last in rows:
            piece, self.n[slot] = S.piece_len(self.A, self.R, self.n[slot], len(c), last)
            want.append(piece)
        x = np.full((B, max([1] + [len(c) for _, c, _ in rows]) + extra), np.nan, dtype=np.float32)
        for b, (_, c, _) in enumerate(rows):
            x[b, : len(c)] = c
        xd = torch.from_numpy(x).to(DEV)
        out = torch.full((B, max([1] + want) + pad), SENTINEL, dtype=torch.float32, device=DEV)
        stats = torch.full((B, 4), -7.0, dtype=torch.float64, device=DEV)
        rc, err, got = self.raw(xd.data_ptr(), x.shape[1], [r[0] for r in rows], [len(r[1]) for r in rows], [r[2] for r in rows], B,
                                out.data_ptr(), out.shape[1], stats.data_ptr())
        assert rc == 0, err
        assert got[:B] == want
        return [(out[b], want[b], stats[b]) for b in range(B)]

    def whole(self, slot, x, pushes, mode, ceiling):
        """one stream alone, pushed straight from one device copy of it (what lies past a chunk is the stream's own future) into
        one device row, piece behind piece.  Returns (samples, the stats after every push)."""
        self.open(slot, mode, ceiling)
        L = len(x)
        xd = torch.from_numpy(np.concatenate([x, np.full(8, np.nan, dtype=np.float32)])).to(DEV)
        out = torch.full((L + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        stats = torch.full((len(pushes), 4), -7.0, dtype=torch.float64, device=DEV)
        n = done = 0
        for t, length in enumerate(pushes):
            last = t == len(pushes) - 1
            piece, n1 = S.piece_len(self.A, self.R, n, length, last)
            rc, err, got = self.raw(xd.data_ptr() + 4 * n, max(1, length), [slot], [length], [last], 1, out.data_ptr() + 4 * done,
                                    max(1, piece), stats.data_ptr() + 32 * t)
            assert rc == 0, err
            assert got[0] == piece
            n, done = n1, done + piece
        assert done == L
        o = out.cpu().numpy()
        assert o[L] in (0.0, SENTINEL) and (o[L + 1:] == SENTINEL).all()    # (an empty piece writes its row's one zero)
        return o[:L], stats.cpu().numpy()


@pytest.fixture(scope="module")
def handles():
    hs = {}

    def get(A, R):
        if (A, R) not in hs:
            hs[(A, R)] = Handle(A, R)
        return hs[(A, R)]

    yield get
    for h in hs.values():
        h.close()


def _stats_at(c, n, last):
    """the stats of the stream ``c`` after n samples: over the samples emitted so far"""
    w = c["want"]
    E = n if last else S.emitted(n, c["A"], c["R"])
    if not E:
        return np.array([0.0, 1.0, 1.0, 0.0])
    return np.array([w["e"][:E].max(), 1.0, w["s"][:E].min(), float(np.count_nonzero(w["s"][:E] < 1.0))])


def _check(c, h, slot, pushes, what):
    got, stats = h.whole(slot, c["x"], pushes, c["mode"], c["ceiling"])
    assert np.array_equal(_bits(got), _bits(c["want"]["out"])), (c["name"], what)
    assert np.array_equal(stats[-1], c["want"]["stats"]), (c["name"], what, stats[-1], c["want"]["stats"])
    n = 0
    for t, length in enumerate(pushes):
        n += length
        assert np.array_equal(stats[t], _stats_at(c, n, t == len(pushes) - 1)), (c["name"], what, t)
    assert not got.size or float(np.abs(got).max()) <= c["ceiling"], (c["name"], what)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("A,R", S.REACHES)
def test_every_case_and_every_chunking_is_the_batch_reference_bit_for_bit(handles, A, R, mode):
    h = handles(A, R)
    cases = [c for c in S.reference() if (c["A"], c["R"], c["mode"]) == (A, R, mode)]
    assert len(cases) >= 17
    limited = 0
    for i, c in enumerate(cases):
        for name, pushes in S.chunkings(c).items():
            _check(c, h, (5 * i + 3) % 80, pushes, name)
        limited += int(c["want"]["stats"][3])
    assert limited > 0


def test_a_stream_as_row_37_of_64_in_another_slot_with_another_stride(handles):
    h = handles(40, 400)
    c = S.case("A40_R400_true_edge")
    others = [k for k in S.reference() if (k["A"], k["R"]) == (40, 400) and k["x"].size >= 600]
    rows = [others[b % len(others)] for b in range(64)]
    rows[37] = c
    for b in range(64):
        h.open(b + 9, rows[b]["mode"], rows[b]["ceiling"])
    L = max(k["x"].size for k in rows)
    step, at, pieces, stats = 509, 0, [], None
    while at < L:
        call = []
        for b, k in enumerate(rows):
            if at < k["x"].size:
                call.append((b, (b + 9, k["x"][at: at + step], at + step >= k["x"].size)))
        res = h.push([r for _, r in call], pad=5 + at % 3, extra=at % 11)
        for (b, _), (o, m, st) in zip(call, res):
            o = o.cpu().numpy()
            assert not o[m:].any()                            # zeros from the piece's end to the stride
            if b == 37:
                pieces.append(o[:m])
                stats = st.cpu().numpy()
        at += step
    got = np.concatenate(pieces)
    assert np.array_equal(_bits(got), _bits(c["want"]["out"]))
    assert np.array_equal(stats, c["want"]["stats"])


def test_the_fill_behind_a_piece_is_zeros_and_nan_past_a_chunk_is_not_read(handles):
    h = handles(3, 5)
    c = S.case("A3_R5_true_hot")
    h.open(1, c["mode"], c["ceiling"])
    x, at, pieces = c["x"], 0, []
    for length in [100, 0, 333, 1, x.size - 434]:
        (o, m, _), = h.push([(1, x[at: at + length], at + length == x.size)], pad=7, extra=13)
        o = o.cpu().numpy()
        assert not o[m:].any()
        pieces.append(o[:m])
        at += length
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(c["want"]["out"]))


def test_two_handles_interleaved():
    a, b = Handle(40, 400, max_streams=2), Handle(3, 5, max_streams=2)
    try:
        ca, cb = S.case("A40_R400_true_hot"), S.case("A3_R5_sample_hot")
        a.open(1, ca["mode"], ca["ceiling"])
        b.open(1, cb["mode"], cb["ceiling"])
        pa, pb, at = [], [], 0
        while at < max(ca["x"].size, cb["x"].size):
            for h, c, p in ((a, ca, pa), (b, cb, pb)):
                if at < c["x"].size:
                    (o, m, st), = h.push([(1, c["x"][at: at + 251], at + 251 >= c["x"].size)])
                    p.append((o[:m].cpu().numpy(), st.cpu().numpy()))
            at += 251
        for c, p in ((ca, pa), (cb, pb)):
            assert np.array_equal(_bits(np.concatenate([o for o, _ in p])), _bits(c["want"]["out"]))
            assert np.array_equal(p[-1][1], c["want"]["stats"])
    finally:
        a.close()
        b.close()


def test_two_streams_of_different_modes_and_ceilings_in_one_call(handles):
    h = handles(40, 400)
    ca, cb = S.case("A40_R400_true_quarter"), S.case("A40_R400_sample_edge")
    assert ca["ceiling"] != cb["ceiling"] and ca["mode"] != cb["mode"]
    h.open(70, ca["mode"], ca["ceiling"])
    h.open(3, cb["mode"], cb["ceiling"])
    pa, pb, at, sa, sb = [], [], 0, None, None
    while at < max(ca["x"].size, cb["x"].size):
        call = [(s, c["x"][at: at + 129], at + 129 >= c["x"].size) for s, c in ((70, ca), (3, cb)) if at < c["x"].size]
        for (s, _, _), (o, m, st) in zip(call, h.push(call)):
            (pa if s == 70 else pb).append(o[:m].cpu().numpy())
            if s == 70:
                sa = st.cpu().numpy()
            else:
                sb = st.cpu().numpy()
        at += 129
    assert np.array_equal(_bits(np.concatenate(pa)), _bits(ca["want"]["out"])) and np.array_equal(sa, ca["want"]["stats"])
    assert np.array_equal(_bits(np.concatenate(pb)), _bits(cb["want"]["out"])) and np.array_equal(sb, cb["want"]["stats"])
    # the quarter-rate sine: the sample mode sees no over, the true-peak mode does
    assert S.case("A40_R400_sample_quarter")["want"]["stats"][3] == 0 and ca["want"]["stats"][3] > 0


def test_stream_limiter_class(handles):
    c = S.case("A40_R400_true_first_last")
    sl = audio.StreamLimiter(4, 1000, device=DEV)
    assert (sl.lookahead, sl.release, sl.delay) == (40, 400, 450)
    sl.open("a", "true", c["ceiling"])
    x = torch.from_numpy(c["x"].copy()).to(DEV)
    L, at, pieces = c["x"].size, 0, []
    first = True
    while at < L:
        n = min(700, L - at)
        rows = [("a", n, at + n == L)]
        if first:
            rows = [("a", 300, False), ("a", n - 300, at + n == L)]      # a key twice: two device calls
        xin = torch.zeros((len(rows), 1000), dtype=torch.float32, device=DEV)
        o = at
        for b, (_, m, _) in enumerate(rows):
            xin[b, :m] = x[o: o + m]
            o += m
        assert sl.piece_lengths(rows) == [S.piece_len(40, 400, at, rows[0][1], rows[0][2])[0]] + \
            ([S.piece_len(40, 400, at + 300, rows[1][1], rows[1][2])[0]] if first else [])
        out, lens = sl.push(xin, rows)
        for b, m in enumerate(lens):
            pieces.append(out[b, :m].cpu().numpy())
        first = False
        at += n
    assert sl.calls == 2 + (L - 1) // 700 and sl.slot("a") is None
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(c["want"]["out"]))
    assert np.array_equal(sl.last_stats[0].cpu().numpy(), c["want"]["stats"])
    with pytest.raises(ValueError, match="mode"):
        sl.open("b", "loud")
    sl.close()


def test_every_refusal_leaves_the_stream_as_it_was(handles):
    h = handles(3, 5)
    l = h.l
    c = S.case("A3_R5_true_first_last")
    x = c["x"]
    L = x.size
    h.open(2, c["mode"], c["ceiling"])
    h.open(4, "sample", 0.5)
    xd = torch.from_numpy(np.stack([x[:600], x[:600]])).to(DEV)
    out = torch.full((2, 700), SENTINEL, dtype=torch.float32, device=DEV)
    pieces = []

    def refused(what, *a, **k):
        rc, err, got = h.raw(*a, **k)
        assert rc == EINVAL and what in err, (what, rc, err)
        assert got[0] == -9                                   # nothing was filled in
        assert (out.cpu().numpy() == SENTINEL).all()          # and nothing was launched

    def good(lo, hi, last):
        (o, m, st), = h.push([(2, x[lo:hi], last)])
        pieces.append(o[:m].cpu().numpy())
        return st.cpu().numpy()

    good(0, 300, False)
    X, O = xd.data_ptr(), out.data_ptr()
    refused("is not open", X, 600, [7], [10], [0], 1, O, 700)                      # never opened
    refused("outside 0..", X, 600, [80], [10], [0], 1, O, 700)                     # no such slot
    refused("is row 0's stream too", X, 600, [2, 2], [10, 10], [0, 0], 2, O, 700)  # twice in one call
    refused("max_chunk", X, 600 + MAX_CHUNK, [2], [MAX_CHUNK + 1], [0], 1, O, 700)
    refused("outside 0..min", X, 600, [2], [601], [0], 1, O, 700)                  # len > stride
    refused("outside 0..min", X, 600, [2], [-1], [0], 1, O, 700)
    refused("B=65", X, 600, [2] * 65, [1] * 65, [0] * 65, 65, O, 700)
    refused("B=0", X, 600, [2], [1], [0], 0, O, 700)
    refused("last[0]=2", X, 600, [2], [10], [2], 1, O, 700)
    refused("overlaps", X, 600, [2], [10], [0], 1, X + 40, 700)                    # out_dev inside in_dev
    refused("out_stride", X, 600, [2], [600], [0], 1, O, 599)                      # shorter than the piece of 600
    refused("out_stride", X, 600, [2, 4], [10, 600], [0, 1], 2, O, 599)            # ... of any row; row 0 is not pushed either
    refused("stride=0", X, 0, [2], [0], [0], 1, O, 700)
    rc, err, _ = h.raw(0, 600, [2], [10], [0], 1, O, 700)
    assert rc == EINVAL and "null" in err
    # smi_limits_open: the slot, the mode, the ceiling; a true-peak stream on a handle without taps
    for args, what in (((80, 1, 0.5), "stream=80"), ((1, 2, 0.5), "true_peak=2"), ((1, 1, 0.0), "ceiling"), ((1, 1, float("nan")), "ceiling"),
                       ((1, 1, float("inf")), "ceiling")):
        assert l.smi_limits_open(h.h, *args) == EINVAL and what in l.smi_last_error().decode(), what
    bare = Handle(3, 5, max_streams=2, n_taps=0)
    try:
        assert l.smi_limits_open(bare.h, 0, 1, 0.5) == EINVAL and "n_taps=0" in l.smi_last_error().decode()
        assert l.smi_limits_open(bare.h, 0, 0, 0.5) == 0
    finally:
        bare.close()
    # the stream goes on to a correct end, and slot 4 was never pushed: it is still at its start
    good(300, 301, False)
    st = good(301, L, True)
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(c["want"]["out"])) and np.array_equal(st, c["want"]["stats"])
    refused("is not open", X, 600, [2], [10], [0], 1, O, 700)                      # closed by its last push
    k = S.case("A3_R5_sample_hot")
    (o, m, st), = h.push([(4, k["x"], True)])
    want = LR.limit(k["x"], 1.0, 0.5, None, 3, 5, audio.limiter_window(3, 5))
    assert np.array_equal(_bits(o[:m].cpu().numpy()), _bits(want["out"])) and np.array_equal(st.cpu().numpy(), want["stats"])


def test_a_stream_is_refused_before_it_passes_2_to_the_28(handles):
    """the count is the host's: empty device work is not needed to reach it"""
    big = Handle(0, 0, max_streams=1, max_chunk=1 << 24)
    try:
        big.open(0, "sample", 0.5)
        xd = torch.zeros((1, 1 << 24), dtype=torch.float32, device=DEV)
        out = torch.empty((1, 1 << 24), dtype=torch.float32, device=DEV)
        for _ in range(16):
            rc, err, got = big.raw(xd.data_ptr(), 1 << 24, [0], [1 << 24], [0], 1, out.data_ptr(), 1 << 24)
            assert rc == 0, err
        rc, err, got = big.raw(xd.data_ptr(), 1 << 24, [0], [1], [0], 1, out.data_ptr(), 1 << 24)
        assert rc == EINVAL and "2^28" in err and got[0] == -9
        rc, err, got = big.raw(xd.data_ptr(), 1 << 24, [0], [0], [1], 1, out.data_ptr(), 1 << 24)
        assert rc == 0 and got[0] == 10, err                 # the last, empty push: the ten samples held back
        torch.cuda.synchronize()
        assert not out[0, :10].cpu().numpy().any()
    finally:
        big.close()
