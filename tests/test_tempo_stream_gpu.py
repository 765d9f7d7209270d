"""smi_tempos_* through the C ABI (and audio.StreamTempo) against tests/tempo_ref.py of the WHOLE input: the concatenation of a
stream's pieces and the frame places bit for bit, whatever the pushes, the slot, the row and the other rows; every refusal
before anything changes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tempo_ref as R
from sparkmi import _lib, audio, streaming

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
TEMPOS = [(5, 4), (4, 5), (2, 1), (1, 2), (101, 100), (1, 1), (3, 2)]
FRAMES = [(16, 4), (16, 0), (64, 8), (512, 240)]
PRIMES = [7, 13, 31, 61, 127, 251, 509, 1021]


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _square(L, period=8, amp=0.25):
    return np.where((np.arange(L) % period) < period // 2, amp, -amp).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _row(kind, L, seed):
    x = {"noise": lambda: R.signal(L, seed), "zero": lambda: np.zeros(L, dtype=np.float32), "square": lambda: _square(L)}[kind]()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(kind, L, seed, p, q, N, D):
    """the reference of one whole input, computed once and shared (read only)"""
    searched = []
    out, s = R.tempo(_row(kind, L, seed), p, q, N, D, searched)
    out.setflags(write=False)
    s.setflags(write=False)
    return out, s, tuple(searched)


def _cuts(style, L, N):
    if style == "ones":
        return [1] * L
    if style == "whole":
        return [L, 0]                      # one whole row, then an empty last push
    step = [N // 2] if style == "H" else PRIMES
    out, i = [], 0
    while sum(out) < L:
        out.append(min(step[i % len(step)], L - sum(out)))
        i += 1
    return out + ([0] if style == "primes" else [])


class Handle:
    """one smi_tempos handle and the host's own count of every stream"""

    def __init__(self, max_streams, max_chunk, N, D):
        self.l, self.N, self.D = _lib.lib(), N, D
        self.h = C.c_void_p()
        w = np.ascontiguousarray(R.window(N))
        self.l.check(self.l.smi_tempos_create(max_streams, max_chunk, N, D, w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self.h)),
                     "smi_tempos_create")
        self.state = {}

    def close(self):
        self.l.smi_tempos_destroy(self.h)

    def open(self, slot, p, q):
        self.l.check(self.l.smi_tempos_open(self.h, slot, p, q), "smi_tempos_open")
        self.state[slot] = [p, q, 0, 0]

    def raw(self, x, slots, lens, lasts, B, out, pos):
        got = (C.c_int32 * max(1, len(slots)))(*([-9] * max(1, len(slots))))
        rc = self.l.smi_tempos_push_rows(self.h, C.c_void_p(x.data_ptr()), x.shape[1], _i32(slots), _i32(lens), _i32(lasts), B,
                                         None if pos is None else C.c_void_p(pos.data_ptr()), 0 if pos is None else pos.shape[1],
                                         C.c_void_p(out.data_ptr()), out.shape[1], got, None)
        return rc, self.l.smi_last_error().decode(), list(got)

    def push(self, rows, pad=3, extra=0, places=True):
        """rows [(slot, chunk, last)]: one call; NaN fills the input past every chunk's length.  Returns per row (piece, places)
        as device tensors, after checking the lengths; ``_gather`` checks the zero fill."""
        B = len(rows)
        want, nf = [], []
        for slot, c, last in rows:
            st = self.state[slot]
            f0 = st[3]
            piece, st[2], st[3] = streaming.tempo_piece_len(st[0], st[1], self.N, self.D, st[2], st[3], len(c), last)
            want.append(piece)
            nf.append(st[3] - f0)
        x = np.full((B, max([1] + [len(c) for _, c, _ in rows]) + extra), np.nan, dtype=np.float32)
        for b, (_, c, _) in enumerate(rows):
            x[b, : len(c)] = c
        xd = torch.from_numpy(x).to(DEV)
        out = torch.full((B, max([1] + want) + pad), SENTINEL, dtype=torch.float32, device=DEV)
        pos = torch.full((B, max([1] + nf) + pad), -7, dtype=torch.int32, device=DEV) if places else None
        rc, err, got = self.raw(xd, [r[0] for r in rows], [len(r[1]) for r in rows], [r[2] for r in rows], B, out, pos)
        assert rc == 0, err
        assert got[:B] == want
        return [(out[b], want[b], None if pos is None else pos[b], nf[b]) for b in range(B)]


def _gather(parts):
    """parts [(out row, piece length, pos row, frames)] of one stream in order -> (samples, places); the fill behind every piece
    and every push's places must be zeros"""
    ys, ps = [], []
    for o, m, p, f in parts:
        o = o.cpu().numpy()
        assert not o[m:].any(), "zeros behind the piece"
        ys.append(o[:m])
        if p is not None:
            p = p.cpu().numpy()
            assert not p[f:].any()
            ps.append(p[:f])
    return np.concatenate(ys), (np.concatenate(ps) if ps else None)


def _straddles(s, searched, p, q, N, D, edges):
    """does a searched frame read across a push edge?  Its target is [t_k, t_k + N), its candidates [a_k - D, a_k + D + N)"""
    H = N // 2
    for k in searched:
        t, a = int(s[k - 1]) + H, (k * H * p) // q
        lo, hi = min(t, a - D), max(t + N, a + D + N)
        if any(lo < e < hi for e in edges):
            return True
    return False


# (pushes of one sample at the smallest frame, where a row has 357 of them)
@pytest.mark.parametrize("N,D,style", [(N, D, st) for N, D in FRAMES for st in ("ones", "primes", "H", "whole") if st != "ones" or N == 16])
def test_pieces_and_places_are_the_batch_result(N, D, style):
    L = 20 * N + 37
    x = _row("noise", L, N + D)
    cuts = _cuts(style, L, N)
    h = Handle(len(TEMPOS), L, N, D)
    try:
        for slot, (p, q) in enumerate(TEMPOS):
            h.open(slot, p, q)
        parts = [[] for _ in TEMPOS]
        at = 0
        for i, c in enumerate(cuts):
            got = h.push([(slot, x[at: at + c], i == len(cuts) - 1) for slot in range(len(TEMPOS))])
            for slot, g in enumerate(got):
                parts[slot].append(g)
            at += c
        torch.cuda.synchronize()
        edges = np.cumsum(cuts)[:-1].tolist()
        for slot, (p, q) in enumerate(TEMPOS):
            want, s, searched = _ref("noise", L, N + D, p, q, N, D)
            y, places = _gather(parts[slot])
            assert np.array_equal(places, s.astype(np.int32)), (p, q)
            assert y.size == want.size and np.array_equal(_bits(y), _bits(want)), (p, q)
            if (p, q) == (1, 1):             # a copy with no latency: every piece is its push
                assert [g[1] for g in parts[slot]] == cuts
            elif style != "whole" and ((N, D, p, q) == (64, 8, 3, 2) or ((N, D) == (16, 0) and (p, q) != (101, 100))):
                assert len(searched) >= len(s) // 2 and _straddles(s, searched, p, q, N, D, edges), (p, q, len(searched))
            if (p, q) != (1, 1) and style == "ones":
                assert sum(g[1] == 0 for g in parts[slot]) > 0, "no push that emits nothing"
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["zero", "square"])
def test_silence_and_a_square_wave_cut_mid_frame(kind):
    """every distance ties on silence and many do on a square wave: the places are the tie rule's"""
    N, D, L = 64, 8, 20 * 64 + 37
    x = _row(kind, L, 0)
    tempos = [(3, 2), (4, 5), (2, 1)]
    cuts = [45] * (L // 45) + [L % 45]
    h = Handle(3, 64, N, D)
    try:
        for slot, (p, q) in enumerate(tempos):
            h.open(slot, p, q)
        parts, at = [[] for _ in tempos], 0
        for i, c in enumerate(cuts):
            for slot, g in enumerate(h.push([(slot, x[at: at + c], i == len(cuts) - 1) for slot in range(3)])):
                parts[slot].append(g)
            at += c
        for slot, (p, q) in enumerate(tempos):
            want, s, _ = _ref(kind, L, 0, p, q, N, D)
            y, places = _gather(parts[slot])
            assert np.array_equal(places, s.astype(np.int32)) and np.array_equal(_bits(y), _bits(want)), (kind, p, q)
    finally:
        h.close()


def test_five_ragged_streams_with_their_own_tempos_in_one_call():
    N, D = 64, 8
    spec = [(1317, (5, 4), 97), (640, (4, 5), 64), (33, (2, 1), 33), (1000, (1, 2), 211), (801, (1, 1), 50)]   # (L, tempo, push length)
    h = Handle(8, 256, N, D)
    try:
        slots = [6, 0, 3, 7, 2]
        for slot, (_, (p, q), _) in zip(slots, spec):
            h.open(slot, p, q)
        parts, at = [[] for _ in spec], [0] * len(spec)
        while any(a is not None for a in at):
            rows, who = [], []
            for i, (L, _, step) in enumerate(spec):
                if at[i] is None:
                    continue
                c = min(step, L - at[i])
                last = at[i] + c == L
                rows.append((slots[i], _row("noise", L, 40 + i)[at[i]: at[i] + c], last))
                who.append(i)
                at[i] = None if last else at[i] + c
            for i, g in zip(who, h.push(rows, extra=len(rows))):
                parts[i].append(g)
        for i, (L, (p, q), _) in enumerate(spec):
            want, s, _ = _ref("noise", L, 40 + i, p, q, N, D)
            y, places = _gather(parts[i])
            assert np.array_equal(places, s.astype(np.int32)) and np.array_equal(_bits(y), _bits(want)), i
    finally:
        h.close()


def test_a_stream_alone_and_in_slot_37_of_64():
    """the same stream alone in a handle of one slot, and in slot 37 as row 5 of calls whose other rows, strides and lengths
    differ: the same bits, those of the reference"""
    N, D, L, (p, q) = 64, 8, 20 * 64 + 37, (3, 2)
    x = _row("noise", L, 72)
    want, s, _ = _ref("noise", L, 72, p, q, N, D)
    cuts = _cuts("primes", L, N)
    alone = Handle(1, L, N, D)
    crowd = Handle(64, L, N, D)
    try:
        alone.open(0, p, q)
        others = [3, 63, 0, 12, 36, 38, 5]
        for k, slot in enumerate(others):
            crowd.open(slot, *TEMPOS[k % len(TEMPOS)])
        crowd.open(37, p, q)
        a_parts, c_parts, at = [], [], 0
        for i, c in enumerate(cuts):
            last = i == len(cuts) - 1
            a_parts += alone.push([(0, x[at: at + c], last)], pad=1)
            rows = [(slot, _row("noise", 4000, 90 + slot)[i * 100: i * 100 + 17 * (k + 1) + i], False) for k, slot in enumerate(others)]
            rows.insert(5, (37, x[at: at + c], last))
            c_parts.append(crowd.push(rows, pad=5 + i, extra=i)[5])
            at += c
        for parts in (a_parts, c_parts):
            y, places = _gather(parts)
            assert np.array_equal(places, s.astype(np.int32)) and np.array_equal(_bits(y), _bits(want))
        assert [g[1] for g in a_parts] == [g[1] for g in c_parts]
    finally:
        alone.close()
        crowd.close()


def test_a_key_twice_in_one_poll_and_the_default_frame_through_stream_tempo():
    """audio.StreamTempo: a request's last chunk and its empty flush in one push make two calls; the pieces are the reference's"""
    N, D = audio.tempo_frame(16000)
    L = 20 * N + 37
    xa, xb = _row("noise", L, 11), _row("noise", 3000, 12)
    t = audio.StreamTempo(4, L, (N, D), device=DEV)
    try:
        t.open("a", 5, 4)
        t.open("b", 4, 5)
        dev = lambda rows: torch.from_numpy(np.stack([np.pad(r, (0, L - r.size), constant_values=np.nan) for r in rows])).to(DEV)  # noqa: E731
        o1, n1 = t.push(dev([xa[:5000], xb[:1999]]), [("a", 5000, False), ("b", 1999, False)])
        o2, n2, pos, nf = t.push(dev([xa[5000:], xa[:0], xb[1999:]]), [("a", L - 5000, False), ("a", 0, True), ("b", 1001, True)],
                                 return_places=True)
        assert t.calls == 3 and t.slot("a") is None and t.slot("b") is None
        wa, sa, _ = _ref("noise", L, 11, 5, 4, N, D)
        wb, sb, _ = _ref("noise", 3000, 12, 4, 5, N, D)
        o1, o2, pos = o1.cpu().numpy(), o2.cpu().numpy(), pos.cpu().numpy()
        ya = np.concatenate([o1[0, : n1[0]], o2[0, : n2[0]], o2[1, : n2[1]]])
        yb = np.concatenate([o1[1, : n1[1]], o2[2, : n2[2]]])
        assert np.array_equal(_bits(ya), _bits(wa)) and np.array_equal(_bits(yb), _bits(wb))
        assert n2[1] > 0 and np.array_equal(np.concatenate([pos[0, : nf[0]], pos[1, : nf[1]]]), sa.astype(np.int32)[-(nf[0] + nf[1]):])
    finally:
        t.close()


def test_every_refusal_leaves_state_and_output_untouched():
    N, D, L, (p, q) = 16, 4, 20 * 16 + 37, (5, 4)
    x = _row("noise", L, 21)
    want, s, _ = _ref("noise", L, 21, p, q, N, D)
    h = Handle(4, 200, N, D)
    l = h.l
    try:
        for bad, name in (((9, p, q), "stream"), ((0, 0, q), "p"), ((0, p, 0), "q"), ((0, 9, 2), "p/q")):
            assert l.smi_tempos_open(h.h, *bad) == EINVAL and name in l.smi_last_error().decode()
        h.open(0, p, q)
        h.open(2, 1, 2)
        parts = h.push([(0, x[:150], False), (2, x[:90], False)])[:1]
        xd = torch.from_numpy(np.stack([np.pad(x[150:250], (0, 300), constant_values=np.nan)] * 2)).to(DEV)
        out = torch.full((2, 400), SENTINEL, dtype=torch.float32, device=DEV)
        pos = torch.full((2, 64), -7, dtype=torch.int32, device=DEV)
        small = torch.full((2, 8), SENTINEL, dtype=torch.float32, device=DEV)
        tiny = torch.full((2, 1), -7, dtype=torch.int32, device=DEV)
        cases = [
            (([0, 4], [100, 100], [0, 0], 2, out, pos), "stream[1]"),
            (([0, 1], [100, 100], [0, 0], 2, out, pos), "not open"),
            (([0, 0], [100, 100], [0, 0], 2, out, pos), "stream too"),
            (([0, 2], [100, 100], [0, 2], 2, out, pos), "last[1]"),
            (([0, 2], [100, 201], [0, 0], 2, out, pos), "len[1]"),
            (([0, 2], [-1, 100], [0, 0], 2, out, pos), "len[0]"),
            (([0, 2], [100, 100], [0, 0], 0, out, pos), "B="),
            (([0, 2], [100, 100], [0, 0], 65, out, pos), "B="),
            (([0, 2], [100, 100], [0, 0], 2, small, pos), "out_stride"),
            (([0, 2], [100, 100], [0, 0], 2, out, tiny), "pos_stride"),
            (([0, 2], [100, 100], [0, 0], 2, xd, pos), "overlaps"),
        ]
        for (slots, lens, lasts, B, o, ps), name in cases:
            rc, err, got = h.raw(xd, slots, lens, lasts, B, o, ps)
            assert rc == EINVAL and name in err, (name, rc, err)
            assert got == [-9, -9], name                    # not even the lengths are filled
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((small == SENTINEL).all()) and bool((pos == -7).all())
        # the streams go on as if nothing had been asked
        parts += h.push([(0, x[150:250], False), (2, x[90:180], False)])[:1]
        parts += h.push([(0, x[250:], True)])
        y, places = _gather(parts)
        assert np.array_equal(places, s.astype(np.int32)) and np.array_equal(_bits(y), _bits(want))
        rc, err, _ = h.raw(xd, [0], [10], [0], 1, out, pos)
        assert rc == EINVAL and "not open" in err               # a stream closes with its last push
    finally:
        h.close()
