"""smi_pitchs_* through the C ABI (and audio.StreamPitch) against tests/pitch_ref.py of the WHOLE input: the concatenation of a
stream's pieces and the stretch's frame places bit for bit, whatever the pushes, the slot, the row and the other rows; one
independent cross-check against the device's own StreamTempo and StreamJoiner; every refusal before anything changes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pitch_ref as P
import pitch_stream_ref as PS
import tempo_ref as R
from sparkmi import _lib, audio, streaming

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
EINVAL = -1   # include/sparkmi.h, SMI_EINVAL
PITCHES = [(3, 2), (2, 3), (28, 25), (89, 100)]
TEMPOS = [(1, 1), (5, 4), (4, 5)]
PAIRS = [(t, r) for r in PITCHES for t in TEMPOS]
PRIMES = [7, 13, 31, 61, 127, 251, 509, 1021]
MAX_TAPS = 3981


def _i32(v):
    v = [int(a) for a in v]
    return (C.c_int32 * len(v))(*v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _row(L, seed):
    x = R.signal(L, seed)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(L, seed, t, r, N, D):
    """the reference of one whole input, computed once and shared (read only)"""
    out, s = P.pitch(_row(L, seed), t, r, N, D)
    out.setflags(write=False)
    s.setflags(write=False)
    return out, s


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
    """one smi_pitchs handle and the host's own count of every stream"""

    def __init__(self, max_streams, max_chunk, N, D, max_taps=MAX_TAPS):
        self.l, self.N, self.D = _lib.lib(), N, D
        self.h = C.c_void_p()
        w = np.ascontiguousarray(R.window(N))
        self.l.check(self.l.smi_pitchs_create(max_streams, max_chunk, N, D, w.ctypes.data_as(C.POINTER(C.c_double)), max_taps,
                                              C.byref(self.h)), "smi_pitchs_create")
        self.state = {}

    def close(self):
        self.l.smi_pitchs_destroy(self.h)

    def raw_open(self, slot, t, r, taps):
        n = 0 if taps is None else int(taps.size)
        rc = self.l.smi_pitchs_open(self.h, slot, t[0], t[1], r[0], r[1], None if taps is None else taps.ctypes.data_as(C.POINTER(C.c_float)),
                                    n, None)
        return rc, self.l.smi_last_error().decode()

    def open(self, slot, t, r):
        pl = P.plan(0, t, r, self.N)
        taps = None if (pl["up"], pl["down"]) == (1, 1) else np.ascontiguousarray(P.taps32(pl["up"], pl["down"]))
        rc, err = self.raw_open(slot, t, r, taps)
        assert rc == 0, err
        if taps is not None:
            taps[:] = np.nan               # the host buffer is free on return
        self.state[slot] = [t, r, 0 if taps is None else int(taps.size), 0, 0, 0]

    def raw(self, x, slots, lens, lasts, B, out, pos):
        got = (C.c_int32 * max(1, len(slots)))(*([-9] * max(1, len(slots))))
        rc = self.l.smi_pitchs_push_rows(self.h, C.c_void_p(x.data_ptr()), x.shape[1], _i32(slots), _i32(lens), _i32(lasts), B,
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
            f0 = st[4]
            piece, st[3], st[4], st[5] = streaming.pitch_piece_len(*st[0], *st[1], self.N, self.D, st[2], st[3], st[4], st[5], len(c), last)
            want.append(piece)
            nf.append(st[4] - f0)
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


def _same(parts, want, s, what):
    y, places = _gather(parts)
    assert np.array_equal(places, s.astype(np.int32)), what
    assert y.size == want.size and np.array_equal(_bits(y), _bits(want)), what


def _run(h, slots, specs, cuts, x, **kw):
    """the streams ``slots`` all fed ``x`` in ``cuts``: per slot its parts"""
    parts, at = [[] for _ in slots], 0
    for i, c in enumerate(cuts):
        got = h.push([(slot, x[at: at + c], i == len(cuts) - 1) for slot in slots], **kw)
        for j, g in enumerate(got):
            parts[j].append(g)
        at += c
    return parts


# (pushes of one sample at the smallest frame, where a row has 357 of them)
@pytest.mark.parametrize("N,D,style", [(N, D, st) for N, D in ((16, 3), (64, 8)) for st in ("ones", "primes", "H", "whole")
                                       if st != "ones" or N == 16])
def test_pieces_and_places_are_the_batch_result(N, D, style):
    L = 20 * N + 37
    x = _row(L, N + D)
    cuts = _cuts(style, L, N)
    h = Handle(len(PAIRS), L, N, D)
    try:
        for slot, (t, r) in enumerate(PAIRS):
            h.open(slot, t, r)
        parts = _run(h, list(range(len(PAIRS))), PAIRS, cuts, x)
        torch.cuda.synchronize()
        quiet = two_tiles = 0
        for slot, (t, r) in enumerate(PAIRS):
            want, s = _ref(L, N + D, t, r, N, D)
            _same(parts[slot], want, s, (t, r))
            assert [g[1] for g in parts[slot]] == [p.size for p in PS.stream(x, cuts, t, r, N, D)[0]]
            quiet += sum(g[1] == 0 and g[3] > 0 for g in parts[slot])      # frames became final, no output did
            two_tiles += sum(g[1] > 1024 for g in parts[slot])
        if N == 16 and style in ("ones", "H"):   # (8 stretched samples are not yet the filter's reach)
            assert quiet > 0, "no push whose piece is empty although frames became final"
        if style == "whole" and N == 64:
            assert two_tiles > 0, "no piece of more than one tile"
    finally:
        h.close()


def test_the_long_filter_at_the_default_frame():
    """199/100: 3981 taps and the widest window of stretched samples in LDS; a piece of more than one tile"""
    N, D = audio.tempo_frame(16000)
    L, t, r = 6 * N + 40, (1, 1), (199, 100)
    x = _row(L, 5)
    want, s = _ref(L, 5, t, r, N, D)
    h = Handle(2, L, N, D)
    try:
        h.open(1, t, r)
        cuts = [1021, 509, 1, 1300, L - 2831, 0]
        parts = _run(h, [1], None, cuts, x)[0]
        _same(parts, want, s, "199/100")
        assert max(g[1] for g in parts) > 1024
    finally:
        h.close()


def test_seven_pairs_in_one_call_with_unpitched_and_plain_rows():
    """rp = rq is the tempo stream, tp = tq too a copy with no latency, and tp / tq = rp / rq a stretch that copies"""
    N, D, L = 64, 8, 20 * 64 + 37
    pairs = [((1, 1), (1, 1)), ((5, 4), (1, 1)), ((1, 1), (3, 2)), ((4, 5), (2, 3)), ((5, 4), (28, 25)), ((3, 2), (3, 2)), ((1, 1), (89, 100))]
    x = _row(L, 33)
    cuts = _cuts("primes", L, N)
    h = Handle(7, L, N, D)
    try:
        for slot, (t, r) in enumerate(pairs):
            h.open(slot, t, r)
        parts = _run(h, list(range(7)), pairs, cuts, x, extra=2)
        for slot, (t, r) in enumerate(pairs):
            want, s = _ref(L, 33, t, r, N, D)
            _same(parts[slot], want, s, (t, r))
        assert [g[1] for g in parts[0]] == cuts                           # a copy: every piece is its push
        tw, ts_ = R.tempo(x, 5, 4, N, D)
        assert np.array_equal(_bits(_gather(parts[1])[0]), _bits(tw))     # the tempo stream's bits
    finally:
        h.close()


def test_five_ragged_streams_with_their_own_ratios_in_one_call():
    N, D = 64, 8
    spec = [(1317, (5, 4), (28, 25), 97), (640, (4, 5), (2, 3), 64), (33, (1, 1), (3, 2), 33), (1000, (1, 1), (89, 100), 211),
            (801, (1, 1), (1, 1), 50)]   # (L, tempo, pitch, push length)
    h = Handle(8, 256, N, D)
    try:
        slots = [6, 0, 3, 7, 2]
        for slot, (_, t, r, _) in zip(slots, spec):
            h.open(slot, t, r)
        parts, at = [[] for _ in spec], [0] * len(spec)
        while any(a is not None for a in at):
            rows, who = [], []
            for i, (L, _, _, step) in enumerate(spec):
                if at[i] is None:
                    continue
                c = min(step, L - at[i])
                last = at[i] + c == L
                rows.append((slots[i], _row(L, 40 + i)[at[i]: at[i] + c], last))
                who.append(i)
                at[i] = None if last else at[i] + c
            for i, g in zip(who, h.push(rows, extra=len(rows))):
                parts[i].append(g)
        for i, (L, t, r, _) in enumerate(spec):
            want, s = _ref(L, 40 + i, t, r, N, D)
            _same(parts[i], want, s, i)
    finally:
        h.close()


def test_a_stream_alone_and_in_slot_37_of_64():
    """the same stream alone in a handle of one slot, and in slot 37 as row 5 of calls whose other rows, strides and lengths
    differ, NaN past every chunk: the same bits, those of the reference"""
    N, D, L, t, r = 64, 8, 20 * 64 + 37, (5, 4), (28, 25)
    x = _row(L, 72)
    want, s = _ref(L, 72, t, r, N, D)
    cuts = _cuts("primes", L, N)
    alone = Handle(1, L, N, D)
    crowd = Handle(64, L, N, D)
    try:
        alone.open(0, t, r)
        others = [3, 63, 0, 12, 36, 38, 5]
        for k, slot in enumerate(others):
            crowd.open(slot, *PAIRS[(5 * k) % len(PAIRS)])
        crowd.open(37, t, r)
        a_parts, c_parts, at = [], [], 0
        for i, c in enumerate(cuts):
            last = i == len(cuts) - 1
            a_parts += alone.push([(0, x[at: at + c], last)], pad=1)
            rows = [(slot, _row(4000, 90 + slot)[i * 100: i * 100 + 17 * (k + 1) + i], False) for k, slot in enumerate(others)]
            rows.insert(5, (37, x[at: at + c], last))
            c_parts.append(crowd.push(rows, pad=5 + i, extra=i)[5])
            at += c
        for parts in (a_parts, c_parts):
            _same(parts, want, s, "slot 37")
        assert [g[1] for g in a_parts] == [g[1] for g in c_parts]
    finally:
        alone.close()
        crowd.close()


def test_a_slot_opened_again_with_another_ratio():
    N, D, L = 16, 3, 20 * 16 + 37
    x, x2 = _row(L, 61), _row(L, 62)
    h = Handle(2, L, N, D)
    try:
        h.open(1, (5, 4), (3, 2))
        first = _run(h, [1], None, _cuts("primes", L, N), x)[0]
        h.open(1, (1, 1), (89, 100))          # longer taps, another stretch; the ended stream's state is of no account
        second = _run(h, [1], None, [100, 0, 57, 200], x2)[0]
        _same(first, *_ref(L, 61, (5, 4), (3, 2), N, D), "first")
        _same(second, *_ref(L, 62, (1, 1), (89, 100), N, D), "second")
    finally:
        h.close()


@pytest.mark.parametrize("t,r", [((5, 4), (28, 25)), ((1, 1), (2, 3))])
def test_the_devices_own_tempo_stream_and_joiner_give_the_same_pieces(t, r):
    """independent of the reference: StreamTempo at P / Q, fed into a StreamJoiner(overlap 0, up, down) with the same fp32 taps,
    cut to n_out -- through audio.StreamPitch, a key's last chunk and its empty flush in one push"""
    N, D, L = 64, 8, 20 * 64 + 37
    x = _row(L, 17)
    pl = P.plan(L, t, r, N)
    cuts = [300, 1, 0, 700, L - 1001]
    sp = audio.StreamPitch(2, L, (N, D), device=DEV)
    st = audio.StreamTempo(2, L, (N, D), device=DEV)
    sj = audio.StreamJoiner(2, 4 * (st.history + L) + N, 0, pl["up"], pl["down"], device=DEV)
    try:
        sp.open("k", t, r)
        st.open("k", pl["P"], pl["Q"])
        got, two, at = [], [], 0
        for i, c in enumerate(cuts):
            xd = torch.from_numpy(np.pad(x[at: at + c], (0, L - c), constant_values=np.nan)[None]).to(DEV)
            rows = [("k", c, False)] if i < len(cuts) - 1 else [("k", c, False), ("k", 0, True)]
            xd = xd if len(rows) == 1 else torch.cat([xd, xd])
            o, n = sp.push(xd, rows)
            got += [o[b, : n[b]].cpu().numpy() for b in range(len(rows))]
            for b, row in enumerate(rows):
                z, m = st.push(xd[b: b + 1].contiguous(), [row])
                y, k = sj.push(z.contiguous(), [("k", m[0], row[2])])
                two.append(y[0, : k[0]].cpu().numpy())
            at += c
        got, two = np.concatenate(got), np.concatenate(two)
        assert got.size == pl["n_out"] <= two.size and sp.calls == len(cuts) + 1
        assert np.array_equal(_bits(got), _bits(two[: pl["n_out"]]))
        assert np.array_equal(_bits(got), _bits(_ref(L, 17, t, r, N, D)[0]))
    finally:
        sp.close()
        st.close()
        sj.close()


def test_every_refusal_leaves_state_and_output_untouched():
    N, D, L, t, r = 16, 3, 20 * 16 + 37, (5, 4), (3, 2)
    x = _row(L, 21)
    want, s = _ref(L, 21, t, r, N, D)
    h = Handle(4, 200, N, D, max_taps=401)
    l = h.l
    taps = np.ascontiguousarray(P.taps32(2, 3))
    try:
        wide = np.zeros(321, dtype=np.float32)
        for (slot, tt, rr, tp), name in (((9, t, r, taps), "slot"), ((0, (0, 4), r, taps), "tp"), ((0, (5, 0), r, taps), "tq"),
                                         ((0, t, (0, 2), taps), "rp"), ((0, t, (3, 40000), taps), "rq"), ((0, (4, 1), (1, 4), None), "stretch"),
                                         ((0, t, r, taps[:60]), "n_taps"), ((0, t, r, None), "n_taps"), ((0, t, (7, 7), taps), "n_taps"),
                                         ((0, (1, 1), (2, 3), taps[:5]), "below up"), ((0, t, r, np.zeros(403, np.float32)), "max_taps"),
                                         ((0, (4, 1), (16, 1), wide), "LDS")):
            rc, err = h.raw_open(slot, tt, rr, tp)
            assert rc == EINVAL and name in err, (name, rc, err)
        h.open(0, t, r)
        h.open(2, (1, 1), (2, 3))
        parts = h.push([(0, x[:150], False), (2, x[:90], False)])[:1]
        # an open that is refused changes nothing of a stream that lives
        assert h.raw_open(0, (0, 1), r, taps)[0] == EINVAL
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
        _same(parts, want, s, "after the refusals")
        rc, err, _ = h.raw(xd, [0], [10], [0], 1, out, pos)
        assert rc == EINVAL and "not open" in err               # a stream closes with its last push
    finally:
        h.close()
