"""smi_join_*: the device-side stream joiner through the C ABI, on synthetic chunks, against tests/join_ref.py.

The concatenated pieces of a stream are, bit for bit, ``DeviceAudio.resample_rows`` of the reference-joined waveform (at 1/1 the
reference join itself) and lie within the running-error bound of the float64 direct formula; the same chunks give the same bits
alone or beside other streams, in other slots and rows; everything past a piece is zero; the lengths are the host function's; a
refused call changes nothing and launches nothing."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import join_ref as jr
import resample_ref as rr
from sparkmi import _lib, audio, streaming

pytestmark = pytest.mark.gpu

RATIOS = [(1, 1), (3, 2), (441, 160), (3, 1), (1, 2)]
GARBAGE = 7.5e8
# name -> (overlap n, chunk lengths; the last one is the stream's last chunk)
CASES = {
    "short_last": (5, [12, 10, 10, 7]),        # the last chunk is shorter than 2n; the first push is shorter than every filter's latency
    "single": (5, [37]),
    "empty_last": (0, [30, 25, 0]),            # n = 0: plain concatenation; the empty last chunk flushes the resampler
    "no_overlap": (0, [12, 10, 7]),
    "tiles": (5, [40, 2500, 30]),              # output-tile edges (1024 samples) fall inside the second piece
}


def _signal(seed, n):
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * 0.013 * np.arange(n)) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def _chunks(name):
    n, lengths = CASES[name]
    return n, [_signal(100 * len(name) + i, L) for i, L in enumerate(lengths)]


def _half(up, down):
    return 0 if (up, down) == (1, 1) else 10 * max(up, down)


class _Join:
    def __init__(self, n, up, down, max_streams=4, max_chunk=4096):
        self.l = _lib.lib()
        self.n, self.up, self.down, self.half = n, up, down, _half(up, down)
        taps = np.ascontiguousarray(audio.resample_taps(up, down)) if self.half else np.zeros(1)
        fi, fo = np.ascontiguousarray(np.linspace(0, 1, n)), np.ascontiguousarray(np.linspace(1, 0, n))
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        self.h = C.c_void_p()
        self.l.check(self.l.smi_join_create(max_streams, max_chunk, n, pd(fi), pd(fo), up, down, pd(taps), taps.size, C.byref(self.h)),
                     "smi_join_create")

    def __del__(self):
        self.l.smi_join_destroy(self.h)

    def open(self, slot):
        self.l.check(self.l.smi_join_open(self.h, slot), "smi_join_open")

    def raw_push(self, rows, out_stride=None, B=None):
        """rows [(slot, chunk, last)] in one call: (rc, out [B][out_stride] numpy, n_out)"""
        B = len(rows) if B is None else B
        stride = max(1, max(c.size for _, c, _ in rows))
        x = np.full((len(rows), stride), GARBAGE, np.float32)
        for b, (_, c, _) in enumerate(rows):
            x[b, : c.size] = c
        x = torch.from_numpy(x).cuda()
        # (a piece can exceed its chunk's own resampled length by the filter's latency, which a last push flushes)
        out_stride = out_stride or max(rr.out_len(c.size, self.up, self.down) for _, c, _ in rows) + 2 * self.half // self.down + 2
        y = torch.full((len(rows), out_stride), GARBAGE, dtype=torch.float32, device="cuda")
        i32 = lambda v: (C.c_int32 * len(rows))(*[int(t) for t in v])   # noqa: E731
        got = (C.c_int32 * len(rows))(*([-9] * len(rows)))
        rc = self.l.smi_join_push_rows(self.h, C.c_void_p(x.data_ptr()), stride, i32(s for s, _, _ in rows), i32(c.size for _, c, _ in rows),
                                       i32(last for _, _, last in rows), B, C.c_void_p(y.data_ptr()), out_stride, got, None)
        torch.cuda.synchronize()
        return rc, y.cpu().numpy(), list(got)

    def push(self, rows, out_stride=None):
        rc, y, got = self.raw_push(rows, out_stride)
        self.l.check(rc, "smi_join_push_rows")
        for b in range(len(rows)):
            assert not y[b, got[b]:].any(), f"row {b}: the padding past its piece is not zero"
        return [y[b, : got[b]].copy() for b in range(len(rows))], got


@functools.lru_cache(maxsize=None)
def _device_audio():
    return audio.DeviceAudio("cuda:0")


@functools.lru_cache(maxsize=None)
def _reference(name, up, down):
    """(the reference-joined waveform, its resampling by DeviceAudio.resample_rows): computed once, shared, left unchanged"""
    n, chunks = _chunks(name)
    x = jr.joined(chunks, n)
    if (up, down) == (1, 1):
        return x, x
    y, n_out = _device_audio().resample_rows(torch.from_numpy(x[None]).cuda(), [x.size], [up], [down])
    return x, y.cpu().numpy()[0, : n_out[0]].copy()


def _host_lengths(n, lengths, up, down):
    """piece lengths by sparkmi.streaming.join_piece_len and by the library's smi_join_piece_len, which must agree"""
    l, half, N, K, out = _lib.lib(), _half(up, down), 0, 0, []
    for i, L in enumerate(lengths):
        na, ka = C.c_longlong(), C.c_longlong()
        c_piece = l.smi_join_piece_len(n, up, down, 2 * half + 1, int(i == 0), N, K, L, int(i == len(lengths) - 1), C.byref(na), C.byref(ka))
        piece, N, K = streaming.join_piece_len(n, up, down, half, i == 0, N, K, L, i == len(lengths) - 1)
        assert (c_piece, na.value, ka.value) == (piece, N, K)
        out.append(piece)
    return out


@functools.lru_cache(maxsize=None)
def _solo(name, up, down):
    """the pieces of a case's stream pushed alone: slot 0, row 0, one chunk a call"""
    n, chunks = _chunks(name)
    j = _Join(n, up, down)
    j.open(0)
    pieces, lens = [], []
    for i, c in enumerate(chunks):
        p, got = j.push([(0, c, i == len(chunks) - 1)])
        pieces.append(p[0])
        lens.append(got[0])
    return pieces, lens


@pytest.mark.parametrize("up,down", RATIOS)
@pytest.mark.parametrize("name", list(CASES))
def test_pieces_are_the_resampling_of_the_joined_stream(name, up, down):
    n, chunks = _chunks(name)
    x, want = _reference(name, up, down)
    pieces, lens = _solo(name, up, down)
    assert lens == _host_lengths(n, [c.size for c in chunks], up, down)
    got = np.concatenate(pieces)
    assert got.dtype == np.float32 and got.size == want.size == rr.out_len(x.size, up, down)
    assert x.size == sum(c.size for c in chunks) - n * (len(chunks) - 1)
    assert np.array_equal(got, want), f"{name} at {up}/{down}: {np.count_nonzero(got != want)} samples differ"
    if (up, down) != (1, 1):
        ref, absum, N = rr.direct(x, up, down, audio.resample_taps(up, down))
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err <= rr.bound(absum, N)), f"{name} at {up}/{down}: worst excess {np.max(err - rr.bound(absum, N))}"
    if name == "short_last" and (up, down) != (1, 1):
        assert lens[0] == 0, "7 joined samples are fewer than the filter's latency: the first push emits nothing"
    if name == "empty_last" and (up, down) != (1, 1):
        assert lens[-1] > 0, "the empty last chunk flushes the filter's latency"


@pytest.mark.parametrize("up,down", RATIOS)
def test_same_bits_beside_other_streams_in_other_slots_and_rows(up, down):
    """three streams with n = 5 advance together, their rows in another order every call, in slots 3, 1, 2 of a handle; then one
    of them again in slot 3 right after another stream has used it"""
    names = ["short_last", "single", "tiles"]
    slots = {"short_last": 3, "single": 1, "tiles": 2}
    j = _Join(5, up, down)
    for s in slots.values():
        j.open(s)
    data = {nm: _chunks(nm)[1] for nm in names}
    got = {nm: [] for nm in names}
    for step in range(4):
        rows = [(nm, step) for nm in names if step < len(data[nm])]
        rows = rows[step % len(rows):] + rows[: step % len(rows)]
        pieces, _ = j.push([(slots[nm], data[nm][i], i == len(data[nm]) - 1) for nm, i in rows], out_stride=7600 + step)
        for (nm, _), p in zip(rows, pieces):
            got[nm].append(p)
    j.open(3)                                    # a slot is used again: nothing of its last stream is left
    for i, c in enumerate(data["tiles"]):
        got.setdefault("again", []).append(j.push([(3, c, i == 2)])[0][0])
    for nm in names + ["again"]:
        solo = _solo("tiles" if nm == "again" else nm, up, down)[0]
        assert len(got[nm]) == len(solo)
        for i, (a, b) in enumerate(zip(got[nm], solo)):
            assert np.array_equal(a, b), f"{nm} push {i} at {up}/{down}"


def test_refusals_change_nothing_and_launch_nothing():
    up, down, n = 3, 2, 5
    _, chunks = _chunks("short_last")
    solo = _solo("short_last", up, down)[0]
    j = _Join(n, up, down)
    j.open(0)
    j.open(1)
    first, _ = j.push([(0, chunks[0], False)])
    assert np.array_equal(first[0], solo[0])
    ok = _signal(1, 12)
    bad_calls = [
        ([(0, chunks[1], False), (1, ok, False), (0, chunks[2], False)], None, b"stream[2]"),      # a stream twice in a call
        ([(1, ok, False), (0, _signal(2, 2 * n - 1), False)], None, b"len[1]"),                     # L < 2n, not the last chunk
        ([(0, chunks[1], False), (4, ok, False)], None, b"stream[1]"),                              # a slot the handle has not
        ([(0, chunks[1], False), (-1, ok, False)], None, b"stream[1]"),
        ([(0, chunks[1], False), (2, ok, False)], None, b"not open"),                               # a slot never opened
        ([(0, chunks[1], False)], 65, b"B=65"),                                                      # more rows than a call takes
        ([(0, _signal(3, n - 1), True)], None, b"len[0]"),                                          # a last chunk below n
    ]
    for rows, B, word in bad_calls:
        rc, y, got = j.raw_push(rows, B=B)
        assert rc == -1 and word in j.l.smi_last_error(), (word, j.l.smi_last_error())
        assert np.all(y == np.float32(GARBAGE)) and got == [-9] * len(rows), f"{word}: something was written"
    # the refused calls changed no counter and no state: both streams go on with the bits of their solo runs
    for i in (1, 2, 3):
        rows = [(0, chunks[i], i == 3)] + ([(1, ok, False)] if i == 1 else [])
        pieces, _ = j.push(rows)
        assert np.array_equal(pieces[0], solo[i]), f"push {i} after the refusals"
    rc, _, _ = j.raw_push([(0, chunks[0], False)])
    assert rc == -1 and b"not open" in j.l.smi_last_error()            # a stream closes with its last chunk


def test_a_stream_up_to_2_31_and_its_refusal_beyond():
    """Indices are 32-bit: at 441/160 a stream may hold 4.8 M samples (N up = 2.117e9 < 2^31 = 2.147e9) and its bits near that end
    are still those of the whole-stream resampler; the push that would pass 2^31 is refused by name and launches nothing."""
    up, down = 441, 160
    x = _signal(77, 4_800_000)
    j = _Join(0, up, down, max_streams=1, max_chunk=4_000_000)
    j.open(0)
    first, _ = j.push([(0, x[:4_000_000], False)])
    rc, y, got = j.raw_push([(0, x[:1_000_000], False)], out_stride=16)
    assert rc == -1 and b"2^31" in j.l.smi_last_error() and np.all(y == np.float32(GARBAGE)) and got == [-9]
    rest, _ = j.push([(0, x[4_000_000:], True)])
    want, n_out = _device_audio().resample_rows(torch.from_numpy(x[None]).cuda(), [x.size], [up], [down])
    want = want.cpu().numpy()[0, : n_out[0]]
    got = np.concatenate([first[0], rest[0]])
    assert got.size == want.size == rr.out_len(x.size, up, down) and np.array_equal(got, want)
