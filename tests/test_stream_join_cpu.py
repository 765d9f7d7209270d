"""The stream joiner's host side (sparkmi/streaming.py: join_piece_len, join_history, split_calls; sparkmi/audio.py: StreamJoiner
with a stand-in library) against tests/join_ref.py: piece lengths, the history bound, the join's agreement with
``streaming.crossfade`` and its two documented deviations, the slot bookkeeping, and the wrong variants a bit comparison must
reject.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import join_ref as jr
import resample_ref as rr
from sparkmi import audio, streaming

# 16 kHz -> 8, 22.05, 24, 44.1, 48 kHz, and the model's own rate
RATIOS = [rr.ratio(16000, r) for r in (8000, 22050, 24000, 44100, 48000, 16000)]


def _half(up, down):
    return 0 if (up, down) == (1, 1) else 10 * max(up, down)


def _signal(seed, n):
    rng = np.random.default_rng(seed)
    return (0.3 * np.sin(2 * np.pi * 0.013 * np.arange(n)) + 0.1 * rng.standard_normal(n)).astype(np.float32)


def _chain(lengths, n, up, down):
    """piece lengths of a stream through join_piece_len, with the counters after every push"""
    half, N, K, out = _half(up, down), 0, 0, []
    for i, L in enumerate(lengths):
        piece, N, K = streaming.join_piece_len(n, up, down, half, i == 0, N, K, L, i == len(lengths) - 1)
        out.append((piece, N, K))
    return out


@pytest.mark.parametrize("up,down", RATIOS)
def test_piece_lengths_against_the_definition(up, down):
    rng = np.random.default_rng(up * 1000 + down)
    half, zero_pieces = _half(up, down), 0
    for trial in range(40):
        n = int(rng.choice([0, 1, 5, 32]))
        m = int(rng.integers(1, 9))
        total = n * m + int(rng.integers(0, 400))
        lengths = jr.random_cuts(rng, total, n, m)
        got = _chain(lengths, n, up, down)
        Ns = jr.joined_lengths(lengths, n)
        k_prev = 0
        for i, ((piece, N, K), N_ref) in enumerate(zip(got, Ns)):
            k_ref = jr.emitted(N_ref, up, down, half, i == m - 1)
            assert (N, K, piece) == (N_ref, k_ref, k_ref - k_prev), (lengths, n, i)
            zero_pieces += piece == 0
            k_prev = k_ref
        assert sum(p for p, _, _ in got) == rr.out_len(total, up, down) == audio.out_len(total, up, down)
        assert Ns[-1] == total == sum(lengths) - n * (m - 1)
    assert zero_pieces > 0, "no push that emits nothing among the cuts"


def test_piece_len_of_the_library_is_the_python_twin():
    from sparkmi import _lib
    l = _lib.lib()
    rng = np.random.default_rng(5)
    for up, down in RATIOS:
        half = _half(up, down)
        for trial in range(50):
            n = int(rng.choice([0, 3, 64]))
            first, last = bool(rng.integers(2)), bool(rng.integers(2))
            N, L = int(rng.integers(0, 5000)), int(rng.integers(0, 400))
            K = jr.emitted(N, up, down, half, False)
            na, ka = C.c_longlong(-7), C.c_longlong(-7)
            got = l.smi_join_piece_len(n, up, down, 2 * half + 1, int(first), N, K, L, int(last), C.byref(na), C.byref(ka))
            try:
                want = streaming.join_piece_len(n, up, down, half, first, N, K, L, last)
            except ValueError:
                assert got == -1
                continue
            assert (got, na.value, ka.value) == want


@pytest.mark.parametrize("up,down", RATIOS[:5])
def test_history_bound_holds(up, down):
    rng = np.random.default_rng(up + 7 * down)
    half = _half(up, down)
    bound = streaming.join_history(up, down, half)
    assert bound == -((-(2 * half + down)) // up) + 1
    worst = 0
    for trial in range(200):
        n = int(rng.choice([0, 5]))
        m = int(rng.integers(2, 12))
        lengths = jr.random_cuts(rng, n * m + int(rng.integers(0, 600)), n, m)
        used = jr.history_used(lengths, n, up, down, half)
        worst = max([worst] + used)
    assert 0 < worst <= bound, (worst, bound)
    assert streaming.join_history(1, 1, 0) == 0


def test_joined_reference_is_crossfade_where_every_chunk_has_two_overlaps():
    rng = np.random.default_rng(3)
    for n, lengths in ((5, [12, 10, 10, 11]), (32, [64, 64, 100]), (1, [2, 2, 2, 2]), (1600, [8000, 16000, 3200])):
        chunks = [_signal(int(rng.integers(1 << 30)), L) for L in lengths]
        want = streaming.crossfade(chunks, n).astype(np.float32)
        got = jr.joined(chunks, n)
        assert got.dtype == np.float32 and got.size == sum(lengths) - n * (len(lengths) - 1)
        assert np.array_equal(got, want)
    one = _signal(1, 40)
    assert np.array_equal(jr.joined([one], 5), streaming.crossfade([one], 5))


def test_the_two_documented_deviations_from_crossfade():
    a, b, c = _signal(1, 12), _signal(2, 10), _signal(3, 7)
    # n = 0: plain concatenation, where crossfade's slices degenerate (chunks[0][:-0] is empty, chunks[i - 1][-0:] a whole chunk)
    cat = jr.joined([a, b, c], 0)
    assert np.array_equal(cat, np.concatenate([a, b, c]))
    with pytest.raises(ValueError):
        streaming.crossfade([a, b, c], 0)
    # a last chunk with n <= L < 2n: the table's rule gives sum L - n (m - 1) samples; crossfade repeats samples there
    n = 5
    got = jr.joined([a, b, c], n)
    assert got.size == 12 + 10 + 7 - 2 * n
    assert np.array_equal(got[-2:], c[n:]) and np.array_equal(got[: 12 - n], a[: 12 - n])
    cf = streaming.crossfade([a, b, c], n)
    assert cf.size == got.size + (2 * n - c.size) and np.array_equal(cf[-n:], c[-n:])
    # the lengths the rules refuse
    with pytest.raises(ValueError):
        streaming.join_piece_len(n, 1, 1, 0, False, 20, 20, 2 * n - 1, False)
    with pytest.raises(ValueError):
        streaming.join_piece_len(n, 1, 1, 0, False, 20, 20, n - 1, True)
    assert streaming.join_piece_len(n, 1, 1, 0, True, 0, 0, 0, True) == (0, 0, 0)      # an empty only chunk
    assert streaming.join_piece_len(0, 3, 2, 30, False, 100, 135, 0, True) == (15, 100, 150)   # an empty last chunk flushes


def test_wrong_variants_are_rejected_by_the_bit_comparison():
    n, lengths = 5, [12, 10, 10, 7]
    chunks = [_signal(10 + i, L) for i, L in enumerate(lengths)]
    good = jr.joined(chunks, n)
    assert not np.array_equal(jr.joined(chunks, n, swap_fades=True), good)
    assert not np.array_equal(jr.joined(chunks, n, tail_shift=1), good)
    assert jr.joined(chunks, n, swap_fades=True).size == jr.joined(chunks, n, tail_shift=1).size == good.size
    chunks = [_signal(20 + i, L) for i, L in enumerate([90, 75, 61, 140, 33])]
    for up, down in RATIOS[:5]:
        h = audio.resample_taps(up, down)
        whole = rr.emulate_fp32(jr.joined(chunks, n), up, down, h)
        good = np.concatenate(jr.pieces(chunks, n, up, down, h))
        assert np.array_equal(good, whole), "the streaming emission is the whole stream's resampling"
        for wrong in (dict(early=1), dict(short=1)):
            bad = np.concatenate(jr.pieces(chunks, n, up, down, h, **wrong))
            assert bad.size == whole.size and not np.array_equal(bad, whole), (up, down, wrong)


def test_split_calls():
    assert streaming.split_calls([]) == []
    assert streaming.split_calls([1, 2, 3]) == [(0, 3)]
    assert streaming.split_calls([1, 2, 2, 3]) == [(0, 2), (2, 4)]            # a request's last full chunk and its flush
    assert streaming.split_calls([4, 4, 4]) == [(0, 1), (1, 2), (2, 3)]
    assert streaming.split_calls(list(range(130))) == [(0, 64), (64, 128), (128, 130)]
    assert streaming.split_calls([0, 1, 0, 1], max_rows=8) == [(0, 2), (2, 4)]


class _FakeLib:
    """records what StreamJoiner sends to the library"""

    def __init__(self):
        self.created, self.opened, self.pushes, self.destroyed = [], [], [], 0

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_join_create(self, max_streams, max_chunk, overlap, fi, fo, up, down, taps, n_taps, href):
        self.created.append((max_streams, max_chunk, overlap, up, down, n_taps))
        href._obj.value = 1234
        return 0

    def smi_join_destroy(self, h):
        self.destroyed += 1
        return 0

    def smi_join_open(self, h, slot):
        self.opened.append(slot)
        return 0

    def smi_join_push_rows(self, h, src, stride, streams, lens, lasts, B, dst, out_stride, n_out, stream):
        assert len(set(streams[:B])) == B, "a stream twice in one call"
        self.pushes.append((list(streams[:B]), list(lens[:B]), list(lasts[:B]), out_stride))
        return 0


def test_stream_joiner_slots_with_a_stand_in_library():
    fake = _FakeLib()
    j = audio.StreamJoiner(3, 4000, 5, 3, 2, lib=fake)
    assert fake.created == [(3, 4000, 5, 3, 2, 61)] and j.history == streaming.join_history(3, 2, 30) == 22
    _, lens = j.push(None, [("a", 12, False), ("b", 30, False), ("c", 40, True)])
    assert fake.opened == [0, 1, 2] and j.calls == 1
    assert lens == [streaming.join_piece_len(5, 3, 2, 30, True, 0, 0, L, last)[0] for L, last in ((12, False), (30, False), (40, True))]
    assert lens[0] == 0 and lens[2] == 60          # 7 samples are fewer than the filter's latency; an only chunk comes out whole
    assert j.slot("c") is None and j.slot("a") == 0 and j.slot("b") == 1
    # a's last full chunk and its flush in one poll: two calls; its slot and c's are free afterwards and are used again
    _, lens = j.push(None, [("a", 10, False), ("a", 7, True), ("b", 10, False), ("d", 12, False)])
    assert j.calls == 3 and [p[0] for p in fake.pushes[1:]] == [[0], [0, 1, 2]]
    assert sum(lens[:2]) == rr.out_len(12 + 10 + 7 - 2 * 5, 3, 2)
    assert fake.opened == [0, 1, 2, 2] and j.slot("a") is None and j.slot("d") == 2
    j.push(None, [("e", 12, False)])
    assert j.slot("e") == 0
    with pytest.raises(ValueError):
        j.push(None, [("f", 12, False)])           # a fourth open request: beyond the bound the caller stated
    with pytest.raises(ValueError):
        j.push(None, [("b", 9, False)])            # L < 2n on a chunk that is not the last: refused before the library is called
    assert j.calls == 4
    j.reset()
    assert j.slot("b") is None and j.open("g") == 0
    j.close()
    assert fake.destroyed == 1


def test_slots_cannot_run_out_at_the_stated_bound():
    """serve_stream's sizing: at most max(max_open, max_batch) requests are between their admission and their last chunk's
    push, so that many slots never run out, whatever the order in which the requests speak and end"""
    rng = np.random.default_rng(9)
    bound = 5
    fake = _FakeLib()
    j = audio.StreamJoiner(bound, 4000, 5, lib=fake)
    left, nxt, peak = {}, 0, 0         # open request -> chunks it still has to push
    for poll in range(300):
        while len(left) < bound and rng.random() < 0.7:
            left[nxt] = int(rng.integers(1, 5))
            nxt += 1
        rows = []
        for key in list(left):
            for _ in range(int(rng.integers(0, 3))):
                if key in left:
                    left[key] -= 1
                    rows.append((key, 40, left[key] == 0))
                    if left[key] == 0:
                        del left[key]
        if rows:
            j.push(None, rows)
        peak = max(peak, bound - len(j._free))
    assert peak == bound and nxt > 100 and j.calls > 100
