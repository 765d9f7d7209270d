"""The k_attn_pf2 tiles of a prompt pass's row group (``smi_llm_pf_tiles`` of libsparkmi_diag.so: the helper ``prefill_prompts``
builds its tile list with, host only, no GPU call): runs of up to 16 rows that are consecutive positions of one KV slot.  Checked
as properties on random plans and on the row groups of tests/test_llm_prefill_ops_gpu.py, and against one hand-written list."""
import ctypes as C

import numpy as np
import pytest

# the row groups of tests/test_llm_prefill_ops_gpu.py: (first position, rows) per sequence
OP_CASES = [[(0, 65)], [(0, 127)], [(0, 70), (0, 65), (0, 96)], [(0, 257), (0, 255)], [(0, 257), (0, 256)], [(0, 689)],
            [(651, 38)], [(651, 38), (0, 300)]]


def _rows(plan, slots=None):
    """(M, 2) (slot, pos) rows of a plan of (first position, rows) sequences, sequence b in slots[b] (default: b)."""
    out = []
    for b, (p0, n) in enumerate(plan):
        s = b if slots is None else slots[b]
        out += [(s, p0 + t) for t in range(n)]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def _tiles(rows, cap=None):
    from sparkmi import _lib
    d = _lib.diag()
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    M = rows.shape[0]
    cap = M if cap is None else cap
    out = np.full((max(cap, 1), 4), -1, dtype=np.int32)
    n = C.c_int32(-1)
    ip = C.POINTER(C.c_int32)
    d.check(d.smi_llm_pf_tiles(rows.ctypes.data_as(ip), M, out.ctypes.data_as(ip), cap, C.byref(n)), "smi_llm_pf_tiles")
    return out[: min(n.value, cap)], n.value


def _check(rows):
    tiles, n = _tiles(rows)
    M = rows.shape[0]
    assert n == len(tiles)
    nxt = 0
    for i, (m0, cnt, slot, pos0) in enumerate(tiles.tolist()):
        assert m0 == nxt and 1 <= cnt <= 16, f"tile {i}: rows {m0} .. +{cnt} after row {nxt}"       # a partition, in order
        assert (rows[m0: m0 + cnt, 0] == slot).all(), f"tile {i} crosses a slot"
        assert (rows[m0: m0 + cnt, 1] == pos0 + np.arange(cnt)).all(), f"tile {i}: positions not consecutive from {pos0}"
        nxt = m0 + cnt
        if cnt < 16 and nxt < M:    # ended early: the next row starts another run
            assert rows[nxt, 0] != slot or rows[nxt, 1] != pos0 + cnt, f"tile {i} of {cnt} rows ends inside a run"
    assert nxt == M
    return tiles


@pytest.mark.parametrize("plan", OP_CASES, ids=lambda p: "+".join(f"{a}:{n}" for a, n in p))
def test_tiles_of_the_op_test_row_groups(plan):
    tiles = _check(_rows(plan))
    assert len(tiles) == sum((n + 15) // 16 for _, n in plan)


def test_tiles_of_random_plans():
    rng = np.random.default_rng(20240)
    for it in range(200):
        nseq = int(rng.integers(1, 7))
        lens = [int(rng.integers(1, 701)) if it % 4 else int(rng.integers(1, 40)) for _ in range(nseq)]
        plan = [(int(rng.integers(0, 900)) if rng.random() < 0.4 else 0, n) for n in lens]
        slots = rng.permutation(64)[:nseq].tolist()
        tiles = _check(_rows(plan, slots))
        assert len(tiles) == sum((n + 15) // 16 for n in lens)


def test_tiles_break_where_rows_are_not_consecutive():
    """Rows of one slot that skip or repeat a position, and two sequences whose positions happen to continue across the slot
    boundary, start new tiles; an empty row list gives no tile; cap limits what is written, not what is counted."""
    rows = np.array([(2, 5), (2, 6), (2, 8), (2, 8), (3, 9), (3, 10)], dtype=np.int32)
    assert _check(rows).tolist() == [[0, 2, 2, 5], [2, 1, 2, 8], [3, 1, 2, 8], [4, 2, 3, 9]]
    assert _tiles(np.zeros((0, 2), dtype=np.int32))[1] == 0
    few, n = _tiles(_rows([(0, 100)]), cap=3)
    assert n == 7 and few.tolist() == [[0, 16, 0, 0], [16, 16, 0, 16], [32, 16, 0, 32]]


def test_tiles_of_three_sequences_by_hand():
    """70 + 65 + 96 rows in slots 3, 0, 6: tiles break mid-16 at the sequence boundaries (rows 70 and 135)."""
    want = [[0, 16, 3, 0], [16, 16, 3, 16], [32, 16, 3, 32], [48, 16, 3, 48], [64, 6, 3, 64],
            [70, 16, 0, 0], [86, 16, 0, 16], [102, 16, 0, 32], [118, 16, 0, 48], [134, 1, 0, 64],
            [135, 16, 6, 0], [151, 16, 6, 16], [167, 16, 6, 32], [183, 16, 6, 48], [199, 16, 6, 64], [215, 16, 6, 80]]
    assert _check(_rows([(0, 70), (0, 65), (0, 96)], [3, 0, 6])).tolist() == want
