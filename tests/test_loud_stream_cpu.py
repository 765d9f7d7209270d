"""Loudness of joined streams, host side (tests/loud_stream_ref.py; smi_louds_piece_len; sparkmi/streaming.py:
loudness_piece_len): the emission arithmetic, the knot rules of include/sparkmi.h on signals that reach each of them, the
device's order of operations against the longdouble result over the committed cases -- the measurement behind the GPU
tolerance --, that no committed case decides a branch within 1e-6, and that the tolerance rejects wrong
readings of the definition.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import loud_ref as LR
import loud_stream_ref as S
from sparkmi import streaming

BLOCKS = [64, 400, 6400]


def _cuts(rng, total, m):
    at = np.sort(rng.integers(0, total + 1, size=m - 1))
    return np.diff(np.concatenate([[0], at, [total]])).astype(int).tolist()


@pytest.mark.parametrize("block", BLOCKS)
def test_piece_lengths_against_the_reference_and_the_library(block):
    from sparkmi import _lib
    l = _lib.lib()
    hop = block // 4
    rng = np.random.default_rng(block)
    zero_pieces = 0
    for trial in range(40):
        total = int(rng.integers(0, 30 * hop + 17))
        cuts = _cuts(rng, total, int(rng.integers(1, 14)))
        n = out = 0
        for i, c in enumerate(cuts):
            last = i == len(cuts) - 1
            piece, n1, k1 = S.piece_len(block, n, c, last)
            assert streaming.loudness_piece_len(block, n, c, last) == (piece, n1, k1)
            na, ka = C.c_longlong(-7), C.c_longlong(-7)
            assert l.smi_louds_piece_len(block, n, c, int(last), C.byref(na), C.byref(ka)) == piece
            assert (na.value, ka.value) == (n1, k1)
            # hop j leaves once n >= (j + 5) hop, and no later
            assert last or (piece % hop == 0 and (out + piece == 0 or out + piece + 4 * hop <= n1) and n1 < out + piece + 5 * hop)
            zero_pieces += piece == 0 and c > 0
            n, out = n1, out + piece
        assert out == total                                  # the stage delays pieces and keeps the total
    assert zero_pieces > 0
    for L in (0, 1, hop - 1, hop, 5 * hop - 1, 5 * hop):     # single pushes
        assert S.piece_len(block, 0, L, False)[0] == (hop if L == 5 * hop else 0)
        assert S.piece_len(block, 0, L, True) == (L, L, (L - 1) // hop + 2 if L else 0)
        assert l.smi_louds_piece_len(block, 0, L, 1, None, None) == L
    assert l.smi_louds_piece_len(block + 1, 0, 10, 0, None, None) == -1
    assert l.smi_louds_piece_len(block, -1, 10, 0, None, None) == -1
    assert l.smi_louds_piece_len(block, 0, 10, 2, None, None) == -1
    for bad in ((block + 1, 0, 10, False), (block, -1, 10, False), (block, 0, -1, True)):
        with pytest.raises(ValueError):
            streaming.loudness_piece_len(*bad)


def test_final_loudness_of_the_device_order_is_the_batch_emulation_bit_for_bit():
    for c in S.reference():
        d = S.stream(c["x"], c["coef"], c["block"], c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"], device=True)
        assert d["loudness"] == LR.emulate(c["x"], c["coef"], c["block"]), c["name"]
        want = LR.loudness(c["x"], c["coef"], c["block"], np.longdouble)
        # (the definition sums hop by hop, loud_ref's short-span rule sample by sample: roundings of the longdouble sums apart)
        assert c["ref"]["loudness"] == want or abs(float(c["ref"]["loudness"] - want)) < 1e-15, c["name"]


def _run(name, **kw):
    c = S.case(name)
    a = dict(target=c["target"], max_gain_db=c["max_gain_db"], ceiling=c["ceiling"], max_slew_db=c["max_slew_db"])
    a.update(kw)
    return c, S.stream(c["x"], c["coef"], c["block"], **a)


def test_hold_on_a_silent_lead_in():
    c, r = _run("b64_talk")
    hop = c["block"] // 4
    silent = 400 // hop - 3                     # blocks that lie in the 400 silent samples
    assert silent >= 5
    assert all(f == S.F_HOLD and g == 1.0 for g, f in zip(r["G"][:silent], r["flags"][:silent]))
    assert not r["flags"][silent + 4] & S.F_HOLD


def test_slew_binds_up_and_down():
    c, r = _run("b64_talk")
    up, dn = S.slew_factors(c["max_slew_db"])
    G, F = r["G"], r["flags"]
    ups = [j for j in range(1, len(G)) if F[j] & S.F_SLEW and G[j] == G[j - 1] * up]
    dns = [j for j in range(1, len(G)) if F[j] & S.F_SLEW and G[j] == G[j - 1] * dn]
    assert len(ups) >= 3 and len(dns) >= 3
    for j in range(1, len(G)):                  # no knot moves faster than the slew rate unless the ceiling pulls it down
        assert G[j] <= G[j - 1] * up
        assert G[j] >= G[j - 1] * dn or F[j] & S.F_CEILING


def test_the_ceiling_wins_after_the_slew_step_and_bounds_every_sample():
    c, r = _run("b64_click")
    hop = c["block"] // 4
    j = 1203 // hop
    G, F = r["G"], r["flags"]
    up, dn = S.slew_factors(c["max_slew_db"])
    for k in (j, j + 1):                        # the two knots whose hops hold the click
        assert F[k] & S.F_CEILING and G[k] == c["ceiling"] / float(np.abs(c["x"][max(0, (k - 1) * hop): (k + 1) * hop]).max())
    assert G[j] < G[j - 1] * dn                 # the ceiling pulled it below the slew bound
    assert F[j + 2] & S.F_SLEW and G[j + 2] == G[j + 1] * up   # and the gain comes back at the slew rate
    y = S.apply(c["x"], G, hop)
    assert float(np.abs(y).max()) <= c["ceiling"] * (1 + 2.0 ** -23)
    assert float(np.abs(y).max()) > 0.99 * c["ceiling"]
    for name in ("b64_talk", "b400_talk", "real_3s"):
        cc = S.case(name)
        assert float(np.abs(cc["y"]).max()) <= cc["ceiling"] * (1 + 2.0 ** -23)


def test_nan_target_is_the_identity():
    c, r = _run("b64_measure_only")
    assert all(g == 1.0 for g in r["G"]) and not any(r["flags"])
    assert np.array_equal(S.apply(c["x"], r["G"], c["block"] // 4).view(np.uint32), c["x"].view(np.uint32))
    assert math.isfinite(float(r["loudness"]))


@pytest.mark.parametrize("block", [64, 400])
def test_shorter_than_a_block(block):
    hop = block // 4
    c, r = _run(f"b{block}_len{block - 1}")
    L = block - 1
    loud = r["loudness"]
    assert abs(loud - LR.loudness(c["x"], c["coef"], block)) < 1e-13   # (hop by hop here, sample by sample there)
    A = 10.0 ** ((c["target"] - loud) / 20.0)
    assert len(r["G"]) == (L - 1) // hop + 2 and r["G"][0] == A and not any(r["flags"])
    assert all(abs(g / A - 1) < 1e-15 for g in r["G"])
    c, r = _run("b64_len1")
    assert len(r["G"]) == 2
    x0 = np.zeros(7, dtype=np.float32)
    r = S.stream(x0, c["coef"], 64, -23.0)
    assert r["G"] == [1.0, 1.0] and r["flags"] == [S.F_HOLD, S.F_HOLD] and r["loudness"] == -math.inf


def _device_all():
    out = []
    for c in S.reference():
        m = dict(gate=math.inf, bound=math.inf)
        d = S.stream(c["x"], c["coef"], c["block"], c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"], device=True, margins=m)
        out.append((c, d, m))
    return out


def test_the_device_order_against_longdouble_and_no_case_near_a_branch():
    """Measured here over the committed cases: the largest knot-gain difference 3.8e-14 relative and the
    largest running-loudness difference 3.3e-13 LU, both inside loud_ref's EMU_GAIN = 1.2e-13 and EMU_LU = 1e-12, so the running
    order needs no larger constants.  No block lies within 1e-6 relative of a gate and no knot within 1e-6 of a bound it is
    compared with: the device and the reference cannot decide a branch differently."""
    worst_g = worst_i = 0.0
    flags_seen = 0
    for c, d, m in _device_all():
        r = c["ref"]
        assert d["flags"] == r["flags"], c["name"]
        assert len(d["G"]) == len(r["G"]) == ((len(c["x"]) - 1) // (c["block"] // 4) + 2 if len(c["x"]) else 0)
        for a, b in zip(d["G"], r["G"]):
            worst_g = max(worst_g, abs(float(a / b - 1)))
        for a, b in zip(d["I"], r["I"]):
            assert math.isfinite(float(a)) == math.isfinite(float(b))
            if math.isfinite(float(b)):
                worst_i = max(worst_i, abs(float(a - b)))
        assert m["gate"] > 1e-6 and m["bound"] > 1e-6, (c["name"], m)
        for f in r["flags"]:
            flags_seen |= f
    print(f"device order vs longdouble: gain {worst_g:.3e} relative, loudness {worst_i:.3e} LU")
    assert worst_g <= LR.EMU_GAIN and worst_i <= LR.EMU_LU
    assert flags_seen == 15                     # every rule binds somewhere among the cases


@pytest.mark.parametrize("variant,name,factor", [("early", "b64_talk", 1e6), ("peak1", "b64_click", 1e6),
                                                 ("slew_after_peak", "b64_click", 1e6), ("rel30", "b64_talk", 1e6)])
def test_the_tolerance_rejects_wrong_readings(variant, name, factor):
    """every wrong variant moves a knot gain by more than 1e6 times the tolerance (measured: 1e10 and more)"""
    c, w = _run(name, variant=variant)
    r = S.stream(c["x"], c["coef"], c["block"], c["target"], c["max_gain_db"], c["ceiling"], c["max_slew_db"])
    worst = max(abs(float(a / b - 1)) for a, b in zip(w["G"], r["G"]))
    print(f"{variant}: largest knot-gain difference {worst:.3e} = {worst / S.TOL_GAIN:.1e} tolerances")
    assert worst > factor * S.TOL_GAIN


class _FakeLib:
    """a stand-in for the library: it fills the pieces' lengths with the reference's arithmetic and records the calls"""

    def __init__(self, block):
        self.block, self.n, self.opened, self.pushes = block, {}, [], []

    def check(self, rc, what=""):
        assert rc == 0, what

    def smi_louds_create(self, max_streams, max_chunk, block, coef, max_blocks, out):
        assert block == self.block and max_blocks >= 1
        return 0

    def smi_louds_destroy(self, h):
        return 0

    def smi_louds_open(self, h, slot, target, max_gain_db, ceiling, max_slew_db):
        self.n[slot] = 0
        self.opened.append((slot, target))
        return 0

    def smi_louds_push_rows(self, h, src, stride, slots, lens, lasts, B, gain, gstride, dst, ostride, got, stats, stream):
        assert len(set(slots[:B])) == B          # a stream at most once in a call
        for b in range(B):
            got[b], self.n[slots[b]], _ = S.piece_len(self.block, self.n[slots[b]], lens[b], lasts[b])
        self.pushes.append([(slots[b], lens[b], lasts[b]) for b in range(B)])
        return 0


def test_stream_loudness_bookkeeping_with_a_stand_in_library():
    from sparkmi import audio
    fake = _FakeLib(64)
    sl = audio.StreamLoudness(2, 500, block=64, coef=np.zeros(10), max_blocks=100, lib=fake)
    sl.open("a", -23.0)
    with pytest.raises(ValueError, match="already open"):
        sl.open("a", -20.0)
    assert sl.piece_lengths([("a", 100, False), ("b", 79, False), ("a", 0, True)]) == [32, 0, 68]
    out, lens = sl.push(None, [("a", 100, False), ("b", 79, False), ("a", 0, True)])      # "a" twice: two device calls
    assert lens == [32, 0, 68] and sl.calls == 2 and fake.pushes == [[(0, 100, 0), (1, 79, 0)], [(0, 0, 1)]]
    assert math.isnan(fake.opened[1][1])         # a key met unopened measures and copies
    assert sl.slot("a") is None and sl.slot("b") == 1
    sl.open("c", -23.0)                          # slot 0 is free again
    assert sl.slot("c") == 0
    with pytest.raises(ValueError, match="slots are in use"):
        sl.open("d")
    with pytest.raises(ValueError, match="max_chunk"):
        sl.push(None, [("b", 501, False)])
    assert sl.push(None, [("b", 1, True)])[1] == [80]
    sl.reset()
    assert sl.slot("c") is None and sorted(sl._free) == [0, 1]
