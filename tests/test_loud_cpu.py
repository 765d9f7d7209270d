"""Output loudness on the host: the coefficient design, the standard's check signal, the restatement in tests/loud_ref.py
against scipy, the tolerance the GPU tests use (derived here from the device's order of operations emulated in float64), the
wrong variants that tolerance must reject, and the distance of every block from the gates."""
import math

import numpy as np
import pytest

import loud_ref as R
from sparkmi import audio

TABLE_48K = [1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
             1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]


def test_k_weighting_reproduces_the_standards_table_at_48k():
    got = audio.k_weighting(48000)
    assert got.dtype == np.float64 and got.shape == (10,)
    assert np.max(np.abs(got - np.array(TABLE_48K))) <= 5e-14


def test_k_weighting_other_rates_and_bad_ones():
    for sr in (16000, 24000, 44100):
        c = audio.k_weighting(sr)
        assert np.all(np.isfinite(c)) and c[5:8].tolist() == [1.0, -2.0, 1.0]
        # both stages are stable: poles inside the unit circle
        for a1, a2 in ((c[3], c[4]), (c[8], c[9])):
            assert abs(a2) < 1 and abs(a1) < 1 + a2
    for bad in (0, -16000, 3000):
        with pytest.raises(ValueError):
            audio.k_weighting(bad)


def test_loudness_block_is_four_whole_hops():
    assert audio.loudness_block(16000) == 6400 and audio.loudness_block(48000) == 19200 and audio.loudness_block(44100) == 17640
    assert audio.loudness_block(22050) % 4 == 0


def test_full_scale_997_hz_sine_reads_minus_3_01_lufs():
    x = np.sin(2 * np.pi * 997.0 * np.arange(3 * 48000) / 48000.0).astype(np.float32)
    got = float(R.loudness(x, audio.k_weighting(48000), audio.loudness_block(48000)))
    print("997 Hz, full scale, 3 s at 48 kHz:", got)
    assert abs(got - (-3.01)) <= 0.005


def test_scipy_lfilter_agrees_with_the_recurrence():
    signal = pytest.importorskip("scipy.signal")
    for c in R.reference():
        if not 0 < c["x"].size <= 10000:
            continue
        coef = c["coef"]
        y = signal.lfilter(coef[0:3], [1.0, coef[3], coef[4]], c["x"].astype(np.float64))
        y = signal.lfilter(coef[5:8], [1.0, coef[8], coef[9]], y)
        mine = np.array(R.kfilter(c["x"], coef))
        assert np.max(np.abs(mine - y)) <= 1e-9 * max(1.0, float(np.max(np.abs(y)))), c["name"]


def test_gpu_tolerance_is_the_emulations_distance_from_longdouble():
    """the device's order of operations, emulated in float64, against the longdouble restatement over every committed case"""
    d_lu, d_gain = 0.0, 0.0
    for c in R.reference():
        emu = R.emulate(c["x"], c["coef"], c["block"])
        if c["loudness"] == -math.inf:
            assert emu == -math.inf, c["name"]
            continue
        g, limit = R.gain(emu, c["peak"], c["target"], c["max_gain_db"], c["ceiling"])
        assert limit == c["limit"], c["name"]
        d_lu = max(d_lu, float(abs(np.longdouble(emu) - c["loudness"])))
        d_gain = max(d_gain, float(abs(np.longdouble(g) / c["gain"] - 1)))
    print(f"largest |emulation - longdouble|: {d_lu:.3e} LU, {d_gain:.3e} relative gain")
    assert d_lu <= R.EMU_LU and d_gain <= R.EMU_GAIN
    assert R.TOL_LU == R.EMU_LU * R.MARGIN and R.TOL_GAIN == R.EMU_GAIN * R.MARGIN


def _a2_off(coef):
    c = np.array(coef, dtype=np.float64)
    c[9] += 1e-6
    return c


VARIANTS = {
    "50 % block overlap": dict(hops=2),
    "relative gate at -8 LU": dict(rel=-8.0),
    "no absolute gate": dict(use_abs=False),
    "the tail hop included": dict(tail=True),
    "a2 of stage 2 off by 1e-6": dict(coef=_a2_off),
    "offset -0.691 dropped": dict(offset=0.0),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_the_tolerance_rejects_wrong_variants(name):
    kw = dict(VARIANTS[name])
    bend = kw.pop("coef", lambda c: c)
    worst = 0.0
    for c in R.reference():
        if c["x"].size > 10000:
            continue
        got = R.loudness(c["x"], bend(c["coef"]), c["block"], **kw)
        want = float(c["loudness"])
        if got == want:
            continue
        worst = max(worst, math.inf if math.inf in (abs(got), abs(want)) else abs(float(got) - want))
    print(f"{name}: off by up to {worst:.3e} LU, the tolerance is {R.TOL_LU:.1e}")
    assert worst >= 100 * R.TOL_LU


def test_cases_hold_one_where_the_minus_8_and_minus_10_gates_differ():
    differ = 0
    for c in R.reference():
        z = R.blocks(c["x"], c["coef"], c["block"], np.longdouble)
        _, _, m10 = R.gates(z, c["x"].size, c["block"], np.longdouble)
        _, _, m8 = R.gates(z, c["x"].size, c["block"], np.longdouble, rel=-8.0)
        differ += m10 != m8
    assert differ >= 1


def test_no_block_lies_at_a_gate():
    """no z_j within a factor 1 +- 1e-6 of the absolute or of the relative gate: device and oracle cannot disagree on a gate"""
    for c in R.reference():
        z = R.blocks(c["x"], c["coef"], c["block"], np.longdouble)
        _, thr, _ = R.gates(z, c["x"].size, c["block"], np.longdouble)
        for g in [R.abs_gate(np.longdouble)] + ([] if thr is None else [thr]):
            for zz in z:
                assert abs(zz / g - 1) > 1e-6, (c["name"], float(zz), float(g))


def test_cases_cover_the_lengths_and_signals():
    ref = {c["name"]: c for c in R.reference()}
    b, h, s = R.SMALL_BLOCK, R.SMALL_BLOCK // 4, R.LD_SEG
    for L in (0, 1, b - 1, b, b + h - 1, s - 1, s, s + 1, 3 * s + 5, R.LD_TILE + 300):
        assert ref[f"len{L}"]["x"].size == L
    assert any((c["x"].size - c["block"]) % (c["block"] // 4) for c in ref.values() if c["x"].size > c["block"])
    assert ref["under_abs_gate"]["loudness"] == -math.inf and ref["zeros"]["loudness"] == -math.inf
    assert ref["max_gain_binds"]["limit"] == 1 and ref["ceiling_binds"]["limit"] == 2 and ref["measure_only"]["gain"] == 1
    assert ref["real_3s_16k"]["x"].size == 48000 and ref["real_3s_16k"]["block"] == audio.loudness_block(16000)
    assert {c["sr"] for c in ref.values()} == {16000, 48000}


def test_check_loudness_refuses_bad_parameters():
    audio.check_loudness(None, audio.PEAK_CEILING, 20.0)
    audio.check_loudness(-23, 1.0, 0)
    for bad in ((math.nan, 0.9, 20.0), (math.inf, 0.9, 20.0), ("-23", 0.9, 20.0), (True, 0.9, 20.0), (-23.0, 0.0, 20.0),
                (-23.0, -1.0, 20.0), (-23.0, math.nan, 20.0), (-23.0, 0.9, -1.0), (-23.0, 0.9, math.inf)):
        with pytest.raises(ValueError):
            audio.check_loudness(*bad)
