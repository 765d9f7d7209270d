"""The int8 screen of the one-row greedy lm_head on the CPU: the numpy model of tests/lm_screen_ref.py (the copy, the screen
values, the bound, the selection) against float64.

For every case: |S_v - sum_k w_vk g_k| <= B_v - slack_v for every row (the closed-form part of the bound alone, without the
term that covers fp32 rounding); every tile that holds a row attaining the float64 maximum within head_cases.head_bound is
listed; and the list is not everything unless the case ties every tile."""
import numpy as np
import pytest

import head_cases as H
import lm_screen_ref as R

CASES = R.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_bound_holds_and_every_possible_winner_is_listed(name):
    W, gamma, x = CASES[name]
    V, K = W.shape
    g = (gamma * x).astype(np.float32)
    tiles, S, B, slack = R.model_list(W, g)
    t = H.f64(W) @ H.f64(g)
    err, room = np.abs(H.f64(S) - t), H.f64(B) - H.f64(slack)
    worst = float((err / np.maximum(room, 1e-300)).max())
    print(f"LM_SCREEN {name}: V={V} K={K} worst |S - t| / (B - slack) = {worst:.3f}, {len(tiles)} of {R.n_tiles(V)} tiles listed")
    assert (err <= room).all(), f"{name}: the screen value leaves its bound ({worst:.3f})"
    need = R.possible_winner_tiles(W, gamma, x)
    assert np.isin(need, tiles).all(), f"{name}: tiles {sorted(set(need) - set(tiles))} hold a possible winner and are not listed"
    assert np.isin(int(np.argmax(t)) // R.TILE, tiles)
    assert np.array_equal(tiles, np.unique(tiles)) and tiles.min() >= 0 and tiles.max() < R.n_tiles(V)
    if name == "identical":
        assert len(tiles) == R.n_tiles(V), "identical rows: every tile ties and must be listed"
    elif name != "huge_row":
        assert len(tiles) < R.n_tiles(V), f"{name}: the model lists everything"


def test_the_copy():
    W, gamma, x = CASES["zero_row"]
    s, q, sq = R.pack8(W)
    assert s[40] == 0 and not q[40].any() and sq[40] == 0, "a zero row: s = 0, q = 0"
    live = s > 0
    assert (np.abs(q[live]).max(axis=1) == 127).all() and np.abs(q).max() == 127
    e = np.abs(H.f64(W) - H.f64(s)[:, None] * q)
    # (the fp32 quotient w / s, at most 127, carries 127 * 2^-24 < 2^-17 of rounding into rint: part of what the slack term covers)
    assert (e <= H.f64(s)[:, None] * (0.5 + 2.0 ** -17)).all(), "|w - s q| <= s / 2"


def test_the_operand_split():
    for name, (W, gamma, x) in CASES.items():
        g = (gamma * x).astype(np.float32)
        op = R.operand(g)
        assert not op["all"]
        assert np.abs(op["X1"]).max() == 127 and np.abs(op["X2"]).max() <= 127
        r = H.f64(g) - (H.f64(op["a"]) * op["X1"] + H.f64(op["b"]) * op["X2"])
        assert (np.abs(r) <= H.f64(op["b"]) * (0.5 + 2.0 ** -16)).all(), f"{name}: the leftover exceeds b / 2"
    assert R.operand(np.zeros(64, np.float32))["all"] and R.operand(np.full(64, np.nan, np.float32))["all"]
    bad = np.ones(64, np.float32)
    bad[3] = np.inf
    assert R.operand(bad)["all"]


@pytest.mark.parametrize("hidden,vocab", [(64, 1003), (64, 4099), (928, 1003), (928, 4099)])
def test_the_gpu_tests_gaussian_rows_list_at_most_a_tenth_of_the_tiles(hidden, vocab):
    W, gamma = R.gaussian(hidden, vocab)
    x = R.gaussian_rows(hidden, vocab, W, gamma, 64)
    s, q, sq = R.pack8(W)
    most = 0
    for i in range(64):
        S, B, _ = R.screen(s, q, sq, R.operand((gamma * x[i]).astype(np.float32)))
        most = max(most, len(R.select(S, B, vocab)))
    assert most <= 0.10 * R.n_tiles(vocab), f"{most} of {R.n_tiles(vocab)} tiles"


def test_the_form_report_names_the_screened_head_only_when_asked():
    """smi_llm_gemm_forms (host only): default flags keep k_lm<1>; the new lm_screen flag names the three launches on the same grid."""
    import ctypes as C
    import dataclasses
    from sparkmi import _lib, config as cfgs
    from sparkmi.arena import llm_cfg_struct
    cs = llm_cfg_struct(dataclasses.replace(cfgs.spark_0p5b_llm(), num_hidden_layers=3), 64, 576, "bf16", False)
    d = _lib.diag()

    def head(M, **flags):
        out = (_lib.GemmFormInfo * 5)()
        rc = d.smi_llm_gemm_forms(C.byref(cs), M, _lib.SMI_LAYER_LAST, C.byref(_lib.GemmFlags(**flags)), out)
        return rc, out[4]

    rc, plain = head(1)
    assert rc == 0 and plain.kernel == b"k_lm<1,0>" and plain.launches == 1
    rc, off = head(1, lm_screen=0)
    assert rc == 0 and off.kernel == plain.kernel
    rc, scr = head(1, lm_screen=1)
    assert rc == 0 and scr.kernel == b"k_lm_screen+k_lm_select+k_lm<1,1,1>" and scr.launches == 3
    assert (scr.grid[0], scr.grid[1], scr.block, scr.lds_bytes) == (plain.grid[0], plain.grid[1], plain.block, plain.lds_bytes)
    assert head(2, lm_screen=1)[0] != 0 and head(1, lm_screen=1, exact=1)[0] != 0 and head(1, lm_screen=1, lm_restricted=1)[0] != 0
