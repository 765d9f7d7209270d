"""The bars of test_llm_long_ctx_gpu.py and test_llm_paged_ops_gpu.py have teeth, and can be met (no GPU needed).

On the GPU modules' own inputs -- rows of their cases, on the same model, residual rows and cached contexts -- the attention of a
row is recomputed in float64 with one known defect at a time, each the kind of slip the kernels could make:
  the first key of the second segment dropped; the segments added without rescaling to the common maximum; a page looked up one
  entry early at a page edge; the last key of a partially filled chunk dropped.
Every one of them must miss the attention stage's bar (1e-5 of the stage's max |value|) by at least 10x.  The other way round, the
fp32 restatement of the kernels' documented summation order (llm_ctx_cases.attn_f32_restated: 128- / 256-key chunks, wave streams,
1024-key segments) must meet the bar with a factor 2 to spare on the same rows: a correct fp32 kernel passes, these defects do not."""
import numpy as np
import pytest

import llm_ctx_cases as X


@pytest.fixture(scope="module")
def model():
    cfg = X.model_cfg()
    return cfg, X.model_weights(cfg)


def _row_operands(model, layer, rows, m):
    """q (heads, 64) of row m after bias and RoPE, and the K / V of positions 0 .. pos that it attends to, in float64"""
    from oracle.llm_ref import layer_stages_f64
    cfg, weights = model
    rows, x, kc, vc = X.decode_inputs(cfg, layer, rows)
    ref = layer_stages_f64(cfg, weights, layer, rows, x, kc, vc, mlp=False)
    s, pos = rows[m]
    K, V = np.zeros((pos + 1, 2, 64)), np.zeros((pos + 1, 2, 64))
    K[: len(kc[s])], V[: len(vc[s])] = kc[s], vc[s]
    for i in np.flatnonzero((rows[:, 0] == s) & (rows[:, 1] <= pos)):
        K[rows[i, 1]], V[rows[i, 1]] = ref["k"][i], ref["v"][i]
    good = X.attn_f64(ref["q"][m], K, V)
    assert np.abs(good - ref["attn"][m]).max() <= 1e-12 * np.abs(good).max()      # attn_f64 without a defect is the reference
    return ref["q"][m], K, V, good


# (case of the GPU modules, row, the defects that apply at that row's position)
LONG = [("1row-slot0-1024", 0, ("drop-seg-first", "no-rescale")), ("1row-slot0-1025", 0, ("drop-seg-first", "no-rescale", "drop-chunk-last")),
        ("9rows", 2, ("drop-seg-first", "no-rescale")), ("9rows-straddle", 2, ("drop-seg-first", "no-rescale", "drop-chunk-last")),
        ("1row-slot0-3072", 0, ("drop-seg-first", "no-rescale", "drop-chunk-last")), ("64rows-last", 3, ("drop-seg-first", "no-rescale")),
        ("1row-slot3-2048", 0, ("drop-seg-first", "no-rescale", "drop-chunk-last"))]


@pytest.mark.parametrize("case,m,defects", LONG, ids=[c for c, _, _ in LONG])
def test_segment_and_chunk_defects_miss_the_bar_tenfold(model, case, m, defects):
    for layer in (0, 2):
        q, K, V, good = _row_operands(model, layer, X.DECODE_CASES[case], m)
        scale = np.abs(good).max()
        for d in defects:
            for chunk in ((128, 256) if d == "drop-chunk-last" else (256,)):
                miss = np.abs(X.attn_f64(q, K, V, d, chunk=chunk) - good).max() / scale
                print(f"{case} row {m} layer {layer}: {d} (chunk {chunk}) misses by {miss:.2e} of scale")
                assert miss >= 10 * X.REL, f"{case} row {m} layer {layer}: '{d}' moves the attention row by {miss:.2e} of its scale only"


@pytest.mark.parametrize("page", [16, 64])
def test_a_page_lookup_off_by_one_misses_the_bar_tenfold(model, page):
    for pos in [p for p in X.paged_positions(page) if p >= page]:
        for layer in (0, 2):
            q, K, V, good = _row_operands(model, layer, [(0, pos)], 0)
            miss = np.abs(X.attn_f64(q, K, V, "page-off-by-one", page=page) - good).max() / np.abs(good).max()
            print(f"page {page}, position {pos}, layer {layer}: misses by {miss:.2e} of scale")
            assert miss >= 10 * X.REL, f"page {page}, position {pos}, layer {layer}: moves the attention row by {miss:.2e} of its scale only"


@pytest.mark.parametrize("f32_cache", [True, False], ids=["f32", "bf16"])
def test_the_fp32_restatement_of_the_kernels_order_meets_the_bar(model, f32_cache):
    """1025, 2049 and 4096 keys (2, 3 and 4 segments, a one-key last segment among them) and 1024 keys (one segment)."""
    worst = 0.0
    for case, m in (("1row-slot0-1024", 0), ("1row-slot3-2048", 0), ("1row-slot0-4095", 0), ("9rows-straddle", 1)):
        q, K, V, good = _row_operands(model, 0, X.DECODE_CASES[case], m)
        q32, K32, V32 = q.astype(np.float32), K.astype(np.float32), V.astype(np.float32)
        want = X.attn_f64(q32, K32, V32)                    # (float64 on the operands as fp32 holds them)
        err = np.abs(X.attn_f32_restated(q32, K32, V32, f32_cache) - want).max() / np.abs(want).max()
        print(f"{case} row {m}: fp32 restatement {err:.2e} of scale")
        worst = max(worst, err)
    assert worst <= X.REL / 2, f"fp32 in the kernels' order: {worst:.2e} of scale (bar {X.REL:g})"
