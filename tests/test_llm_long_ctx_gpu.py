"""Attention beyond one context segment (kAttnSeg = 1024 keys), stage by stage against float64, on a three-layer model of the
0.5B widths (hidden 896, intermediate 4864, 14 / 2 heads) with 4096 positions per slot -- what SparkTTS runs by default and what
no sibling module reaches (they stop at 704 positions).

Decode (``smi_llm_debug_layer``, layers 0 and 2, stages 0-4, f32 and bf16 cache): with a row at position >= 1024 even a one-row
step leaves the fused one-row kernel for the general ``k_attn<KV, 0>`` with one block per (head, row, segment) and ``k_attn_merge``;
``ensure_apart`` grows the partial buffer (the cases run 2, then 3, then 4 segments).  Rows: one row in slot 0 at every position
of {1022 .. 1025, 1279, 1280, 2047 .. 2049, 3071, 3072, 4094, 4095}; one row in slot 3; 2, 9, 17 and 64 rows with at most three long
rows among short ones (positions below 64: their later segments are empty), short rows before and after a long one, permuted
slots, two consecutive positions of one slot on either side of 1023 / 1024.  Bit for bit, as the code states: (i) a row below 1024
in a call with several segments equals the row alone with one (k_attn_merge's comment); (ii) a long row alone equals the row among
9 or 64; (iii) identity slots equal permuted slots.

Prompt pass (``smi_llm_debug_prefill_layer``, layer 0, stages 0-2; ``k_attn_pf<f32>``, ``k_attn_pf2``, ``k_attn_pf<bf16>``): 1025 rows
from position 0, 70 rows from 1000 (tiles whose keys straddle 1024), 65 rows from 2040 beside 300 from 0, 65 rows ending on the
cache's last position, and the row-grouped family on 40 rows from 1010.

Leak sentinel: in every call, every cache position above a slot's last row, up to the slot's end, holds K = 0 (an ordinary
score), V = 1e4 -- a key read beyond the row's own position would shift the output by many bars; one test runs the same rows over
zeros instead and wants the same bits.

Bars, relative to each stage's max |value|: 1e-5, the sibling modules'.  The attention stage beyond 704 keys: an fp32 restatement
in the kernels' summation order (llm_ctx_cases.attn_f32_restated; test_llm_long_ctx_cpu.py holds it to half the bar) gives 4.5e-7 ..
9.7e-7 on rows of these cases with 1024 to 4096 keys.  bf16 cache: appended K / V elements within one bf16 rounding of the
reference; the reference then attends over the cache as stored (``debug_get_kv``).
Measured on MI355X over every (engine, case, layer): attention 8.8e-8 .. 1.9e-6 (below 5e-6: the 1e-5 bar stays), q 1.1e-7 ..
1.2e-6, f32 K / V rows 9.2e-8 .. 8.8e-7, o_proj + residual 3.3e-8 .. 7.1e-7, SwiGLU 1.2e-7 .. 5.1e-7, down_proj + residual 1.7e-7 ..
3.7e-7; bf16 K / V rows 1.5e-3 .. 3.8e-3 of the rows' scale (2^-8 = 3.9e-3).  Printed per stage and at teardown (pytest -s)."""
import numpy as np
import pytest

import llm_ctx_cases as X

pytestmark = pytest.mark.gpu

MEASURED = {}


@pytest.fixture(scope="module")
def model():
    cfg = X.model_cfg()
    weights = X.model_weights(cfg)
    return cfg, weights, X.device_arena(cfg, weights)


@pytest.fixture(scope="module")
def engines(model):
    cfg, _, arena = model
    out = {"f32": X.make_engine(cfg, arena, "f32", 64), "bf16": X.make_engine(cfg, arena, "bf16", 64),
           "bf16-pf0": X.make_engine(cfg, arena, "bf16", 8, {"SPARKMI_ATTN_PF2": "0"})}
    for e in out.values():
        e.cache = X.Cache(e)
    yield out
    for e in out.values():
        e.close()
    X.report("long-context layer stages", MEASURED)


def _last(rows):
    return {int(s): int(rows[rows[:, 0] == s, 1].max()) for s in np.unique(rows[:, 0])}


def _load(llm, cfg, layer, case_rows, cache=None):
    rows, x, kc, vc = X.decode_inputs(cfg, layer, case_rows)
    (cache or llm.cache).load(layer, kc, vc, _last(rows))
    return rows, x, kc, vc


def _fused(llm, rows):
    return len(rows) == 1 and rows[0, 0] == 0 and rows[0, 1] < X.SEG and llm.debug_fused_o()


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("case", list(X.DECODE_CASES))
def test_decode_stages_beyond_one_segment_against_float64(model, engines, kv, case):
    from oracle.llm_ref import layer_stages_f64
    cfg, weights, _ = model
    llm = engines[kv]
    for layer in (0, 2):
        rows, x, kc, vc = _load(llm, cfg, layer, X.DECODE_CASES[case])
        nseg = -(-(int(rows[:, 1].max()) + 1) // X.SEG)
        tag = f"{case} ({len(rows)} rows, {nseg} segments), {kv} KV, layer {layer}:"
        errs = MEASURED.setdefault((kv, case, layer), {})
        out0 = llm.debug_layer(layer, rows, x, 0)
        if kv == "bf16":   # the reference attends over the cache as stored (context and the rows' own K / V rows, in bf16)
            for s, lp in _last(rows).items():
                kc[s], vc[s] = llm.debug_get_kv(layer, s, 0, lp + 1)
        ref = layer_stages_f64(cfg, weights, layer, rows, x, kc, vc, own_kv=kv == "f32")
        X.check_qkv(out0, ref, kv == "f32", tag, errs)
        if not _fused(llm, rows):   # (one row below 1024 in slot 0: stage 1 happens inside the fused kernel)
            X.close(llm.debug_layer(layer, rows, x, 1)["attn"], ref["attn"], f"{tag} stage 1 attention", errs, "attn")
        X.close(llm.debug_layer(layer, rows, x, 2)["h"], ref["h_mid"], f"{tag} stage 2 o_proj + residual", errs, "h_mid")
        X.close(llm.debug_layer(layer, rows, x, 3)["act"], ref["act"], f"{tag} stage 3 SwiGLU", errs, "act")
        X.close(llm.debug_layer(layer, rows, x, 4)["h"], ref["h_out"], f"{tag} stage 4 down_proj + residual", errs, "h_out")
        for s, lp in _last(rows).items():
            assert llm.cache.sentinel_intact(layer, s, lp + 1, min(64, X.MAX_POS - lp - 1)), f"{tag} slot {s}: the append wrote above position {lp}"


def _bits(llm, cfg, layer, case_rows, cache=None):
    """Appended K / V rows and the stage 1 and 2 outputs of one call (stage 1: None for the fused one-row kernel)"""
    rows, x, _, _ = _load(llm, cfg, layer, case_rows, cache)
    out0 = llm.debug_layer(layer, rows, x, 0)
    return {"k": out0["k"], "v": out0["v"], "attn": None if _fused(llm, rows) else llm.debug_layer(layer, rows, x, 1)["attn"],
            "h_mid": llm.debug_layer(layer, rows, x, 2)["h"]}


def _same_rows(a, ia, b, ib, what):
    for name in a:
        if a[name] is not None and b[name] is not None:
            assert np.array_equal(a[name][ia], b[name][ib]), f"{what}: {name} differs"


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_a_short_row_keeps_its_bits_in_a_call_with_several_segments(model, engines, kv):
    """(i) k_attn_merge: 'a row with one segment reproduces the unsplit result bit for bit'.  Short rows of the 9-row call (3
    segments) and of the straddling call, before, between and after the long rows, against the same row alone (1 segment); the
    row of slot 0 alone takes the fused one-row kernel (no stage 1 buffer: its stage 2 row is compared)."""
    cfg = model[0]
    llm = engines[kv]
    for case, picks in (("9rows", (0, 1, 6, 8)), ("9rows-straddle", (0, 1, 3, 8)), ("2rows-short-long", (0,)), ("2rows-long-short", (1,))):
        rows = X.DECODE_CASES[case]
        batch = _bits(llm, cfg, 0, rows)
        for m in picks:
            assert rows[m][1] < X.SEG
            solo = _bits(llm, cfg, 0, [rows[m]])
            _same_rows(solo, 0, batch, m, f"{kv} KV, {case}: row {m} {rows[m]} alone (1 segment) vs in the call")


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_a_long_row_alone_equals_the_row_among_9_and_64(model, engines, kv):
    """(ii) the same (slot, position), residual row and context: alone, among 9 rows and among 64 rows (slot 2, position 2047)."""
    cfg = model[0]
    llm = engines[kv]
    for layer in (0, 2):
        solo = _bits(llm, cfg, layer, [(2, 2047)])
        for case in ("9rows", "64rows"):
            assert X.DECODE_CASES[case][2] == (2, 2047)
            _same_rows(solo, 0, _bits(llm, cfg, layer, X.DECODE_CASES[case]), 2, f"{kv} KV, layer {layer}: (2, 2047) alone vs in {case}")
    for m in (5, 7):   # the other long rows of the 9-row call
        row = X.DECODE_CASES["9rows"][m]
        _same_rows(_bits(llm, cfg, 0, [row]), 0, _bits(llm, cfg, 0, X.DECODE_CASES["9rows"]), m, f"{kv} KV: {row} alone vs among 9")


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_identity_and_permuted_slots_give_the_same_bits(model, engines, kv):
    """(iii) the 9 rows in slots 0 .. 8 in order (the slot == row addressing) and in permuted slots (row descriptors)."""
    cfg = model[0]
    llm = engines[kv]
    a, b = X.DECODE_CASES["9rows"], X.DECODE_CASES["9rows-perm"]
    assert [p for _, p in a] == [p for _, p in b] and [s for s, _ in a] != [s for s, _ in b]
    for layer in (0, 2):
        _same_rows(_bits(llm, cfg, layer, a), slice(None), _bits(llm, cfg, layer, b), slice(None), f"{kv} KV, layer {layer}: identity vs permuted slots")


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_the_leak_sentinel_changes_nothing(model, engines, kv):
    """The straddling 9-row call over a cache whose positions above the rows hold K = 0 / V = 1e4, and over zeros there: same bits."""
    cfg = model[0]
    llm = engines[kv]
    rows = X.DECODE_CASES["9rows-straddle"]
    with_sentinel = _bits(llm, cfg, 0, rows)
    for s, lp in _last(np.array(rows)).items():
        llm.cache.fill(0, s, lp + 1, X.MAX_POS - lp - 1, 0.0, 0.0)
    try:
        over_zeros = _bits(llm, cfg, 0, rows, cache=X.Cache(llm, sentinel=False))
    finally:
        for s, lp in _last(np.array(rows)).items():
            llm.cache.fill(0, s, lp + 1, X.MAX_POS - lp - 1, 0.0, X.SENTINEL_V)
    _same_rows(with_sentinel, slice(None), over_zeros, slice(None), f"{kv} KV: sentinel vs zeros above the rows")


PF_CASES = [(e, c) for e in ("f32", "bf16", "bf16-pf0") for c in X.PREFILL_CASES if X.PREFILL_CASES[c][1] == X.PF_PGEMM or e == "f32"]


@pytest.mark.parametrize("eng,case", PF_CASES, ids=[f"{e}-{c}" for e, c in PF_CASES])
def test_prompt_pass_beyond_one_segment_against_float64(model, engines, eng, case):
    from oracle.llm_ref import layer_stages_f64
    cfg, weights, _ = model
    llm = engines[eng]
    f32 = eng == "f32"
    plan, family = X.PREFILL_CASES[case]
    seqs, rows, x, kc, vc = X.prefill_inputs(cfg, 0, plan, sum(n for _, n in plan))
    llm.cache.load(0, kc, vc, {s: p0 + n - 1 for s, p0, n in seqs})
    tag = f"prompt pass {case} ({'grouped' if family == X.PF_GROUPED else 'k_pgemm'}), {eng}, layer 0:"
    errs = MEASURED.setdefault((eng, "pf " + case, 0), {})
    run = lambda stage: llm.debug_prefill_layer(0, seqs, x, stage, family)  # noqa: E731
    out0 = run(0)
    if not f32:
        for s, p0, n in seqs:
            kc[s], vc[s] = llm.debug_get_kv(0, s, 0, p0 + n)
    ref = layer_stages_f64(cfg, weights, 0, rows, x, kc, vc, own_kv=f32, mlp=False)
    X.check_qkv(out0, ref, f32, tag, errs)
    X.close(run(1)["attn"], ref["attn"], f"{tag} stage 1 attention", errs, "attn")
    X.close(run(2)["h"], ref["h_mid"], f"{tag} stage 2 o_proj + residual", errs, "h_mid")
    for s, p0, n in seqs:
        assert llm.cache.sentinel_intact(0, s, p0 + n, min(64, X.MAX_POS - p0 - n)), f"{tag} slot {s}: the append wrote above its rows"
