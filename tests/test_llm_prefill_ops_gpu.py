"""One decoder layer of the Spark-TTS-0.5B shape as the PROMPT pass runs it, stage by stage, against a float64 restatement of the
layer (``oracle.llm_ref.layer_stages_f64``, pinned to transformers' classes by ``tests/test_oracle_llm.py``).  The sibling module
(``test_llm_ops_full_gpu.py``) goes through ``launch_one`` and stops at 64 rows; this one goes through
``smi_llm_debug_prefill_layer``, i.e. the per-layer launch function every layer of a pass over more than 64 prompt rows goes through
(``launch_layer_big``), with the tiles and the RMSNorm-partial layout the pass itself builds: ``k_pgemm`` in its few-row shapes
(64-row blocks, split-K o_proj / down_proj + ``k_resid_comb``) and its many-row shapes (128-row blocks, K segments summed in the
block), ``k_attn_pf<f32>``, ``k_attn_pf<bf16>`` (``SPARKMI_ATTN_PF2=0``), ``k_attn_pf2`` on its 16-row tiles, ``k_load_hidden`` in the
big workspace, and the row-grouped decode GEMMs with their ``[rows][NT * 4]`` partials (``PF_GROUPED``).

Layer 0 runs stages 0-5 (5 = the layer, then layer 1's QKV: the one reader of the partials down_proj leaves; its reference input
is the h the kernels left after stage 4, so the stage measures that QKV alone), layer ``num_layers - 2`` stages 0-4, the last
layer stage 0 (a pass launches nothing after its K/V append).

Bars, relative to each stage's max |value|: 1e-5, the sibling module's, on the same argument (exact products of bf16 weights with
exactly split fp32 operands, fp32 sums; ``k_attn_pf2``'s q is an exact bf16 triple and its P x V is fp32).  bf16 cache: appended K / V
elements within one bf16 rounding of the reference (2^-8 |want|, plus the bar); the reference then attends over the cache as stored.
Measured on MI355X over every (engine, case, layer, stage): 1.7e-7 .. 1.7e-6; bf16 K / V rows 2.0e-3 .. 3.0e-3 of the rows' scale
(2^-8 = 3.9e-3).  Printed per stage and at teardown (pytest -s)."""
import os

import numpy as np
import pytest

from conftest import FULL_MAX_POS

pytestmark = pytest.mark.gpu

REL = 1e-5
MEASURED = {}          # (engine, case, layer) -> {stage: max |diff| / scale}
SLOTS = [3, 0, 6]      # sequence b of a case sits in KV slot SLOTS[b]
PF_GROUPED, PF_PGEMM = 1, 2

# case -> ((first position, rows) per sequence, family)
CASES = {
    "a-65": ([(0, 65)], PF_PGEMM),
    "b-127": ([(0, 127)], PF_PGEMM),
    "c-70+65+96": ([(0, 70), (0, 65), (0, 96)], PF_PGEMM),
    "d-257+255": ([(0, 257), (0, 255)], PF_PGEMM),
    "e-257+256": ([(0, 257), (0, 256)], PF_PGEMM),
    "f-689": ([(0, 689)], PF_PGEMM),
    "g-651:38": ([(651, 38)], PF_PGEMM),
    "g-651:38+300": ([(651, 38), (0, 300)], PF_PGEMM),
    "h-127-grouped": ([(0, 127)], PF_GROUPED),
}
ENGINES = ["f32", "bf16", "bf16-pf0"]     # k_attn_pf<1>, k_attn_pf2, k_attn_pf<0>


def _make(full_llm, kv, env=None, **kw):
    """A diagnostics engine on the session's arena; ``env`` is in the environment while it is created (the switches are read then)."""
    from sparkmi.llm import SparkLLM
    cfg, _, arena = full_llm
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return SparkLLM(cfg, None, "cuda:0", max_slots=8, max_positions=FULL_MAX_POS, arena=arena, kv_dtype=kv, diag=True, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def layer_weights(full_llm):
    cfg, syn, _ = full_llm
    nl = cfg.num_hidden_layers
    pre = tuple(f"model.layers.{l}." for l in (0, 1, nl - 2, nl - 1))
    return {n: syn[n] for n in syn.names() if n.startswith(pre)}


@pytest.fixture(scope="module")
def engines(full_llm):
    out = {"f32": _make(full_llm, "f32"), "bf16": _make(full_llm, "bf16"),
           "bf16-pf0": _make(full_llm, "bf16", {"SPARKMI_ATTN_PF2": "0"})}
    yield out
    for e in out.values():
        e.close()
    for key, errs in sorted(MEASURED.items()):
        print(f"[0.5B prompt-pass layer stages] {key}: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))
    allv = [e for errs in MEASURED.values() for s, e in errs.items() if not s.endswith("(bf16 rows)")]
    if allv:
        print(f"[0.5B prompt-pass layer stages] range over the fp32 outputs: {min(allv):.2e} .. {max(allv):.2e}")


def _seqs(plan):
    return [(SLOTS[b], p0, n) for b, (p0, n) in enumerate(plan)]


def _rows(seqs):
    return np.array([(s, p0 + t) for s, p0, n in seqs for t in range(n)], dtype=np.int32).reshape(-1, 2)


def _inputs(cfg, seqs, layer, seed):
    """The residual rows entering the layer and, per slot, the cached K / V below the sequence's first position."""
    rng = np.random.default_rng(seed)
    M = sum(n for _, _, n in seqs)
    x = rng.standard_normal((M, cfg.hidden_size)).astype(np.float32)
    nkv = cfg.num_key_value_heads
    kc = {s: rng.standard_normal((p0, nkv, 64)).astype(np.float32) for s, p0, _ in seqs}
    vc = {s: rng.standard_normal((p0, nkv, 64)).astype(np.float32) for s, p0, _ in seqs}
    return x, kc, vc


def _fill(llm, layer, kc, vc):
    for s in kc:
        if len(kc[s]):
            llm.debug_set_kv(layer, s, kc[s], vc[s])


def _rounded(got, want, what, errs, key):
    """bf16 cache rows: each element within one rounding of the fp64 value, |got - want| <= 2^-8 |want| (+ the fp32 bar)"""
    scale = float(np.abs(want).max())
    excess = np.abs(got.astype(np.float64) - want) - 2.0 ** -8 * np.abs(want)
    errs[key] = float(np.abs(got.astype(np.float64) - want).max()) / scale
    print(f"{what}: {errs[key]:.3e} of scale (bf16 rows)")
    assert excess.max() <= REL * scale, f"{what}: an element is {excess.max():.3e} beyond one bf16 rounding (scale {scale:.3f})"


def _close(got, want, what, errs, key):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    errs[key] = err / scale
    print(f"{what}: {err / scale:.3e} of scale")
    assert err <= REL * scale, f"{what}: max |diff| {err:.3e} against scale {scale:.3f} ({err / scale:.2e}; bar {REL:g})"


def _qkv(out, ref, f32, tag, errs, suffix=""):
    _close(out["q"], ref["q"], f"{tag} q", errs, "q" + suffix)
    for name in ("k", "v"):
        if f32:
            _close(out[name], ref[name], f"{tag} {name}", errs, name + suffix)
        else:
            _rounded(out[name], ref[name], f"{tag} {name} (bf16 cache row)", errs, name + suffix + " (bf16 rows)")


# (the row-grouped family is pinned with the f32 cache only: its attention kernels are the other cases')
STAGE_CASES = [(e, c) for e in ENGINES for c in CASES if CASES[c][1] == PF_PGEMM or e == "f32"]


@pytest.mark.parametrize("eng,case", STAGE_CASES, ids=[f"{e}-{c}" for e, c in STAGE_CASES])
def test_prompt_pass_layer_stages_against_float64(full_llm, layer_weights, engines, eng, case):
    from oracle.llm_ref import layer_stages_f64
    cfg = full_llm[0]
    plan, family = CASES[case]
    llm = engines[eng]
    f32 = eng == "f32"
    seqs = _seqs(plan)
    rows = _rows(seqs)
    nl = cfg.num_hidden_layers
    for layer in (0, nl - 2, nl - 1):
        x, kc, vc = _inputs(cfg, seqs, layer, 5000 + 31 * len(rows) + layer)
        _fill(llm, layer, kc, vc)
        tag = f"{case}, {eng}, layer {layer}:"
        errs = MEASURED.setdefault((eng, case, layer), {})
        run = lambda stage: llm.debug_prefill_layer(layer, seqs, x, stage, family)  # noqa: E731
        out0 = run(0)
        if layer == nl - 1:
            _qkv(out0, layer_stages_f64(cfg, layer_weights, layer, rows, x, {}, {}, qkv_only=True), f32, f"{tag} stage 0", errs)
            continue
        if not f32:   # the reference attends over the cache as stored (context and the rows' own K / V rows, in bf16)
            for s, p0, n in seqs:
                kc[s], vc[s] = llm.debug_get_kv(layer, s, 0, p0 + n)
        ref = layer_stages_f64(cfg, layer_weights, layer, rows, x, kc, vc, own_kv=f32)
        _qkv(out0, ref, f32, f"{tag} stage 0", errs)
        _close(run(1)["attn"], ref["attn"], f"{tag} stage 1 attention", errs, "attn")
        _close(run(2)["h"], ref["h_mid"], f"{tag} stage 2 o_proj + residual", errs, "h_mid")
        _close(run(3)["act"], ref["act"], f"{tag} stage 3 SwiGLU", errs, "act")
        h4 = run(4)["h"]
        _close(h4, ref["h_out"], f"{tag} stage 4 down_proj + residual", errs, "h_out")
        if layer == 0:   # layer 1's QKV on what down_proj left: h, its norm operand, the RMSNorm partials
            nxt = layer_stages_f64(cfg, layer_weights, 1, rows, h4, {}, {}, qkv_only=True)
            _qkv(run(5), nxt, f32, f"{tag} stage 5 (layer 1's QKV)", errs, "+1")


def _bits(llm, layer, seqs, x, family=PF_PGEMM):
    """K / V rows and the stage 1, 2, 4 outputs of one call, as (name, rows) pairs"""
    out0 = llm.debug_prefill_layer(layer, seqs, x, 0, family)
    return {"k": out0["k"], "v": out0["v"], "attn": llm.debug_prefill_layer(layer, seqs, x, 1, family)["attn"],
            "h_mid": llm.debug_prefill_layer(layer, seqs, x, 2, family)["h"],
            "h_out": llm.debug_prefill_layer(layer, seqs, x, 4, family)["h"]}


def _solo_equals_batch(llm, cfg, plan, which, what):
    seqs = _seqs(plan)
    x, kc, vc = _inputs(cfg, seqs, 0, 77 + len(plan))
    _fill(llm, 0, kc, vc)
    batch = _bits(llm, 0, seqs, x)
    m0 = 0
    for b, sq in enumerate(seqs):
        n = sq[2]
        if b in which:
            solo = _bits(llm, 0, [sq], x[m0: m0 + n])
            for name, got in solo.items():
                assert np.array_equal(got, batch[name][m0: m0 + n]), f"{what}: sequence {b} ({n} rows) alone vs in the batch: {name} differs"
        m0 += n


@pytest.mark.parametrize("eng", ENGINES)
def test_a_sequence_of_a_pass_equals_its_solo_run(full_llm, engines, eng):
    """Three sequences in one pass (m-tiles and attention tiles break mid-16 at the sequence boundaries): each one's K / V rows and
    its stage 1, 2, 4 rows are the bits of the same sequence run alone in the same slot."""
    _solo_equals_batch(engines[eng], full_llm[0], CASES["c-70+65+96"][0], (0, 1, 2), f"{eng}, 70 + 65 + 96 rows")


@pytest.mark.parametrize("eng", ENGINES)
def test_few_row_and_many_row_shapes_give_the_same_bits(full_llm, engines, eng):
    """257 rows alone take k_pgemm's few-row shapes (split-K o_proj / down_proj + k_resid_comb); beside 256 more rows the pass
    has 513 and takes the many-row shapes (K segments summed in the block): same bits."""
    _solo_equals_batch(engines[eng], full_llm[0], CASES["e-257+256"][0], (0,), f"{eng}, 257 of 513 rows")


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_split_k_combine_equals_the_in_block_segments(full_llm, engines, kv):
    """SPARKMI_PG_SPLIT_ROWS=0 keeps the in-block form of the segmented o_proj / down_proj sums at any row count: on the
    127-row prompt its h after stages 2 and 4 is the split-K form's, bit for bit."""
    cfg = full_llm[0]
    seqs = _seqs(CASES["b-127"][0])
    x, _, _ = _inputs(cfg, seqs, 0, 127)
    inblock = _make(full_llm, kv, {"SPARKMI_PG_SPLIT_ROWS": "0"})
    try:
        for stage in (2, 4):
            a = engines[kv].debug_prefill_layer(0, seqs, x, stage)["h"]
            b = inblock.debug_prefill_layer(0, seqs, x, stage)["h"]
            assert np.array_equal(a, b), f"{kv} KV, stage {stage}: split-K + k_resid_comb vs in-block K segments"
    finally:
        inblock.close()


def test_refusals_leave_the_engine_usable(full_llm, engines):
    from sparkmi._lib import SparkMIError
    cfg = full_llm[0]
    llm = engines["f32"]
    nl = cfg.num_hidden_layers
    x = np.random.default_rng(9).standard_normal((65, cfg.hidden_size)).astype(np.float32)
    ok = [(1, 0, 65)]
    want = llm.debug_prefill_layer(0, ok, x, 2)["h"]
    with pytest.raises(SparkMIError):
        llm.debug_prefill_layer(nl - 1, ok, x, 1)                         # the last layer ends with its K/V append
    with pytest.raises(SparkMIError):
        llm.debug_prefill_layer(0, [(1, 0, 0)], x[:0], 0)                  # M = 0
    with pytest.raises(SparkMIError):
        llm.debug_prefill_layer(0, np.zeros((0, 3), dtype=np.int32), x[:0], 0)
    with pytest.raises(SparkMIError):
        llm.debug_prefill_layer(0, [(1, FULL_MAX_POS - 64, 65)], x, 0)     # the last row sits at position max_positions
    with pytest.raises(SparkMIError):
        llm.debug_prefill_layer(0, [(8, 0, 65)], x, 0)                     # slot beyond max_slots
    assert np.array_equal(llm.debug_prefill_layer(0, ok, x, 2)["h"], want)
    assert llm.debug_prefill_layer(nl - 1, ok, x, 0)["q"].shape == (65, cfg.num_attention_heads, 64)
    paged = _make(full_llm, "f32", kv_page_tokens=64, kv_pages=32)
    try:
        # a paged cache is no refusal any more (tests/test_llm_paged_ops_gpu.py): the slot gets its pages and the bits are the same
        assert np.array_equal(paged.debug_prefill_layer(0, ok, x, 2)["h"], want)
        with pytest.raises(SparkMIError):
            paged.debug_prefill_layer(0, [(1, 0, 65), (8, 0, 65)], np.concatenate([x, x]), 0)   # slot beyond max_slots
        prompt = np.random.default_rng(10).integers(0, cfg.vocab_size, size=9).tolist()
        assert len(paged.generate_ids([prompt], 2)[0]) == 2                # the paged engine still generates
    finally:
        paged.close()
