"""One decoder layer of the Spark-TTS-0.5B shape (hidden 896, intermediate 4864, 14 / 2 heads) taken apart, stage by stage, against
a float64 restatement of the layer (``oracle.llm_ref.layer_stages_f64``, pinned to transformers' own classes by
``tests/test_oracle_llm.py::test_float64_layer_stages_match_transformers_classes``) at every row-count regime of a decode step:
1 row (the fused attention + o_proj path in slot 0; the general path in another slot), 2..8 rows (the few-row GEMVs), 7+ rows
(the chain-split down_proj, ``dc_min``), 9..16 / 17..32 / 33..64 rows (``k_downC`` with one, two or four m-tiles; from 35 rows
its LDS passes 64 KiB), and the 14-head o_proj in its ``M > 8`` form.  The kernels run through ``smi_llm_debug_layer``, i.e.
``launch_one``: the launch builders and per-row-count kernel choices of a real step, on layer 0 and on the last layer of the
session's synthetic 0.5B arena.  Every slot holds its own cached context (positions 0 .. 703 across the rows).

Bars, relative to each stage's max |value|: 1e-5 (the kernels multiply exactly -- bf16 weights by exactly split fp32 operands --
and sum in fp32, so what remains is fp32 summation order; measured 1e-7 .. 6e-7).  bf16 KV cache: every element of the appended
K / V rows is held to one bf16 rounding of the reference's value (2^-8 of that element, the unit roundoff of 8 significand bits,
plus the 1e-5 bar), and the reference's attention reads the cache as the kernels left it (``debug_get_kv`` after stage 0), so
the later bars measure the kernels, not the cache rounding."""
import numpy as np
import pytest

from conftest import FULL_MAX_POS

pytestmark = pytest.mark.gpu

POSITIONS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 460, 690, FULL_MAX_POS - 1]
REL = 1e-5
MEASURED = {}          # (kv, layer, rows) -> {stage: max |diff| / scale}; printed at the end of the module (pytest -s)


@pytest.fixture(scope="module")
def layer_weights(full_llm):
    """The synthetic weights of layer 0 and of the last layer, generated once (SyntheticLLM builds a tensor on every lookup)."""
    cfg, syn, _ = full_llm
    return {n: syn[n] for n in syn.names() if n.startswith(("model.layers.0.", f"model.layers.{cfg.num_hidden_layers - 1}."))}


@pytest.fixture(scope="module")
def engines(full_llm):
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    out = {kv: SparkLLM(cfg, None, "cuda:0", max_slots=64, max_positions=FULL_MAX_POS, arena=arena, kv_dtype=kv, diag=True)
           for kv in ("f32", "bf16")}
    yield out
    for e in out.values():
        e.close()
    for key, errs in sorted(MEASURED.items()):
        print(f"[0.5B layer stages] {key}: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))


def _layout(nrows, shuffled):
    """(slot, pos) rows: row m in slot m (slot == row, the decode step's identity layout) or in a permuted slot; positions cycle
    through POSITIONS so that every row count sees short and long contexts.  40 rows: rows 38, 39 are the next two positions
    of row 37's slot (a prefill chunk's shape)."""
    slots = np.arange(nrows)
    if shuffled:
        slots = np.random.default_rng(nrows).permutation(64)[:nrows]
    pos = np.array([POSITIONS[(5 * m + nrows) % len(POSITIONS)] for m in range(nrows)])
    if nrows == 40:
        pos[37] = 300
        slots[38:] = slots[37]
        pos[38:] = [301, 302]
    return np.stack([slots, pos], axis=1).astype(np.int32)


def _rounded(got, want, what, errs, key):
    """bf16 cache rows: each element within one rounding of the fp64 value, |got - want| <= 2^-8 |want| (+ the fp32 bar)"""
    scale = float(np.abs(want).max())
    excess = np.abs(got.astype(np.float64) - want) - 2.0 ** -8 * np.abs(want)
    errs[key] = float(np.abs(got.astype(np.float64) - want).max()) / scale
    assert excess.max() <= REL * scale, f"{what}: an element is {excess.max():.3e} beyond one bf16 rounding (scale {scale:.3f})"


def _close(got, want, rel, what, errs, key):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    errs[key] = err / scale
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} against scale {scale:.3f} ({err / scale:.2e}; bar {rel:g})"


CASES = [(1, False), (1, True), (2, False), (7, False), (8, True), (9, True), (16, False), (17, False), (32, False), (33, False),
         (34, True), (35, False), (40, True), (64, False)]


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("nrows,shuffled", CASES, ids=[f"{n}{'-perm' if s else ''}" for n, s in CASES])
def test_full_size_layer_stages_against_float64(full_llm, layer_weights, engines, kv, nrows, shuffled):
    from oracle.llm_ref import layer_stages_f64
    cfg, syn, _ = full_llm
    llm = engines[kv]
    rows = _layout(nrows, shuffled)
    rng = np.random.default_rng(1000 + 7 * nrows + shuffled)
    nkv = cfg.num_key_value_heads
    for layer in (0, cfg.num_hidden_layers - 1):
        x = rng.standard_normal((nrows, cfg.hidden_size)).astype(np.float32)
        kc, vc = {}, {}
        for s in np.unique(rows[:, 0]):
            n = int(rows[rows[:, 0] == s, 1].min())          # context below the slot's first row
            kc[s] = rng.standard_normal((n, nkv, 64)).astype(np.float32)
            vc[s] = rng.standard_normal((n, nkv, 64)).astype(np.float32)
            if n:
                llm.debug_set_kv(layer, int(s), kc[s], vc[s])
        tag = f"{nrows} rows{' (permuted slots)' if shuffled else ''}, {kv} KV, layer {layer}"
        errs = MEASURED.setdefault((kv, layer, f"{nrows}{'p' if shuffled else ''}"), {})
        out0 = llm.debug_layer(layer, rows, x, 0)
        if kv == "bf16":   # the reference attends over the cache as stored (context and the rows' own K / V rows, in bf16)
            for s in kc:
                n = int(rows[rows[:, 0] == s, 1].max()) + 1
                kc[s], vc[s] = llm.debug_get_kv(layer, int(s), 0, n)
        ref = layer_stages_f64(cfg, layer_weights, layer, rows, x, kc, vc, own_kv=kv == "f32")
        _close(out0["q"], ref["q"], REL, f"{tag}: stage 0 q", errs, "q")
        for name in ("k", "v"):
            if kv == "f32":
                _close(out0[name], ref[name], REL, f"{tag}: stage 0 {name}", errs, name)
            else:
                _rounded(out0[name], ref[name], f"{tag}: stage 0 {name} (bf16 cache row)", errs, name)
        fused = nrows == 1 and rows[0, 0] == 0 and llm.debug_fused_o()
        if not fused:    # one row in slot 0: stage 1 happens inside the fused attention + o_proj kernel (no buffer to read)
            _close(llm.debug_layer(layer, rows, x, 1)["attn"], ref["attn"], REL, f"{tag}: stage 1 attention", errs, "attn")
        _close(llm.debug_layer(layer, rows, x, 2)["h"], ref["h_mid"], REL, f"{tag}: stage 2 o_proj + residual", errs, "h_mid")
        _close(llm.debug_layer(layer, rows, x, 3)["act"], ref["act"], REL, f"{tag}: stage 3 SwiGLU", errs, "act")
        _close(llm.debug_layer(layer, rows, x, 4)["h"], ref["h_out"], REL, f"{tag}: stage 4 down_proj + residual", errs, "h_out")
