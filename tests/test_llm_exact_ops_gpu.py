"""The exact-weights mode (``weights_exact = 1``, DESIGN.md 3.10: k_gemm_x with its QKV, o_proj, gate_up, down_proj and lm_head
epilogues) at the 0.5B widths on an fp32-saved checkpoint, against float64.  Four engines on one fp32 arena (three layers, vocab
320, max_positions 1024, 64 slots): f32 and bf16 cache, each contiguous and paged (16-token pages).  The cases, their inputs, the
checks and the corruptions they reject live in tests/llm_exact_cases.py; tests/test_llm_exact_ops_cpu.py shows on the CPU that an
fp32 model of the kernel's arithmetic passes every check here and that every corruption fails one.

a. Stage by stage (``smi_llm_debug_layer`` stages 0-4, layer 0 and the last layer) against ``oracle.llm_ref.layer_stages_f64`` on
   the fp32 weights: decode steps of 1, 2, 15, 16, 17, 32, 33, 49, 64 rows (every edge of gy = ceil(M / 16)) in identity and in
   permuted slots, and the three chunk shapes of the mode's prompt path (64 rows of one slot; 22 rows; 40 + 20 rows of two
   sequences).  Bar: 1e-5 of each stage's max |value| -- the siblings' bar (test_llm_ops_full_gpu.REL) on the siblings' argument:
   what separates the kernel from float64 is fp32 summation.  Here a length-K fp32 chain stands where they have exact products,
   and an fp32 model that rounds every product AND every sum of that chain stays at or below 3.9e-6 (h_out, K = 4864; CPU
   module), so the bar holds with a factor of 2.6 for a kernel that rounds less.  bf16 cache: the appended K / V elements within
   one bf16 rounding (2^-8 |want| plus the bar); the reference then attends over the cache as stored.
b. Whole model: ``forward_logits`` of 70 ids (chunks of 64 + 6: embed_row_x, and the hand-off of down_proj's ``ssout`` partials and
   ``XSout`` triples to the next layer's QKV and to the lm_head, which no stage test runs) against the float64 forward.  Bar:
   4 x ``WHOLE_MODEL_ERR``, the error of the fp32 chain model of the same forward on the same ids (4.5e-6 of max |logit|,
   measured on the CPU, never from a device); the factor covers the matrix instruction's order over its 4 k's and the device's
   expf / sqrtf.  The arg-max of every row is the float64 one wherever the float64 gap exceeds twice the bar.
c. Rows keep their solo bits: ``generate_ragged`` of 20 and of 40 ragged prompts (3 .. 90 tokens: one or two chunks) for 12 tokens
   on every engine -- the tokens, and the K / V rows of every layer read back with ``debug_get_kv`` from the same calls with the rows
   kept live, equal the same prompt run alone, bit for bit (two and three m-tiles per decode step, mixed chunks).  No bar: equality.

Measured on an MI355X (worst over all engines, cases and both layers): q 1.7e-6, k 1.4e-6, v 1.3e-6 (f32 caches), attn 2.6e-6,
h_mid 1.5e-6, act 2.5e-6, h_out 4.0e-6; whole model 5.8e-6.  The values of a run are printed at teardown (pytest -s)."""
import numpy as np
import pytest

import llm_ctx_cases as X
import llm_exact_cases as E

pytestmark = pytest.mark.gpu

MEASURED = {}          # (engine, case, layer) -> {stage: max |diff| / scale}
N_NEW = 12


@pytest.fixture(scope="module")
def rig():
    cfg = E.model_cfg()
    weights = E.model_weights()
    arena = E.exact_arena(cfg, weights)
    engines = {}
    for name, (kv, page) in E.ENGINES.items():
        engines[name] = E.make_engine(cfg, arena, name)
        engines[name].cache = X.Cache(engines[name], page=page, sentinel=False)
    yield cfg, weights, engines
    for e in engines.values():
        e.close()
    X.report("exact-weights layer stages", MEASURED)


@pytest.mark.parametrize("engine", list(E.ENGINES))
@pytest.mark.parametrize("name", list(E.CASES))
def test_exact_layer_stages_against_float64(rig, name, engine):
    cfg, weights, engines = rig
    llm = engines[engine]
    bf16 = E.ENGINES[engine][0] == "bf16"
    for layer in E.layers_under_test(cfg):
        rows, x, kc, vc = E.case_inputs(cfg, name, layer)
        llm.cache.load(layer, kc, vc, {})
        assert not llm.debug_fused_o(), "the exact-weights mode has no fused attention + o_proj"
        out = dict(llm.debug_layer(layer, rows, x, 0))
        stored = None
        if bf16:   # the cache as the kernels left it: the contexts and the rows' own K / V, in bf16
            stored = ({}, {})
            for s in kc:
                n = int(rows[rows[:, 0] == s, 1].max()) + 1
                stored[0][s], stored[1][s] = llm.debug_get_kv(layer, s, 0, n)
        out["attn"] = llm.debug_layer(layer, rows, x, 1)["attn"]
        out["h_mid"] = llm.debug_layer(layer, rows, x, 2)["h"]
        out["act"] = llm.debug_layer(layer, rows, x, 3)["act"]
        out["h_out"] = llm.debug_layer(layer, rows, x, 4)["h"]
        errs = MEASURED.setdefault((engine, name, layer), {})
        msg = E.judge(out, cfg, weights, layer, rows, x, kc, vc, bf16, stored, f"{engine}, case {name}, layer {layer}", errs)
        print(f"{engine} {name} layer {layer}: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))
        assert msg is None, msg


@pytest.mark.parametrize("engine", ["f32", "f32-paged"])
def test_exact_whole_model_logits_against_float64(rig, engine):
    cfg, weights, engines = rig
    ids = E.whole_model_ids(cfg)
    want = E.forward_f64(cfg, weights, ids)
    got = engines[engine].forward_logits(ids).cpu().numpy()
    ok, err, msg = E.whole_model_check(got, want, E.WHOLE_FACTOR * E.WHOLE_MODEL_ERR)
    print(f"[exact-weights whole model] {engine}: {err:.3e} of max |logit| (bar {E.WHOLE_FACTOR * E.WHOLE_MODEL_ERR:.1e}); {msg}")
    assert ok, f"{engine}: {msg}"


def _run_prompts(llm, cfg, prompts):
    """(tokens, K rows, V rows) per prompt of one greedy batch: N_NEW tokens each; K / V of every layer over the prompt and the
    generated positions that were fed back."""
    llm.session_begin(None)
    slots = llm.admit([list(p) for p in prompts])
    llm.decode(N_NEW - 1)
    toks = [t for t, _ in llm.slots_tokens(slots, N_NEW)]
    out = []
    for s, p, t in zip(slots, prompts, toks):
        kv = [llm.debug_get_kv(layer, s, 0, len(p) + N_NEW - 1) for layer in range(cfg.num_hidden_layers)]
        out.append((t, np.stack([k for k, _ in kv]), np.stack([v for _, v in kv])))
    llm.retire_many(slots)
    return out


@pytest.mark.parametrize("engine", list(E.ENGINES))
def test_exact_rows_keep_their_solo_bits(rig, engine):
    cfg, weights, engines = rig
    llm = engines[engine]
    prompts = E.ragged_prompts(cfg, 40)
    assert min(map(len, prompts)) == 3 and max(map(len, prompts)) == 90 and sum(len(p) > 64 for p in prompts) >= 4
    solo = [_run_prompts(llm, cfg, [p])[0] for p in prompts]
    assert all(len(t) == N_NEW for t, _, _ in solo)
    for n in (20, 40):
        ragged = llm.generate_ragged(prompts[:n], [N_NEW] * n)
        assert ragged == [t for t, _, _ in solo[:n]], f"{engine}: generate_ragged of {n} prompts does not emit the solo runs' tokens"
        batch = _run_prompts(llm, cfg, prompts[:n])    # generate_ragged's own calls, the rows kept live so that a paged cache still holds their pages
        for b in range(n):
            assert batch[b][0] == solo[b][0], f"{engine}, {n} prompts: row {b} (prompt of {len(prompts[b])}) emits {batch[b][0]}, alone {solo[b][0]}"
            for what, i in (("K", 1), ("V", 2)):
                same = np.array_equal(batch[b][i].view(np.uint32), solo[b][i].view(np.uint32))
                assert same, f"{engine}, {n} prompts: {what} rows of row {b} (prompt of {len(prompts[b])}) differ from the solo run's"
