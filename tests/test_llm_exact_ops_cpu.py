"""No GPU: the table behind tests/test_llm_exact_ops_gpu.py (tests/llm_exact_cases.py) is sound.

  * on every case the GPU module runs, the fp32 model of k_gemm_x's arithmetic (``llm_exact_cases.Model32``) stays within the
    stage bar (1e-5 of each stage's max |value|) against ``oracle.llm_ref.layer_stages_f64``; its worst values are printed;
  * every corruption of the table is rejected, by the check and on the case named in ``CAUGHT_BY``;
  * the whole-model constant ``WHOLE_MODEL_ERR`` is the value measured here, to two digits.

Measured here, at most over all cases and both layers (the model rounds every product and every sum; the device fuses them):
q 1.8e-6, k 1.3e-6, v 1.3e-6, attn 2.5e-6, h_mid 1.6e-6, act 2.3e-6, h_out 3.9e-6 (K = 4864) -- no stage reaches half of the bar;
the bar holds with a factor of 2.6 at the stage nearest to it.  Whole model (70 ids, three layers and the head): 4.5e-6 of
max |logit|."""
import numpy as np
import pytest

import llm_exact_cases as E

WORST = {}


@pytest.fixture(scope="module")
def model():
    cfg = E.model_cfg()
    w = E.model_weights()
    yield cfg, w, E.Model32(cfg, w)
    if WORST:
        print("\n[exact-weights fp32 model] worst per stage: " + ", ".join(f"{s} {WORST[s]:.2e}" for s in E.STAGES if s in WORST))


def _run(model, name, layer, bf16, corrupt=None, upto="h_out"):
    cfg, w, m32 = model
    rows, x, kc, vc = E.case_inputs(cfg, name, layer)
    out = m32.layer(layer, rows, x, kc, vc, bf16=bf16, corrupt=corrupt, upto=upto)
    stored = E.stored_cache(rows, kc, vc, out["k"], out["v"], True) if bf16 else None
    errs = {}
    msg = E.judge(out, cfg, w, layer, rows, x, kc, vc, bf16, stored, f"{name} layer {layer}", errs, upto=upto)
    return msg, errs


BF16_TOO = ("17", "33-perm", "chunkC-40+20")


@pytest.mark.parametrize("name", list(E.CASES))
def test_fp32_model_stays_within_the_stage_bar(model, name):
    cfg = model[0]
    for layer in E.layers_under_test(cfg):
        for bf16 in ((False, True) if name in BF16_TOO and layer == 0 else (False,)):
            msg, errs = _run(model, name, layer, bf16)
            print(f"{name} layer {layer} {'bf16' if bf16 else 'f32'}: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))
            assert msg is None, msg
            for s, e in errs.items():
                if not (bf16 and s in ("k", "v")):
                    WORST[s] = max(WORST.get(s, 0.0), e)
                    assert e <= 0.5 * E.REL, f"{name} layer {layer}: {s} at {e:.2e}, above half the bar: say so in the module docstring"


# corruption -> (case, layer, cache of the engine, the stage whose check rejects it); "whole": the whole-model bar (test 2b)
CAUGHT_BY = {
    "drop_last_kstep": ("2", 0, "f32", "q"),
    "weights_bf16": ("1", 0, "f32", "q"),
    "mc_wide": ("32", 0, "f32", "q"),                       # (17 rows cannot show it: row 16 IS row M - 1)
    "neighbour_norm": ("17", 0, "f32", "q"),
    "rope_row_index": ("15-perm", 0, "f32", "q"),
    "swiglu_swapped": ("1", 2, "f32", "act"),
    "no_resid_last_tile": ("33", 0, "f32", "h_mid"),
    "bf16_truncate": ("chunkB-22", 0, "bf16", "k"),
    "ssout_group_missing": ("whole", None, "f32", "logits"),
}


def test_every_corruption_is_listed():
    assert set(CAUGHT_BY) == set(E.CORRUPTIONS)
    assert all(c[0] in E.CASES or c[0] == "whole" for c in CAUGHT_BY.values())


@pytest.mark.parametrize("corrupt", [c for c in E.CORRUPTIONS if CAUGHT_BY[c][0] != "whole"])
def test_stage_corruptions_are_rejected(model, corrupt):
    name, layer, kv, stage = CAUGHT_BY[corrupt]
    msg, errs = _run(model, name, layer, kv == "bf16", upto=stage)
    assert msg is None, f"the clean model fails where {corrupt} is to be shown: {msg}"
    msg, errs = _run(model, name, layer, kv == "bf16", corrupt=corrupt, upto=stage)
    print(f"{corrupt} on {name}, layer {layer}, {kv} cache: {msg}")
    assert msg is not None and f": {stage}" in msg, f"{corrupt} passes the {stage} check of case {name} ({errs})"


def test_whole_model_constant_is_the_measured_one(model):
    cfg, w, m32 = model
    ids = E.whole_model_ids(cfg)
    want = E.forward_f64(cfg, w, ids)
    got = m32.forward(ids)
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max()) / scale
    print(f"whole model, {len(ids)} ids: fp32 chain model at {err:.4e} of max |logit| {scale:.3f}; committed {E.WHOLE_MODEL_ERR:.1e}")
    assert f"{err:.1e}" == f"{E.WHOLE_MODEL_ERR:.1e}", f"measured {err:.4e}, llm_exact_cases.WHOLE_MODEL_ERR is {E.WHOLE_MODEL_ERR:.4e}"
    bar = E.WHOLE_FACTOR * E.WHOLE_MODEL_ERR
    ok, e, msg = E.whole_model_check(got, want, bar)
    assert ok, msg
    held = int(msg.split()[0])
    assert held >= len(ids) // 2, f"only {msg}: the arg-max rule would check too little"
    # the hand-off no stage test sees: down_proj's ssout partials feeding the next layer's norm factor
    bad = m32.forward(ids, corrupt="ssout_group_missing")
    ok, e, msg = E.whole_model_check(bad, want, bar)
    print(f"ssout_group_missing: {msg}")
    assert not ok and e > 100 * bar, f"missing ssout partials pass the whole-model bar ({e:.3e})"
