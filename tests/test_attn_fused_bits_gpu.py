"""The one-row fused attention + o_proj kernel (k_attn<.., ONE = 1, FUSE = 1>) runs the cross-wave merge of its heads' outputs in
every o_proj wave (no second barrier, no shared LDS hand-off).  Its residual rows must keep the bits of the un-fused paths: the
one-row attention kernel followed by the o_proj GEMM, and the batched (several rows, slot == row) attention kernel.  Contexts
inside the first 256-key chunk, on its edge and across it, f32 and bf16 KV caches; one decoder layer (transformers' fixture
layer, tests/golden/llm_ops.npz) through ``debug_layer``."""
import os

import numpy as np
import pytest

from sparkmi import config as C

pytestmark = pytest.mark.gpu

CTXS = [9, 130, 255, 256, 257, 300, 511]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "llm_ops.npz"))


def _cfg():
    return C.LLMConfig(vocab_size=64, hidden_size=256, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2,
                       intermediate_size=608, rope_theta=1000000.0, rms_norm_eps=1e-6)


def _weights(g, cfg):
    from sparkmi.weights import round_bf16
    rng = np.random.default_rng(0)
    w = {"model.embed_tokens.weight": round_bf16((0.02 * rng.standard_normal((cfg.vocab_size, cfg.hidden_size))).astype(np.float32)),
         "model.norm.weight": np.ones(cfg.hidden_size, np.float32),
         "model.layers.0.input_layernorm.weight": g["ln1"], "model.layers.0.post_attention_layernorm.weight": g["ln2"]}
    for k in g.files:
        if k.startswith("attn/"):
            w["model.layers.0.self_attn." + k[5:]] = g[k]
        elif k.startswith("mlp/"):
            w["model.layers.0.mlp." + k[4:]] = g[k]
    return w


def _engine(g, kv, slots, monkeypatch, no_fuse):
    import warnings
    from sparkmi.llm import SparkLLM
    cfg = _cfg()
    with monkeypatch.context() as mp:
        if no_fuse:
            mp.setenv("SPARKMI_NO_FUSE_O", "1")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")        # (the q/k/v biases are fp32; the matrices are bf16-exact)
            return SparkLLM(cfg, _weights(g, cfg), "cuda:0", max_slots=slots, max_positions=512, kv_dtype=kv, diag=True)


def _caches(ctx, seed):
    """Keys and values of `ctx` cached tokens, (ctx, kv heads, 64)"""
    rng = np.random.default_rng(seed)
    k = (1.5 * rng.standard_normal((ctx, 2, 64))).astype(np.float32)
    v = rng.standard_normal((ctx, 2, 64)).astype(np.float32)
    return k, v


@pytest.mark.parametrize("kv", ["f32", "bf16"])
def test_one_row_fused_attention_keeps_the_bits_of_the_unfused_paths(fx, monkeypatch, kv):
    fused = _engine(fx, kv, 1, monkeypatch, no_fuse=False)
    plain = _engine(fx, kv, 1, monkeypatch, no_fuse=True)
    batched = _engine(fx, kv, 3, monkeypatch, no_fuse=False)
    x1 = fx["x"][:1]
    for i, ctx in enumerate(CTXS):
        k, v = _caches(ctx, 100 + i)
        for e in (fused, plain):
            e.debug_set_kv(0, 0, k, v)
        # the batched engine: the row under test in slot 1, other contexts around it
        for s, c in ((0, 40 + i), (1, ctx), (2, 511 - i)):
            kk, vv = (k, v) if s == 1 else _caches(c, 200 + 3 * i + s)
            batched.debug_set_kv(0, s, kk, vv)
        rows1 = np.array([[0, ctx]], np.int32)
        rows3 = np.array([[0, 40 + i], [1, ctx], [2, 511 - i]], np.int32)
        x3 = np.concatenate([fx["x"][1:2], x1, fx["x"][2:3]])
        for stage in (2, 4):   # the residual row after the o_proj, and after the MLP
            a = fused.debug_layer(0, rows1, x1, stage)["h"][0]
            c = batched.debug_layer(0, rows3, x3, stage)["h"][1]
            with monkeypatch.context() as mp:   # (debug_layer, too, reads the switch: where the one-row step leaves h)
                mp.setenv("SPARKMI_NO_FUSE_O", "1")
                b = plain.debug_layer(0, rows1, x1, stage)["h"][0]
            assert np.isfinite(a).all()
            assert np.array_equal(a, b), f"{kv} KV, context {ctx}, stage {stage}: fused one-row attention differs from one row + o_proj"
            assert np.array_equal(a, c), f"{kv} KV, context {ctx}, stage {stage}: fused one-row attention differs from the batched path"
