"""Two of the four one-row decode kernels build the addresses of their first loads at wave entry from a scalar base and a 32-bit lane
offset: the QKV kernel (operand staging load, RMSNorm partials and weight tiles, clamped where a wave has no tile, issued in front
of the row descriptor and the argument lines the epilogue needs) and the fused attention kernel (block id split without
divisions, K / V pieces).  gate_up and down_proj keep the code they had; they run in every step decoded here all the same.  None of
that may change a bit, so greedy one-row decodes are compared -- token ids and the
last step's residual row, bit for bit -- with values RECORDED FROM THE PARENT BUILD on the GPU (tests/golden/entry_loads_parent.npz,
written by tests/golden/gen_golden_entry_loads.py before any kernel was touched; the file names the parent's commit and the
SHA-256 of its smi_llm.hip).

Shapes:
  tiny_llm()              hidden 256, 4 / 2 heads, K_down 608: hot QKV, fused attention, gate_up NOH 4, k_down1<2>
  hidden 64, 1 / 1 head   KT = 2 k tiles: 14 of the hot QKV's 16 waves have no tile, so every clamp of its staging and weight
                          addresses is taken; K_down 160 (5 k tiles): k_down1<2> with most chains empty; unfused attention
  hidden 896, 14 / 2      the 0.5B widths with two layers: the instantiations of the benchmark's step (k_down1<10>, NOH 14)
Prompts of 1, 255, 256 and 257 tokens: a prompt's last token runs as the first one-row step, so the first decode contexts are
1 key, the last key of the attention kernel's first chunk of 256, the chunk edge, and the first key of the second chunk.
Twelve tokens each, all of them one-row steps."""
import os

import numpy as np
import pytest

from sparkmi import config as C

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "entry_loads_parent.npz")
NEW_TOKENS = 12
MAX_POS = 320
CONTEXTS = (1, 255, 256, 257)
SHAPES = {
    "tiny": lambda: C.tiny_llm(),
    "h64": lambda: C.LLMConfig(vocab_size=1003, hidden_size=64, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1,
                               intermediate_size=160, rope_theta=1000000.0, rms_norm_eps=1e-6),
    "h896": lambda: C.LLMConfig(vocab_size=1003, hidden_size=896, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2,
                                intermediate_size=4864, rope_theta=1000000.0, rms_norm_eps=1e-6),
}


def prompt_of(cfg, n):
    return np.random.Generator(np.random.PCG64(100 + n)).integers(0, cfg.vocab_size, size=n).tolist()


def decode_all(name):
    """{context: (token ids int64[NEW_TOKENS], residual row of the last step as uint32[hidden])} on one engine of the shape"""
    from sparkmi import weights as W
    from sparkmi.llm import SparkLLM
    cfg = SHAPES[name]()
    llm = SparkLLM(cfg, W.SyntheticLLM(cfg), "cuda:0", max_slots=1, max_positions=MAX_POS, diag=True)
    out = {}
    for n in CONTEXTS:
        toks = llm.generate_ids([prompt_of(cfg, n)], NEW_TOKENS)[0]
        out[n] = (np.asarray(toks, dtype=np.int64), llm.debug_hidden().view(np.uint32).copy())
    llm.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def decoded():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = decode_all(name)
        return cache[name]
    return get


@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_row_decode_keeps_the_parents_bits(recorded, decoded, name, ctx):
    toks, hid = decoded(name)[ctx]
    want_t, want_h = recorded[f"{name}_{ctx}_tokens"], recorded[f"{name}_{ctx}_hidden"]
    assert len(toks) == NEW_TOKENS and want_t.shape == (NEW_TOKENS,) and want_h.shape == hid.shape
    assert np.isfinite(hid.view(np.float32)).all()
    assert toks.tolist() == want_t.tolist(), f"{name}, first context {ctx} keys: token ids differ from the parent build's"
    diff = int((hid != want_h).sum())
    assert diff == 0, f"{name}, first context {ctx} keys: {diff} of {hid.size} residual values differ in bits from the parent build's"
