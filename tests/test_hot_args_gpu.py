"""The one-row decode step starts its four layer kernels (QKV, fused attention, gate_up, down_proj) through hot entries: the
values on the address path of a kernel's first loads travel as leading scalar parameters (preloaded into SGPRs) in front of the
usual argument struct, and the body is shared with the struct-only entry that every other row count keeps.  A wrong or stale
hot value would move a load, so the step is checked against the launches that do not use the hot entries: the same prompt decoded as row 1 of a three-slot engine (the 2 .. 8-row
kernels, struct entries only) must give the same tokens and the same logits, bit for bit, as the one-slot engine with the step
graph and without it.

Shapes (launch_gemm_kv / launch_attn / launch_lm_persistent pick the instantiation from them):
  tiny_llm()                      hidden 256,  4 / 2 heads, K_down  608 (19 k tiles): k_down1<2>,  fused attention, gate_up NOH 4
  hidden 512, 8 / 2 heads         K_down 1088 (34 k tiles): k_down1<6>; 8 heads are not a fused-o_proj head count, so this shape
                                  runs the unfused attention and the plain one-row gate_up on their struct entries, and the hot
                                  QKV and down_proj around them
  hidden 896, 14 / 2 heads        K_down 4864 (152 k tiles): k_down1<10>, fused attention, gate_up NOH 14
Every sequence asks for log-probabilities, which makes each step's lm_head write its logits; the constrained case restricts
every row to the same id ranges, so the restricted one-row lm_head (k_lm<1, RT = 1>) closes the hot layers' step as well.  (The
lm_head and finalize kernels keep their struct entries: one launch each per step, their hot entries showed no measurable gain.)"""
import numpy as np
import pytest

from sparkmi import config as C

pytestmark = pytest.mark.gpu

STEPS = 6
SHAPES = {
    "tiny": lambda: C.tiny_llm(),
    "h512": lambda: C.LLMConfig(vocab_size=1003, hidden_size=512, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2,
                                intermediate_size=1088, rope_theta=1000000.0, rms_norm_eps=1e-6),
    "h896": lambda: C.LLMConfig(vocab_size=1003, hidden_size=896, num_hidden_layers=2, num_attention_heads=14, num_key_value_heads=2,
                                intermediate_size=4864, rope_theta=1000000.0, rms_norm_eps=1e-6),
}
ALLOWED = list(range(5, 40)) + list(range(300, 420)) + list(range(990, 1003))   # three ranges, the last one in the odd last tile


def _prompts(cfg):
    rng = np.random.Generator(np.random.PCG64(7))
    return [rng.integers(0, cfg.vocab_size, size=n).tolist() for n in (12, 9, 15)]   # the row under test: 9 tokens


def _run(cfg, syn, kv, slots, use_graph, allowed):
    """(tokens, last step's logits) of the 9-token prompt: alone in a one-slot engine, or as row 1 of three"""
    from sparkmi.llm import SparkLLM
    llm = SparkLLM(cfg, syn, "cuda:0", max_slots=slots, max_positions=64, kv_dtype=kv, use_graph=use_graph, diag=True)
    req = {"return_log_probs": True}
    if allowed is not None:
        req["allowed_token_ids"] = allowed
    prompts = _prompts(cfg)
    prompts, row = ([prompts[1]], 0) if slots == 1 else (prompts, 1)
    llm.session_begin()
    got = llm.admit(prompts, sampling=[dict(req) for _ in prompts])
    assert got == list(range(len(prompts)))
    llm.decode(STEPS)
    toks = llm.slots_tokens(got, STEPS + 1)[row][0]
    logits = llm.debug_read(9).view(np.float32).reshape(len(prompts), cfg.vocab_size)[row].copy()
    llm.close()
    return toks, logits


def _check(name, kv, allowed):
    from sparkmi import weights as W
    cfg = SHAPES[name]()
    syn = W.SyntheticLLM(cfg)
    graph = _run(cfg, syn, kv, 1, True, allowed)
    plain = _run(cfg, syn, kv, 1, False, allowed)
    rows = _run(cfg, syn, kv, 3, True, allowed)
    ids = np.arange(cfg.vocab_size) if allowed is None else np.asarray(allowed)   # a restricted lm_head writes the listed tiles only
    assert len(graph[0]) == STEPS + 1 and np.isfinite(graph[1][ids]).all()
    if allowed is not None:
        assert set(graph[0]) <= set(allowed)
    for what, other in (("without the step graph", plain), ("as row 1 of three", rows)):
        assert graph[0] == other[0], f"{name}, {kv} KV: tokens of the one-row step differ {what}\n{graph[0]}\n{other[0]}"
        assert np.array_equal(graph[1][ids].view(np.uint32), other[1][ids].view(np.uint32)), \
            f"{name}, {kv} KV: the last step's logits of the one-row step differ {what}"


@pytest.mark.parametrize("kv", ["bf16", "f32"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_row_hot_entries_keep_tokens_and_logits(name, kv):
    _check(name, kv, None)


def test_one_row_hot_entries_under_a_restricted_lm_head_keep_tokens_and_logits():
    _check("h896", "bf16", ALLOWED)
