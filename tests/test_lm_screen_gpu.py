"""The one-row greedy lm_head behind its int8 screen (k_lm_screen, k_lm_select, k_lm<1, RT, NM>) against the
lm_head it replaces: ``debug_head(screen=True)`` against ``debug_head()`` on the one-layer engines of tests/test_head_ops_gpu.py's
kind, and whole greedy decodes with the screen forced on (SPARKMI_LM_SCREEN=1) against forced off.

The screen must never change a token or the maximum's bits, and it must actually screen: the device's candidate list holds every
tile with a row attaining the stored row maximum, and at most twice the numpy model's list (tests/lm_screen_ref.py) plus two
tiles -- a screen that lists everything fails.  Hidden 1056 is 33 k tiles, outside the persistent lm_head (k_gemm<1, EPI_LM>
runs): there the request must change nothing, and the hook must say so."""
import numpy as np
import pytest

import head_cases as H
import lm_screen_ref as R
from sparkmi import config as C

pytestmark = pytest.mark.gpu

SCREENED = "k_lm_screen+k_lm<1,RT,NM>"
SHAPES = [(h, v) for h in (64, 928, 1056) for v in (1003, 4099)]


class _Cfg(C.LLMConfig):
    """head_dim 64 at any hidden size that is a multiple of 32 (as tests/test_head_ops_gpu.py)."""
    head_dim = property(lambda self: 64)


_ENGINES = {}


def _engine(key, hidden, vocab, W, gamma):
    if key in _ENGINES:
        return _ENGINES[key]
    from sparkmi.llm import SparkLLM
    cfg = _Cfg(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1,
               intermediate_size=32, rms_norm_eps=1e-6)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    p = "model.layers.0."
    w = {"model.embed_tokens.weight": W, "model.norm.weight": gamma, p + "input_layernorm.weight": np.ones(hidden, np.float32),
         p + "post_attention_layernorm.weight": np.ones(hidden, np.float32),
         p + "self_attn.q_proj.weight": z(64, hidden), p + "self_attn.k_proj.weight": z(64, hidden),
         p + "self_attn.v_proj.weight": z(64, hidden), p + "self_attn.q_proj.bias": z(64), p + "self_attn.k_proj.bias": z(64),
         p + "self_attn.v_proj.bias": z(64), p + "self_attn.o_proj.weight": z(hidden, 64),
         p + "mlp.gate_proj.weight": z(32, hidden), p + "mlp.up_proj.weight": z(32, hidden), p + "mlp.down_proj.weight": z(hidden, 32)}
    _ENGINES[key] = SparkLLM(cfg, w, "cuda:0", max_slots=2, max_positions=8, kv_dtype="bf16", diag=True)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for llm in _ENGINES.values():
        llm.close()
    _ENGINES.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pair(llm, x, hidden):
    """(unscreened, screened) debug_head of one row; the screened form where the hook applies, today's elsewhere."""
    off = llm.debug_head(x[None, :])
    on = llm.debug_head(x[None, :], screen=True)
    assert off["form"] == H.expected_form(hidden, llm.cfg.vocab_size, 1)[0]
    assert on["form"] == (SCREENED if H.ktiles(hidden) <= 32 else off["form"]), on["form"]
    assert on["nblk"] == off["nblk"] and on["grid"] == off["grid"] and on["block"] == off["block"]
    return off, on


def _same_pick(off, on, tag):
    assert on["tokens"][0] == off["tokens"][0], f"{tag}: token {on['tokens'][0]} behind the screen, {off['tokens'][0]} without"
    assert _bits(on["pval"].max()) == _bits(off["pval"].max()), f"{tag}: the maximum's bits differ"
    assert np.array_equal(_bits(on["h"]), _bits(off["h"])), f"{tag}: the next residual row differs"


@pytest.mark.parametrize("hidden,vocab", SHAPES, ids=[f"h{h}_v{v}" for h, v in SHAPES])
def test_64_gaussian_rows_same_token_same_maximum_and_a_short_list(hidden, vocab):
    W, gamma = R.gaussian(hidden, vocab)
    screened = H.ktiles(hidden) <= 32
    x = R.gaussian_rows(hidden, vocab, W, gamma, 64) if screened else R.gaussian_rows(hidden, vocab, W, gamma, 64, limit=1.0)
    llm = _engine(("g", hidden, vocab), hidden, vocab, W, gamma)
    nt, longest, model_longest = R.n_tiles(vocab), 0, 0
    s8, q8, sq8 = R.pack8(W)
    for i in range(64):
        tag = f"h{hidden} v{vocab} row {i}"
        off, on = _pair(llm, x[i], hidden)
        _same_pick(off, on, tag)
        if not screened:
            continue
        tiles, _ = llm.debug_lm_screen()
        stored = llm.debug_head(x[i][None, :], reads=[1], finalize=False)["logits_lm"][0]
        need = R.tiles_of(np.flatnonzero(stored == stored.max()))
        assert np.array_equal(tiles, np.unique(tiles)) and tiles.size and tiles.min() >= 0 and tiles.max() < nt, f"{tag}: list {tiles}"
        assert np.isin(need, tiles).all(), f"{tag}: tiles {need} hold the stored maximum, listed {tiles}"
        S, B, _ = R.screen(s8, q8, sq8, R.operand((gamma * x[i]).astype(np.float32)))
        model = R.select(S, B, vocab)
        assert len(model) <= 0.10 * nt
        assert len(tiles) <= 2 * len(model) + 2, f"{tag}: {len(tiles)} tiles listed, the model lists {len(model)}"
        # the partials: listed groups first, idle blocks at (-inf, no id)
        groups = (len(tiles) + 1) // 2
        assert (_bits(on["pval"][0, groups:]) == 0xFF800000).all() and (on["pidx"][0, groups:] == 0x7FFFFFFF).all(), f"{tag}: idle blocks"
        longest, model_longest = max(longest, len(tiles)), max(model_longest, len(model))
    print(f"LM_SCREEN_GPU h{hidden} v{vocab}: longest list {longest} of {nt} tiles (model {model_longest})")


def _planted(hidden, vocab, ids, tag):
    """Gaussian W with the rows `ids` all equal to one strong row, and an operand aligned with it: they tie for the maximum."""
    W, gamma = R.gaussian(hidden, vocab, tag)
    r = H.rng_of(f"lm_screen/planted/{hidden}/{vocab}/{tag}")
    x = r.standard_normal(hidden).astype(np.float32)
    row = H.round_bf16((0.25 * np.sign(gamma * x)).astype(np.float32))
    W = W.copy()
    W[list(ids)] = row
    return W, gamma, x


@pytest.mark.parametrize("hidden", [64, 928, 1056])
def test_planted_ties_take_the_lowest_id(hidden):
    vocab = 1003
    for tag, ids in (("far", (37, 530, 911)), ("last", (321, vocab - 1))):   # equal rows in different tiles; the last valid id tied with a lower one
        W, gamma, x = _planted(hidden, vocab, ids, tag)
        llm = _engine(("p", hidden, tag), hidden, vocab, W, gamma)
        off, on = _pair(llm, x, hidden)
        _same_pick(off, on, f"h{hidden} {tag}")
        assert on["tokens"][0] == min(ids), f"h{hidden} {tag}: token {on['tokens'][0]}, the tied rows are {ids}"
        if H.ktiles(hidden) <= 32:
            tiles, _ = llm.debug_lm_screen()
            assert np.isin(R.tiles_of(ids), tiles).all() and len(tiles) < R.n_tiles(vocab), f"h{hidden} {tag}: listed {tiles}"


@pytest.mark.parametrize("hidden", [64, 928])
def test_identical_rows_list_every_tile_and_give_token_0(hidden):
    vocab = 1003
    W, gamma = R.gaussian(hidden, vocab)
    W = np.repeat(W[:1], vocab, axis=0)
    llm = _engine(("i", hidden), hidden, vocab, W, gamma)
    x = H.rng_of(f"lm_screen/identical/{hidden}").standard_normal(hidden).astype(np.float32)
    off, on = _pair(llm, x, hidden)
    _same_pick(off, on, f"h{hidden} identical")
    tiles, _ = llm.debug_lm_screen()
    assert np.array_equal(tiles, np.arange(R.n_tiles(vocab))) and on["tokens"][0] == 0
    assert np.array_equal(_bits(on["pval"]), _bits(off["pval"])) and np.array_equal(on["pidx"], off["pidx"]), "every tile listed: today's partials"


@pytest.mark.parametrize("hidden", [64, 928, 1056])
def test_a_nan_operand_gives_token_0(hidden):
    vocab = 1003
    W, gamma = R.gaussian(hidden, vocab)
    llm = _engine(("g", hidden, vocab), hidden, vocab, W, gamma)
    x = H.rng_of(f"lm_screen/nan/{hidden}").standard_normal(hidden).astype(np.float32)
    x[hidden // 3] = np.nan
    off, on = _pair(llm, x, hidden)
    assert on["tokens"][0] == 0 and off["tokens"][0] == 0
    assert (_bits(on["pval"]) == 0xFF800000).all() and (on["pidx"] == 0x7FFFFFFF).all()
    if H.ktiles(hidden) <= 32:
        tiles, _ = llm.debug_lm_screen()
        assert np.array_equal(tiles, np.arange(R.n_tiles(vocab))), "a non-finite operand lists every tile"


def _decode(cfg, arena_from, weights, prompt, screen, max_positions):
    """12 greedy tokens and the residual row the last step left, on an engine created with the screen forced on / off."""
    from sparkmi.llm import SparkLLM
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv("SPARKMI_LM_SCREEN", "1" if screen else "0")   # read when the handle is created
        llm = SparkLLM(cfg, weights, "cuda:0", max_positions=max_positions, diag=True, arena=arena_from.arena if arena_from else None)
    finally:
        mp.undo()
    return llm


def _on_off(cfg, weights, lens, max_positions):
    off = _decode(cfg, None, weights, None, False, max_positions)
    on = _decode(cfg, off, weights, None, True, max_positions)     # the same device arena
    try:
        H_ = cfg.hidden_size
        for n in lens:
            prompt = H.rng_of(f"lm_screen/decode/{cfg.vocab_size}/{n}").integers(0, cfg.vocab_size, size=n).tolist()
            on.debug_lm_screen(reset=True)
            a = off.generate_ids([prompt], 12)[0]
            ha = off.debug_read(4, H_ * 4).view(np.uint32).copy()
            b = on.generate_ids([prompt], 12)[0]
            hb = on.debug_read(4, H_ * 4).view(np.uint32).copy()
            _, counts = on.debug_lm_screen()
            assert len(counts) >= 11, f"{n} keys: {len(counts)} screened steps, the 11 decode steps at least take the screen"
            assert a == b, f"{n} keys: tokens differ behind the screen\n{a}\n{b}"
            assert np.array_equal(ha, hb), f"{n} keys: the last residual row differs"
            print(f"LM_SCREEN_GPU decode vocab {cfg.vocab_size} {n} keys: candidate tiles per step {counts.tolist()}")
    finally:
        on.close()
        off.close()


def test_greedy_decode_of_the_tiny_model_is_bit_equal():
    from sparkmi import weights as Wt
    cfg = C.tiny_llm()
    _on_off(cfg, Wt.SyntheticLLM(cfg), (1, 255, 256, 257), 288)


def test_greedy_decode_at_the_0p5b_widths_is_bit_equal():
    """Two layers at the 0.5B widths (hidden 896: the k_lm_screen form the product runs, 14 k tiles of 64) with a vocabulary of
    16 411 -- 1 026 tiles, more than the blocks' waves take in two rounds, V no multiple of 16 -- so that packing the weights
    stays at a few seconds; the full vocabulary runs in bench.py's output check."""
    from sparkmi import weights as Wt
    cfg = C.LLMConfig(vocab_size=16411, num_hidden_layers=2)
    _on_off(cfg, Wt.SyntheticLLM(cfg), (1, 255, 256, 257), 288)
