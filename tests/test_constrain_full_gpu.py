"""Allowed-token constraints at the 0.5B shape, bf16 cache, paged and contiguous: 1, 16, 17, 32, 33 and 64 rows, every row
constrained to several ranges (the restricted lm_head: k_lm<1>, k_lm32, two k_lm32 passes), each row equal to its solo run
and to its run beside an unconstrained row (the full lm_head); one sampled row with the same bits on both paths."""
import numpy as np
import pytest

from sparkmi.llm import ALLOW_KEY

pytestmark = pytest.mark.gpu

N = 12


def _runs(V, b):
    """Four ranges per row: the speech block above the BPE ids, and three narrow ones that differ from row to row."""
    a = 1000 + 977 * b
    return [(a, a + 40), (a + 3000, a + 3003), (151643 + 11 * b, 151643 + 11 * b + 700), (165000 - 5 * b, 165100 - 5 * b)]


def _ids(runs):
    return [i for lo, hi in runs for i in range(lo, hi)]


@pytest.mark.parametrize("paged", [False, True])
def test_every_row_count_equals_its_solo_and_its_mixed_run(full_llm, paged):
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, _, arena = full_llm
    V = cfg.vocab_size
    rng = np.random.Generator(np.random.PCG64(4100))
    prompts = [rng.integers(0, 151643, size=int(rng.integers(3, 40))).tolist() for _ in range(64)]
    recs = [{ALLOW_KEY: _ids(_runs(V, b))} for b in range(64)]
    extra = dict(kv_page_tokens=64, kv_pages=64 * 2) if paged else {}
    one = SparkLLM(cfg, None, "cuda:0", max_slots=2, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16", **extra)
    solo = [one.generate_ragged([prompts[b]], [N], sampling=[recs[b]])[0] for b in range(64)]
    free = rng.integers(0, 151643, size=17).tolist()
    for b in range(64):
        assert all(t in set(_ids(_runs(V, b))) for t in solo[b]), b
        mixed = one.generate_ragged([prompts[b], free], [N, N], sampling=[recs[b], None])
        assert mixed[0] == solo[b], f"row {b}: the full lm_head + stage 0 differs from the restricted one"
    many = SparkLLM(cfg, None, "cuda:0", max_slots=64, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16", **extra)
    for M in (1, 16, 17, 32, 33, 64):
        got = many.generate_ragged(prompts[:M], [N] * M, sampling=recs[:M])
        differ = [b for b in range(M) if got[b] != solo[b]]
        assert differ == [], f"{M} rows: rows that differ from their solo run: {differ}"


def test_a_sampled_row_has_the_same_bits_on_both_paths(full_llm):
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, _, arena = full_llm
    V = cfg.vocab_size
    rng = np.random.Generator(np.random.PCG64(4200))
    p, q = (rng.integers(0, 151643, size=30).tolist() for _ in range(2))
    rec = {ALLOW_KEY: range(151643, 166000), "do_sample": True, "temperature": 0.8, "top_k": 50, "top_p": 0.95, "seed": 77,
           "return_log_probs": True}
    llm = SparkLLM(cfg, None, "cuda:0", max_slots=2, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    alone = llm.generate_ragged([p], [20], sampling=[rec])[0]
    mixed = llm.generate_ragged([p, q], [20, 20], sampling=[rec, None])[0]
    assert alone[0] == mixed[0] and np.array_equal(alone[1], mixed[1])
    assert all(151643 <= t < 166000 for t in alone[0]) and np.isfinite(alone[1]).all()
