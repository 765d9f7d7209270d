"""no_repeat_ngram_size (smi_llm_admit_ngram) without a GPU: the restatement (tests/ngram_ref.py) against the transformers
fixture bit for bit, the request-key checks of sparkmi.llm and sparkmi.pipeline, expand_takes, and the CPU oracle's own run of
the prompts the GPU tests use."""
from pathlib import Path

import numpy as np
import pytest
import torch

from ngram_ref import apply_ngram, banned_ids, greedy_generate, repeats
from sparkmi import _lib
from sparkmi.llm import NGRAM_KEY, expand_takes, ngram_records, ngram_size, sampling_records
from sparkmi.pipeline import _request_sampling

GOLD = Path(__file__).resolve().parent / "golden"
GUARANTEE_SEED, REPLAY_SEED = 1059, 1059  # prompts of the GPU tests (tests/test_ngram_gpu.py)
CHAIN_PEN = {"repetition_penalty": 1.3}    # the penalties of the GPU tests' penalised replay


def logits_row(seed, V, holes=0):   # the generator's own rule (the module imports transformers at load)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(V) * 3.0).astype(np.float32)
    if holes:
        x[rng.integers(0, V, size=holes)] = -np.inf
    return x


def stage_input(row):
    """The row the stage gets: the seeded logits, behind the repetition penalty for a chained row."""
    x = logits_row(row["seed"], row["V"], row["holes"])
    if row["par"]:
        t = torch.from_numpy(x.copy())
        ids = torch.tensor(sorted(set(row["ctx"])), dtype=torch.long)
        rep = torch.tensor(row["par"], dtype=torch.float32)
        t[ids] = torch.where(t[ids] < 0, t[ids] * rep, t[ids] / rep)
        x = t.numpy()
    return x


def fixture_rows():
    d = np.load(GOLD / "ngram.npz")
    for r in range(int(d["n_rows"])):
        k = f"r{r}_"
        yield dict(r=r, V=int(d[k + "V"]), seed=int(d[k + "seed"]), holes=int(d[k + "holes"]), n=int(d[k + "n"]), ctx=d[k + "ctx"].tolist(),
                   par=float(d[k + "par"]), ninf=d[k + "ninf"], argmax=int(d[k + "argmax"]), out=d[k + "out"] if k + "out" in d else None)


def expected(row):
    """transformers' output row: the stage's input with -inf at the fixture's ids (the generator checked the rest bit for bit)."""
    out = stage_input(row)
    out[row["ninf"]] = -np.inf
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def gpu_prompt(seed, cfg):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, cfg.vocab_size, size=int(rng.integers(6, 30))).tolist()


def test_the_fixture_covers_what_the_issue_names():
    rows = list(fixture_rows())
    assert {r["V"] for r in rows} == {1003, 166000}
    assert {r["n"] for r in rows} == {1, 2, 3, 4, 8, 64}
    assert min(len(r["ctx"]) for r in rows) == 1 and max(len(r["ctx"]) for r in rows) == 300
    assert any(len(r["ctx"]) + 1 < r["n"] for r in rows) and any(r["holes"] for r in rows) and any(r["par"] for r in rows)
    assert sum(len(banned_ids(r["ctx"], r["n"])) > 0 for r in rows) >= len(rows) // 2, "matches are frequent"
    src = (GOLD / "gen_golden_ngram.py").read_text()
    assert "standard_normal(V) * 3.0).astype(np.float32)" in src and "x[rng.integers(0, V, size=holes)] = -np.inf" in src


@pytest.mark.parametrize("row", list(fixture_rows()), ids=lambda r: f"r{r['r']}-V{r['V']}-n{r['n']}")
def test_the_restatement_equals_transformers_bit_for_bit(row):
    x = stage_input(row)
    got = apply_ngram(x, row["ctx"], row["n"])
    assert np.array_equal(np.flatnonzero(np.isneginf(got)), row["ninf"])
    if row["out"] is not None:
        assert np.array_equal(_bits(got), _bits(row["out"]))
    assert int(np.argmax(got)) == row["argmax"]
    keep = ~np.isneginf(got)
    assert np.array_equal(_bits(got[keep]), _bits(x[keep])), "no finite logit moves"
    assert set(np.flatnonzero(np.isneginf(got) & ~np.isneginf(x)).tolist()) <= banned_ids(row["ctx"], row["n"])


def test_the_rule():
    assert banned_ids([5], 1) == {5} and banned_ids([], 1) == set()
    assert banned_ids([1, 2, 1], 2) == {2} and banned_ids([1], 2) == set() and banned_ids([1, 1], 2) == {1}
    assert banned_ids([7], 3) == set(), "L + 1 < n: nothing banned"
    assert banned_ids([1, 2, 3, 1, 2], 3) == {3} and banned_ids([1, 2, 3, 9, 2], 3) == set()
    assert banned_ids([4] * 63, 64) == set() and banned_ids([4] * 64, 64) == {4}
    assert banned_ids([1, 2], 0) == set()
    assert repeats([1, 2, 3, 1, 2, 3], 3) and not repeats([1, 2, 3, 1, 2, 4], 3)
    assert not repeats([1, 2, 3, 1, 2, 3, 9], 3, start=6), "only repeats that end at or after `start` count"


@pytest.mark.parametrize("bad", [True, False, -1, 65, 2.0, "3", np.bool_(True)])
def test_bad_values_are_refused_before_any_device_call(bad):
    with pytest.raises(ValueError):
        ngram_size(bad)
    with pytest.raises(ValueError):
        ngram_records([None, {NGRAM_KEY: bad}], 2)
    with pytest.raises(ValueError):
        _request_sampling({"text": "x", NGRAM_KEY: bad})


def test_ngram_records():
    assert ngram_records(None, 2) is None
    assert ngram_records([None, {"temperature": 0.5}], 2) is None, "no request asks for it: no record"
    assert ngram_records([{NGRAM_KEY: 0}, {NGRAM_KEY: None}], 2) is None, "0 is the neutral value"
    r = ngram_records([{NGRAM_KEY: 3}, None, {NGRAM_KEY: np.int64(64)}, {NGRAM_KEY: 0}], 4)
    assert r.dtype == np.int32 and r.tolist() == [3, 0, 64, 0]
    with pytest.raises(ValueError):
        ngram_records([{NGRAM_KEY: 3}], 2)
    assert _lib.SMI_MAX_NGRAM == 64
    # the key is a known key and selects nothing by itself
    assert sampling_records([{NGRAM_KEY: 3}], 1, dict(do_sample=False, temperature=1.0, top_k=1, top_p=1.0)) is None


def test_pipeline_request_key():
    assert _request_sampling({"text": "x"}) is None
    assert _request_sampling({"text": "x", NGRAM_KEY: 0}) is None, "0: the route of the request without the key"
    assert _request_sampling({"text": "x", NGRAM_KEY: 4}) == {NGRAM_KEY: 4}
    assert _request_sampling({"text": "x", NGRAM_KEY: 4, "temperature": 0.5}) == {NGRAM_KEY: 4, "temperature": 0.5}


def test_expand_takes_carries_the_key():
    out = expand_takes([{NGRAM_KEY: 3, "seed": 5}, None, {NGRAM_KEY: 2}], [2, 1, 3])
    assert [None if d is None else d[NGRAM_KEY] for d in out] == [3, 3, None, 2, 2, 2]
    assert [d["seed"] for d in out[:2]] == [5, 6]
    assert ngram_records(out, 6).tolist() == [3, 3, 0, 2, 2, 2]


def test_the_cpu_oracle_on_the_prompts_of_the_gpu_tests():
    """The guarantee test needs a prompt on which plain greedy decoding repeats a 3-gram; the replay test one on which at most
    10 % of the steps have their top two surviving logits within 1e-3."""
    from oracle.llm_ref import Qwen2Ref
    from sparkmi import config as C, weights as W
    cfg = C.tiny_llm()
    ref = Qwen2Ref(cfg, W.SyntheticLLM(cfg), kv_dtype="f32")
    p = gpu_prompt(GUARANTEE_SEED, cfg)
    assert len(p) + 96 <= 128
    plain = ref.generate_greedy(p, 96)
    assert repeats(p + plain, 3, len(p)), "the plain run repeats a 3-gram"
    assert not repeats(p + greedy_generate(ref, p, 96, 3), 3)
    one = greedy_generate(ref, p, 96, 1)
    assert len(set(p) | set(one)) == len(set(p)) + 96
    q = gpu_prompt(REPLAY_SEED, cfg)
    margins = []
    greedy_generate(ref, q, 64, 2, margins=margins)
    assert sum(m < 1e-3 for m in margins) <= 6
    margins = []
    assert not repeats(q + greedy_generate(ref, q, 64, 2, rec=CHAIN_PEN, margins=margins), 2)
    assert sum(m < 1e-3 for m in margins) <= 6


def test_the_inference_argument_is_checked_like_the_key():
    """``SparkTTS.inference(no_repeat_ngram_size=False)`` is refused as the request key refuses it (False == 0 is not "none")."""
    from sparkmi.pipeline import SparkTTS
    tts = SparkTTS.__new__(SparkTTS)
    tts._max_batch = 4
    for bad in (False, True, -1, 65, 2.0):
        with pytest.raises(ValueError, match=NGRAM_KEY):
            tts.inference("x", no_repeat_ngram_size=bad)
