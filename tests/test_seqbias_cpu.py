"""Sequence bias, banned and stop sequences (smi_llm_admit_biased) without a GPU: the restatement (tests/seqbias_ref.py) against
the transformers fixture bit for bit, the packing of smi_seq_params and every field it refuses, the survivor rule with
allowed_token_ids and min_new_tokens, and expand_takes."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from seqbias_ref import apply_bias, applies, bias_totals, stop_met
from sparkmi import _lib
from sparkmi.llm import ALLOW_KEY, SEQ_KEYS, expand_takes, sampling_records, seq_entries, seq_records

GOLD = Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("gen_golden_seqbias", GOLD / "gen_golden_seqbias.py")
NINF = float("-inf")


def logits_row(seed, V):   # the generator's own rule (the module imports transformers at load; this is its two lines)
    return (np.random.Generator(np.random.PCG64(seed)).standard_normal(V) * 3.0).astype(np.float32)


def fixture_rows():
    d = np.load(GOLD / "seqbias.npz")
    for r in range(int(d["n_rows"])):
        k = f"r{r}_"
        ent = [(tuple(int(v) for v in ids[:n]), float(b)) for ids, n, b in zip(d[k + "ids"], d[k + "len"], d[k + "bias"])]
        yield dict(r=r, V=int(d[k + "V"]), seed=int(d[k + "seed"]), plen=int(d[k + "plen"]), ctx=d[k + "ctx"].tolist(), entries=ent,
                   chain=int(d[k + "chain"]), par=float(d[k + "par"]), stage=d[k + "stage"], final=d[k + "final"],
                   probe=d[k + "probe"] if k + "probe" in d else None, argmax=d[k + "argmax"].tolist())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_the_fixture_covers_both_vocabularies_and_the_generator_rule_is_the_one_used():
    rows = list(fixture_rows())
    assert {r["V"] for r in rows} == {1003, 166000} and len(rows) == 16
    src = (GOLD / "gen_golden_seqbias.py").read_text()
    assert "standard_normal(V) * 3.0).astype(np.float32)" in src and "np.random.PCG64(seed)" in src


@pytest.mark.parametrize("row", list(fixture_rows()), ids=lambda r: f"r{r['r']}-V{r['V']}")
def test_the_restatement_equals_transformers_bit_for_bit(row):
    x = logits_row(row["seed"], row["V"])
    stage = apply_bias(x, row["ctx"], row["entries"])
    final = stage
    if row["chain"] == 1:     # RepetitionPenaltyLogitsProcessor on the context ids
        t = torch.from_numpy(stage.copy())
        ids = torch.tensor(sorted(set(row["ctx"])), dtype=torch.long)
        rep = torch.tensor(row["par"], dtype=torch.float32)
        t[ids] = torch.where(t[ids] < 0, t[ids] * rep, t[ids] / rep)
        final = t.numpy()
    elif row["chain"] == 2:   # TemperatureLogitsWarper, log_softmax
        final = torch.log_softmax(torch.from_numpy(stage.copy()) / row["par"], dim=-1).numpy()
    probe = slice(None) if row["probe"] is None else row["probe"]
    assert np.array_equal(_bits(stage[probe]), _bits(row["stage"]))
    assert np.array_equal(_bits(final[probe]), _bits(row["final"]))
    assert [int(np.argmax(stage)), int(np.argmax(final))] == row["argmax"]
    touched = set(bias_totals(row["ctx"], row["entries"]))
    keep = np.ones(row["V"], dtype=bool)
    keep[list(touched)] = False
    assert np.array_equal(_bits(stage[keep]), _bits(x[keep])), "only the ids an applying entry ends in change"


def test_matching_rules():
    assert applies([], (4,)) and applies([1, 2], (2, 9)) and not applies([1, 2], (1, 9))
    assert not applies([2], (1, 2, 9)), "an entry as long as the context + 1 is too long (transformers' rule: L <= len(ctx))"
    assert applies([7, 1, 2], (1, 2, 9)) and not applies([1, 2], (1, 2, 9))
    t = bias_totals([9, 3, 4], [((4, 8), 1e8), ((3, 4, 8), 1.0), ((8,), -1e8)])
    assert t == {8: np.float32(1.0)}, "length-1 first, then record order"


def test_stop_match():
    assert stop_met([5], [[5]]) and not stop_met([5, 6], [[5]])
    assert stop_met([1, 5, 6], [[9], [5, 6]]) and not stop_met([6], [[5, 6]])
    assert stop_met([4, 5, 6], [[4, 5, 6]]) and not stop_met([4, 5, 6], [[4, 5, 6]], min_new=4)
    assert stop_met([4, 5, 6], [[4, 5, 6]], min_new=3)


def _req(**kw):
    return [dict(kw)]


def test_packing():
    assert seq_records(None, 2, 100) is None
    assert seq_records([None, {"temperature": 0.5}], 2, 100) is None, "no key: the admission keeps its route"
    recs = seq_records([{"sequence_bias": [((3, 4), 1.5), ([7], NINF)], "bad_words_ids": [[9, 9, 2]], "stop_sequences": [[5], (6, 7, 8)]},
                        None], 2, 100)
    assert isinstance(recs[0], _lib.SeqParams) and len(recs) == 2
    r = recs[0]
    assert (r.n_bias, r.n_stop) == (3, 2) and list(r.bias_len[:3]) == [2, 1, 3] and list(r.stop_len[:2]) == [1, 3]
    assert r.bias[0] == 1.5 and r.bias[1] == NINF and r.bias[2] == NINF
    L = _lib.SMI_MAX_SEQ_LEN
    assert list(r.bias_ids[0:2]) == [3, 4] and r.bias_ids[L] == 7 and list(r.bias_ids[2 * L:2 * L + 3]) == [9, 9, 2]
    assert r.stop_ids[0] == 5 and list(r.stop_ids[L:L + 3]) == [6, 7, 8]
    assert (recs[1].n_bias, recs[1].n_stop) == (0, 0) and list(r.reserved) == [0, 0]
    import ctypes
    assert ctypes.sizeof(_lib.SeqParams) == 4 * (2 + 32 + 32 + 256 + 8 + 64 + 2)
    # the new keys are known to the sampling records (and alone they leave the token selection to the handle)
    assert sampling_records([{k: [] for k in SEQ_KEYS}], 1, dict(do_sample=False, temperature=1.0, top_k=1, top_p=1.0)) is None


@pytest.mark.parametrize("bad", [
    {"sequence_bias": [((3, 4), float("nan"))]},
    {"sequence_bias": [((3, 4), float("inf"))]},
    {"sequence_bias": [((3, 4), "1.0")]},
    {"sequence_bias": [((3, 4), True)]},
    {"sequence_bias": [(3, 4, 1.0)]},
    {"sequence_bias": {(3, 4): 1.0}},
    {"sequence_bias": [((), 1.0)]},
    {"sequence_bias": [(tuple(range(9)), 1.0)]},
    {"sequence_bias": [((3, 100), 1.0)]},
    {"sequence_bias": [((-1,), 1.0)]},
    {"sequence_bias": [((3.0,), 1.0)]},
    {"sequence_bias": [((3, 4), 1.0), ((3, 4), 2.0)]},
    {"sequence_bias": [((3, 4), 1.0)], "bad_words_ids": [[3, 4]]},
    {"sequence_bias": [((i,), 1.0) for i in range(33)]},
    {"sequence_bias": [((i,), 1.0) for i in range(20)], "bad_words_ids": [[i, 1] for i in range(13)]},
    {"bad_words_ids": [5]},
    {"bad_words_ids": "abc"},
    {"bad_words_ids": [[]]},
    {"bad_words_ids": [[True]]},
    {"stop_sequences": [[5], [5]]},
    {"stop_sequences": [[100]]},
    {"stop_sequences": [[1]] * 0 + [[i] for i in range(9)]},
    {"stop_sequences": [list(range(9))]},
    {"stop_sequences": 7},
])
def test_every_invalid_field_is_refused_on_the_host(bad):
    with pytest.raises(ValueError):
        seq_records([bad], 1, 100)


def test_counts_must_match_and_limits_hold_exactly():
    with pytest.raises(ValueError):
        seq_records([{"stop_sequences": [[1]]}], 2, 100)
    ok = seq_records([{"sequence_bias": [((i,), 1.0) for i in range(32)], "stop_sequences": [[i] * 8 for i in range(8)]}], 1, 100)
    assert (ok[0].n_bias, ok[0].n_stop) == (32, 8)
    b, s = seq_entries({"sequence_bias": [([1, 2], -0.5)], "bad_words_ids": [[3]]}, 10)
    assert b == [((1, 2), np.float32(-0.5)), ((3,), np.float32(NINF))] and s == []


def test_survivor_rule_with_the_allowed_set_and_min_new_tokens():
    V = 40
    ban_all = {"bad_words_ids": [[i] for i in range(30)], ALLOW_KEY: list(range(30))}
    with pytest.raises(ValueError):
        seq_records([ban_all], 1, V)
    # the last id of a LONGER -inf entry counts too (a conservative static bound)
    with pytest.raises(ValueError):
        seq_records([{"bad_words_ids": [[7, 3], [8, 4]], ALLOW_KEY: [3, 4]}], 1, V)
    assert seq_records([{"bad_words_ids": [[7, 3], [8, 4]], ALLOW_KEY: [3, 4, 5]}], 1, V) is not None
    # banned ids outside the set do not count against it
    assert seq_records([{"bad_words_ids": [[i] for i in range(10, 30)], ALLOW_KEY: [3]}], 1, V) is not None
    # min_new_tokens: a survivor that is not an eos id
    left_eos = {"bad_words_ids": [[3], [4]], ALLOW_KEY: [3, 4, 5]}
    assert seq_records([left_eos], 1, V, eos_ids=[5]) is not None
    with pytest.raises(ValueError):
        seq_records([dict(left_eos, min_new_tokens=2)], 1, V, eos_ids=[5])
    assert seq_records([dict(left_eos, min_new_tokens=2)], 1, V, eos_ids=[6]) is not None
    # without an allowed set the whole vocabulary is the set
    assert seq_records([{"bad_words_ids": [[i] for i in range(32)]}], 1, V) is not None
    with pytest.raises(ValueError):
        seq_records([{"bad_words_ids": [[i] for i in range(2)], "min_new_tokens": 1}], 1, 3, eos_ids=[2])
    # finite biases never count
    assert seq_records([{"sequence_bias": [((3,), -1e30), ((4,), -1e30)], ALLOW_KEY: [3, 4]}], 1, V) is not None


def test_expand_takes_carries_the_record_to_every_take():
    d = {"sequence_bias": iter([((3, 4), 1.5)]), "bad_words_ids": [[9]], "stop_sequences": ([5],), "seed": 7}
    takes = expand_takes([d, None], [3, 1])
    assert len(takes) == 4 and takes[3] is None
    for j, t in enumerate(takes[:3]):
        assert list(t["sequence_bias"]) == [((3, 4), 1.5)] and t["bad_words_ids"] == [[9]] and t["stop_sequences"] == ([5],)
        assert t["seed"] == 7 + j
    recs = seq_records(takes, 4, 100)
    assert [(r.n_bias, r.n_stop) for r in recs] == [(2, 1)] * 3 + [(0, 0)]
