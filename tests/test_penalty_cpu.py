"""Host side of the per-request logits penalties: the torch restatement (tests/penalty_ref.py) against transformers' own
processors (tests/golden/penalty.npz), the ctypes record against include/sparkmi.h, the dict -> record resolution of
SparkLLM.admit / generate_ragged / serve, and the route SparkTTS gives a request with penalty keys."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from penalty_ref import history, penalize
from sparkmi import _lib
from sparkmi.llm import PENALTY_KEYS, SAMPLING_KEYS, penalty_records, sampling_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95)


def fixture_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "penalty.npz"))
    for name in g["names"]:
        name = str(name)
        V, seed = int(g[f"{name}.V"]), int(g[f"{name}.seed"])
        if f"{name}.logits" in g:
            x, y = g[f"{name}.logits"], g[f"{name}.out"]
        else:
            x = (np.random.Generator(np.random.PCG64(seed)).standard_normal(V) * 2.0).astype(np.float32)
            x[::97] = 0.0
            y = x.copy()
            y[g[f"{name}.ids"]] = g[f"{name}.vals"]
        r, p, f, n, pp = g[f"{name}.params"]
        rec = dict(repetition_penalty=float(r), presence_penalty=float(p), frequency_penalty=float(f),
                   min_new_tokens=int(n), penalize_prompt=bool(pp))
        gen = g[f"{name}.gen"].tolist()
        yield name, x, y, history(V, g[f"{name}.prompt"].tolist(), gen), rec, len(gen), g[f"{name}.eos"].tolist()


def test_restatement_is_bit_equal_to_transformers(golden_dir):
    seen = set()
    for name, x, y, hist, rec, emitted, eos in fixture_cases(golden_dir):
        got = penalize(torch.from_numpy(x), hist, rec, emitted, eos).numpy()
        assert np.array_equal(got.view(np.uint32), y.view(np.uint32)), name
        assert int(np.argmax(got)) == int(torch.argmax(torch.from_numpy(y))), name
        seen.add(name)
        if name == "argmax_moves":
            assert int(np.argmax(x)) != int(np.argmax(y))
    assert {"rep_prompt", "rep_gen_only", "additive", "min_below", "min_at", "min_above", "big_all"} <= seen


def test_penalty_record_layout_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "sparkmi.h")).read()
    body = re.search(r"typedef struct smi_penalty_params \{(.*?)\} smi_penalty_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|float) (\w+)(\[3\])?;", body)
    assert [f for _, f, _ in fields] == [f for f, _ in _lib.PenaltyParams._fields_]
    assert ctypes.sizeof(_lib.PenaltyParams) == 32 and _lib.PenaltyParams.min_new_tokens.offset == 12
    assert ctypes.sizeof(_lib.SampleParams) == 32   # unchanged


def test_neutral_or_missing_keys_give_no_record():
    assert penalty_records(None, 2) is None
    assert penalty_records([None, {"do_sample": True}], 2) is None
    assert penalty_records([dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0,
                                 penalize_prompt=False)], 1) is None


def test_penalty_dicts_resolve_to_records():
    recs = penalty_records([{"repetition_penalty": 1.3}, None, {"min_new_tokens": 4, "penalize_prompt": False, "seed": 3},
                            {"presence_penalty": 0.5, "frequency_penalty": -0.25, "top_k": 5}], 4)
    a, b, c, d = recs
    assert a.repetition_penalty == pytest.approx(1.3) and a.penalize_prompt == 1 and a.min_new_tokens == 0
    assert b.repetition_penalty == 1.0 and b.presence_penalty == 0.0 and b.min_new_tokens == 0   # neutral row
    assert c.min_new_tokens == 4 and c.penalize_prompt == 0 and c.repetition_penalty == 1.0
    assert d.presence_penalty == 0.5 and d.frequency_penalty == -0.25
    assert all(list(r.reserved) == [0, 0, 0] for r in recs)


def test_penalty_keys_alone_leave_selection_to_the_handle():
    assert sampling_records([{"repetition_penalty": 1.3}], 1, HANDLE) is None
    recs = sampling_records([{"repetition_penalty": 1.3}, {"seed": 3, "min_new_tokens": 2}], 2, HANDLE)
    assert recs[0].mode == _lib.SAMPLING_INHERIT and recs[1].mode == _lib.SAMPLING_SAMPLE and recs[1].has_seed == 1


def test_unknown_keys_are_refused():
    with pytest.raises(ValueError):
        sampling_records([{"repetition_penalty": 1.2, "repetiton_penalty": 1.3}], 1, HANDLE)
    with pytest.raises(ValueError):
        penalty_records([None], 2)
    assert set(PENALTY_KEYS) == {"repetition_penalty", "presence_penalty", "frequency_penalty", "min_new_tokens",
                                 "penalize_prompt"}
    assert not set(PENALTY_KEYS) & set(SAMPLING_KEYS)


def test_pipeline_route_for_penalty_keys():
    from sparkmi.pipeline import _request_sampling
    assert _request_sampling(dict(text="hi")) is None
    # neutral values: the request keeps the route of the same request without them
    assert _request_sampling(dict(text="hi", repetition_penalty=1.0, min_new_tokens=0, penalize_prompt=False)) is None
    assert _request_sampling(dict(text="hi", seed=5, presence_penalty=0.0)) == {"seed": 5}
    d = _request_sampling(dict(text="hi", repetition_penalty=1.2, penalize_prompt=False))
    assert d == {"repetition_penalty": 1.2, "penalize_prompt": False}
    assert penalty_records([d], 1)[0].penalize_prompt == 0


def test_inference_defaults_are_neutral():
    import inspect
    from sparkmi.llm import penalty_neutral
    from sparkmi.pipeline import SparkTTS
    sig = inspect.signature(SparkTTS.inference)
    kw = {k: sig.parameters[k].default for k in PENALTY_KEYS}
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in PENALTY_KEYS)
    assert kw["penalize_prompt"] is True and penalty_neutral(kw)


def test_admission_entry_point_checks_its_arguments():
    l = _lib.lib()
    slots = (ctypes.c_int32 * 1)()
    rc = l.smi_llm_admit_penalized(None, None, None, 1, 1, None, None, slots, None)
    assert rc == -1 and b"null" in l.smi_last_error()
