"""Host side of the per-token log-probabilities (smi_llm_admit_logprobs): the float64 restatement (tests/logprob_ref.py)
against transformers' processors + log_softmax (tests/golden/logprob.npz), the exported symbols and their ctypes
signatures, and the request-key -> flag resolution of SparkLLM.admit / generate_ragged / serve and SparkTTS."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from logprob_ref import fixture_rows, logprob, log_softmax64
from penalty_ref import history, penalize
from sparkmi import _lib
from sparkmi.llm import LOGPROB_KEYS, PENALTY_KEYS, SAMPLING_KEYS, logprob_flags, penalty_records, sampling_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95)


def test_restatement_matches_transformers(golden_dir):
    g = np.load(os.path.join(golden_dir, "logprob.npz"))
    seen = set()
    for name, z, T, ids, lp in fixture_rows(golden_dir):
        got = log_softmax64(z, T)[ids]
        fin = np.isfinite(lp)
        assert np.array_equal(np.isfinite(got), fin), name
        assert (got[~fin] == lp[~fin]).all(), name
        assert np.abs(got[fin] - lp[fin]).max() <= 1e-6, name
        assert logprob(z, ids[0], T) == pytest.approx(float(lp[0]), abs=1e-6)
        # z is what the penalties of tests/penalty_ref.py (the kernel's restatement) make of the raw row
        V, seed = int(g[f"{name}.V"]), int(g[f"{name}.seed"])
        x = (np.random.Generator(np.random.PCG64(seed)).standard_normal(V) * 3.0).astype(np.float32)
        r = float(g[f"{name}.params"][0])
        gen, neg = g[f"{name}.gen"].tolist(), g[f"{name}.neg_inf"].tolist()
        rec = dict(repetition_penalty=r, min_new_tokens=len(gen) + 1 if neg else 0)
        zz = penalize(torch.from_numpy(x), history(V, g[f"{name}.prompt"].tolist(), gen), rec, len(gen), neg).numpy()
        assert np.array_equal(zz.view(np.uint32), z.view(np.uint32)), name
        seen.add(name)
    assert {"greedy", "t03", "t08_rep", "t17_eos_masked", "big_greedy", "big_t03", "big_t08_rep", "big_t17_eos_masked"} <= seen
    temps = {float(g[f"{n}.params"][1]) for n in seen}
    assert {0.3, 0.8, 1.7} <= temps


def test_exported_symbols_and_signatures():
    l = _lib.lib()
    for name in ("smi_llm_admit_logprobs", "smi_llm_slots_logprobs"):
        assert hasattr(l, name), name
        assert name in _lib.SYMBOLS
    res, args = _lib.SYMBOLS["smi_llm_admit_logprobs"]
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int,
                    ctypes.POINTER(_lib.SampleParams), ctypes.POINTER(_lib.PenaltyParams), ctypes.POINTER(ctypes.c_int32),
                    ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    res, args = _lib.SYMBOLS["smi_llm_slots_logprobs"]
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                    ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p]
    assert "smi_llm_debug_logprob" in _lib.DEBUG_SYMBOLS
    txt = open(os.path.join(ROOT, "include", "sparkmi.h")).read()
    assert re.search(r"int smi_llm_admit_logprobs\(smi_llm\* h, const int64_t\* ids_host, const int32_t\* lens_host, int n, int P_max,"
                     r"\s+const smi_sample_params\* params, const smi_penalty_params\* pens, const int32_t\* return_log_probs,"
                     r"\s+int32_t\* slots_out, void\* stream\);", txt)
    assert re.search(r"int smi_llm_slots_logprobs\(smi_llm\* h, const int32_t\* slots, int n, float\* out_host, int cap, "
                     r"int32_t\* n_out, void\* stream\);", txt)
    assert "not provided" in txt and "TemperatureLogitsWarper" in txt
    dbg = open(os.path.join(ROOT, "include", "sparkmi_debug.h")).read()
    assert "int smi_llm_debug_logprob(" in dbg


def test_entry_points_check_their_arguments():
    l = _lib.lib()
    slots = (ctypes.c_int32 * 1)()
    assert l.smi_llm_admit_logprobs(None, None, None, 1, 1, None, None, None, slots, None) == -1
    assert b"null" in l.smi_last_error()
    out = (ctypes.c_float * 4)()
    n = (ctypes.c_int32 * 1)()
    assert l.smi_llm_slots_logprobs(None, slots, 1, out, 4, n, None) == -1


def test_flags_from_request_dicts():
    assert logprob_flags(None, 2) is None
    assert logprob_flags([None, {"do_sample": True}, {"repetition_penalty": 1.2}], 3) is None   # no key: the old route
    f = logprob_flags([{"return_log_probs": True}, None, {"return_log_probs": False, "seed": 3}], 3)
    assert f.dtype == np.int32 and f.tolist() == [1, 0, 0]
    assert logprob_flags([{"return_log_probs": np.bool_(True)}], 1).tolist() == [1]
    with pytest.raises(ValueError):
        logprob_flags([None], 2)
    assert LOGPROB_KEYS == ("return_log_probs",)
    assert not set(LOGPROB_KEYS) & (set(SAMPLING_KEYS) | set(PENALTY_KEYS))


@pytest.mark.parametrize("bad", [1, 0, "yes", None, 1.0, [True]])
def test_a_non_bool_flag_is_refused_before_any_device_call(bad):
    with pytest.raises(ValueError):
        logprob_flags([{"return_log_probs": True}, {"return_log_probs": bad}], 2)
    from sparkmi.pipeline import _request_sampling
    with pytest.raises(ValueError):
        _request_sampling(dict(text="hi", return_log_probs=bad))


def test_the_flag_leaves_selection_and_penalties_alone():
    assert sampling_records([{"return_log_probs": True}], 1, HANDLE) is None          # inherit
    assert penalty_records([{"return_log_probs": True}], 1) is None                   # unpenalised
    recs = sampling_records([{"return_log_probs": True, "seed": 4}, {"return_log_probs": False}], 2, HANDLE)
    assert recs[0].mode == _lib.SAMPLING_SAMPLE and recs[0].has_seed == 1 and recs[1].mode == _lib.SAMPLING_INHERIT
    with pytest.raises(ValueError):
        sampling_records([{"return_log_prob": True}], 1, HANDLE)                     # misspelt: unknown key


def test_pipeline_route_and_signatures():
    from sparkmi.llm import SparkLLM
    from sparkmi.pipeline import SparkTTS, _lp_info, _request_sampling
    assert _request_sampling(dict(text="hi", return_log_probs=False)) is None        # today's route
    assert _request_sampling(dict(text="hi", return_log_probs=True)) == {"return_log_probs": True}
    for f in (SparkTTS.inference, SparkTTS.inference_batch, SparkTTS.serve):
        p = inspect.signature(f).parameters["return_log_probs"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, f.__name__
    for f in (SparkLLM.generate_ragged, SparkLLM.serve):
        assert inspect.signature(f).parameters["return_log_probs"].default is False
    info = _lp_info([5, 6, 7], np.array([-0.5, -1.25, -2.0], dtype=np.float32))
    assert info["token_ids"] == [5, 6, 7] and info["output_log_probs"].dtype == np.float32
    assert isinstance(info["cum_log_prob"], float) and info["cum_log_prob"] == -3.75
