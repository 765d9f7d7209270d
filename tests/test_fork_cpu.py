"""Host side of num_return_sequences (smi_llm_admit_forked): the exported symbol and its ctypes signature, the checks of the
takes count in SparkLLM.admit / serve and SparkTTS.inference / inference_batch / serve (all before any device call), and the
per-take expansion of the request records (a seeded take j draws with seed + j)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from sparkmi import _lib
from sparkmi.llm import FORK_KEY, LOGPROB_KEYS, PENALTY_KEYS, SAMPLING_KEYS, expand_takes, num_returns, sampling_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95)
BAD = [0, -1, -7, True, False, np.bool_(True), 1.0, 2.5, "2", None, [2]]


def test_exported_symbol_and_signature():
    l = _lib.lib()
    assert hasattr(l, "smi_llm_admit_forked") and "smi_llm_admit_forked" in _lib.SYMBOLS
    _, args = _lib.SYMBOLS["smi_llm_admit_forked"]
    P = ctypes.POINTER
    assert args == [ctypes.c_void_p, P(ctypes.c_int64), P(ctypes.c_int32), ctypes.c_int, ctypes.c_int, P(ctypes.c_int32),
                    P(_lib.SampleParams), P(_lib.PenaltyParams), P(ctypes.c_int32), P(ctypes.c_int32), ctypes.c_void_p]
    txt = open(os.path.join(ROOT, "include", "sparkmi.h")).read()
    assert re.search(r"int smi_llm_admit_forked\(smi_llm\* h, const int64_t\* ids_host, const int32_t\* lens_host, int n, int P_max,"
                     r"\s+const int32_t\* n_return, const smi_sample_params\* params, const smi_penalty_params\* pens,"
                     r"\s+const int32_t\* return_log_probs, int32_t\* slots_out, void\* stream\);", txt)
    assert l.smi_version() == 4   # additive ABI: no version bump


def test_entry_point_checks_its_arguments():
    l = _lib.lib()
    slots = (ctypes.c_int32 * 2)()
    nret = (ctypes.c_int32 * 1)(2)
    assert l.smi_llm_admit_forked(None, None, None, 1, 1, nret, None, None, None, slots, None) == -1
    assert b"null" in l.smi_last_error()


@pytest.mark.parametrize("bad", BAD, ids=repr)
def test_num_returns_refuses_what_is_not_a_count(bad):
    with pytest.raises(ValueError):
        num_returns(bad)


def test_num_returns_accepts_counts():
    assert num_returns(1) == 1 and num_returns(np.int64(5)) == 5 and num_returns(np.int32(3)) == 3


def test_seeded_takes_draw_seed_plus_j():
    s = [{"seed": 7, "temperature": 0.5}, None, {"do_sample": False, "repetition_penalty": 1.3}, {"seed": 2 ** 64 - 2}]
    t = expand_takes(s, [3, 2, 2, 3])
    assert len(t) == 10
    assert [d["seed"] for d in t[:3]] == [7, 8, 9] and all(d["temperature"] == 0.5 for d in t[:3])
    assert t[3] is None and t[4] is None
    assert t[5] == t[6] == s[2] and t[5] is not s[2]           # copied as is
    assert [d["seed"] for d in t[7:]] == [2 ** 64 - 2, 2 ** 64 - 1, 0]   # mod 2^64
    assert s[0]["seed"] == 7                                      # the caller's dicts are left alone
    assert expand_takes(None, [2, 3]) is None
    with pytest.raises(ValueError):
        expand_takes([None], [1, 1])
    recs = sampling_records(t, 10, HANDLE)
    assert [recs[j].seed for j in range(3)] == [7, 8, 9] and all(recs[j].has_seed == 1 for j in range(3))
    assert recs[3].mode == _lib.SAMPLING_INHERIT and recs[5].mode == _lib.SAMPLING_GREEDY
    assert [recs[j].seed for j in (7, 8, 9)] == [2 ** 64 - 2, 2 ** 64 - 1, 0]


def test_sampling_records_still_refuses_unknown_keys():
    assert FORK_KEY == "num_return_sequences"
    assert FORK_KEY not in SAMPLING_KEYS + PENALTY_KEYS + LOGPROB_KEYS
    with pytest.raises(ValueError):
        sampling_records([{FORK_KEY: 2}], 1, HANDLE)
    with pytest.raises(ValueError):
        sampling_records([{"num_return_sequence": 2, "seed": 1}], 1, HANDLE)


def _bare_llm(max_slots):
    """A SparkLLM with no handle and no library: any device call raises AttributeError, so a ValueError proves the check
    ran first."""
    from sparkmi.llm import SparkLLM
    llm = object.__new__(SparkLLM)
    llm.max_slots, llm.max_positions = max_slots, 128
    llm._sampling = dict(HANDLE)
    return llm


@pytest.mark.parametrize("bad", [0, -1, True, 1.5])
def test_llm_admit_checks_takes_before_any_device_call(bad):
    llm = _bare_llm(8)
    with pytest.raises(ValueError):
        llm.admit([[1, 2, 3], [4, 5]], None, n_return=[2, bad])
    with pytest.raises(ValueError):
        llm.generate_ragged([[1, 2, 3]], [4], n_return=[bad])


def test_llm_admit_refuses_more_takes_than_slots():
    llm = _bare_llm(4)
    with pytest.raises(ValueError):
        llm.admit([[1, 2, 3], [4, 5]], None, n_return=[3, 2])
    with pytest.raises(ValueError):
        llm.admit([[1, 2, 3]], None, n_return=[1, 1])          # one count per prompt
    with pytest.raises(ValueError):
        llm.generate_ragged([[1, 2], [3]], [4, 4], n_return=[4, 1])


@pytest.mark.parametrize("bad", [0, -2, True, 2.0])
def test_llm_serve_checks_takes_before_any_device_call(bad):
    llm = _bare_llm(4)
    with pytest.raises(ValueError):
        list(llm.serve([("a", [1, 2, 3], 4, None, {FORK_KEY: bad})]))
    with pytest.raises(ValueError):
        list(llm.serve([("a", [1, 2, 3], 4, None, {FORK_KEY: 5})]))            # more than max_live (= max_slots)
    with pytest.raises(ValueError):
        list(llm.serve([("a", [1, 2, 3], 4, None, {FORK_KEY: 3})], max_live=2))


def _bare_tts(max_batch):
    from sparkmi.pipeline import SparkTTS
    tts = object.__new__(SparkTTS)
    tts._max_batch, tts._max_positions = max_batch, 128
    return tts


@pytest.mark.parametrize("bad", [0, -1, True, np.bool_(True), 2.0, "3"])
def test_pipeline_checks_takes_before_any_device_call(bad):
    tts = _bare_tts(4)
    with pytest.raises(ValueError):
        tts.inference("hi", gender="female", pitch="moderate", speed="moderate", num_return_sequences=bad)
    with pytest.raises(ValueError):
        tts.inference_batch([dict(text="hi", gender="male"), dict(text="hi", gender="male", num_return_sequences=bad)])
    with pytest.raises(ValueError):
        list(tts.serve([dict(text="hi", gender="male", num_return_sequences=bad)]))


def test_pipeline_refuses_more_takes_than_max_batch():
    tts = _bare_tts(4)
    with pytest.raises(ValueError):
        tts.inference("hi", gender="female", num_return_sequences=5)
    with pytest.raises(ValueError):
        tts.inference_batch([dict(text="a", gender="male", num_return_sequences=3), dict(text="b", gender="male", num_return_sequences=2)])
    with pytest.raises(ValueError):
        list(tts.serve([dict(text="a", gender="male", num_return_sequences=5)]))


def test_signatures():
    from sparkmi.llm import SparkLLM
    from sparkmi.pipeline import SparkTTS, _request_sampling
    p = inspect.signature(SparkTTS.inference).parameters["num_return_sequences"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1
    for f in (SparkLLM.admit, SparkLLM.generate_ragged):
        assert inspect.signature(f).parameters["n_return"].default is None
    assert _request_sampling(dict(text="hi", num_return_sequences=3)) is None   # not a record key
