"""Host side of the per-request sampling records: the ctypes record against include/sparkmi.h, the dict -> record resolution
of SparkLLM.admit / generate_ragged / serve, the keys SparkTTS takes from a request dict."""
import ctypes
import os
import re

import pytest

from sparkmi import _lib
from sparkmi.llm import SAMPLING_KEYS, sampling_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95)


def test_record_layout_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "sparkmi.h")).read()
    for name, v in (("INHERIT", _lib.SAMPLING_INHERIT), ("GREEDY", _lib.SAMPLING_GREEDY), ("SAMPLE", _lib.SAMPLING_SAMPLE)):
        assert re.search(rf"#define SMI_SAMPLING_{name} {v}\b", txt), name
    body = re.search(r"typedef struct smi_sample_params \{(.*?)\} smi_sample_params;", txt, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|uint64_t|float) (\w+);", body)
    assert [f for _, f in fields] == [f for f, _ in _lib.SampleParams._fields_]
    size = {"int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float}
    for (t, f), (_, ct) in zip(fields, _lib.SampleParams._fields_):
        assert ctypes.sizeof(size[t]) == ctypes.sizeof(ct) and (t == "float") == (ct is ctypes.c_float), f
    assert ctypes.sizeof(_lib.SampleParams) == 32 and _lib.SampleParams.seed.offset == 16


def test_no_record_means_every_prompt_inherits():
    assert sampling_records(None, 3, HANDLE) is None
    assert sampling_records([None, None], 2, HANDLE) is None


def test_dicts_resolve_against_the_handle_settings():
    recs = sampling_records([{"do_sample": False, "seed": 4}, None, {"temperature": 1.3, "seed": -1},
                             {"top_k": 7, "top_p": 0.5}], 4, HANDLE)
    g, i, s, h = recs
    assert g.mode == _lib.SAMPLING_GREEDY and g.has_seed == 0
    assert i.mode == _lib.SAMPLING_INHERIT
    assert s.mode == _lib.SAMPLING_SAMPLE and s.temperature == pytest.approx(1.3) and s.top_k == 50
    assert s.top_p == pytest.approx(0.95) and s.has_seed == 1 and s.seed == 2 ** 64 - 1
    assert h.mode == _lib.SAMPLING_SAMPLE and h.top_k == 7 and h.top_p == pytest.approx(0.5) and h.has_seed == 0
    # a greedy handle: a dict without do_sample follows it
    assert sampling_records([{"seed": 3}], 1, dict(HANDLE, do_sample=False))[0].mode == _lib.SAMPLING_GREEDY


def test_bad_dicts_are_refused_before_the_library():
    with pytest.raises(ValueError):
        sampling_records([{"temperture": 0.5}], 1, HANDLE)
    with pytest.raises(ValueError):
        sampling_records([None], 2, HANDLE)


def test_request_dicts_carry_only_the_sampling_keys():
    from sparkmi.pipeline import _request_sampling
    assert _request_sampling(dict(text="hi", prompt_text=None)) is None
    assert _request_sampling(dict(text="hi", seed=5, top_k=3)) == {"seed": 5, "top_k": 3}
    assert set(SAMPLING_KEYS) == {"do_sample", "temperature", "top_k", "top_p", "seed"}


def test_admission_entry_point_checks_its_arguments():
    l = _lib.lib()
    slots = (ctypes.c_int32 * 1)()
    rc = l.smi_llm_admit_sampled(None, None, None, 1, 1, None, slots, None)
    assert rc == -1 and b"null" in l.smi_last_error()
