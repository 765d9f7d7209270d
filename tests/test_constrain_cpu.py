"""Host side of the allowed-token constraints (smi_llm_admit_constrained): the torch restatement of stage 0
(tests/constrain_ref.py) against transformers' SuppressTokensLogitsProcessor, the id -> run merging and its errors, the
ctypes record against include/sparkmi.h, and the speech_tokens_only set of a synthetic tokenizer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from constrain_ref import allow_mask, constrain, process
from penalty_ref import history, penalize
from sparkmi import _lib
from sparkmi.llm import ALLOW_KEY, allow_ranges, allow_records, sampling_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.95)


@pytest.mark.parametrize("vocab", [1003, 166000])
def test_stage0_is_bit_equal_to_suppress_tokens(vocab):
    from transformers import SuppressTokensLogitsProcessor
    rng = np.random.Generator(np.random.PCG64(vocab))
    cases = [[(0, 5)], [(vocab - 1, vocab)], [(3, 40), (41, 42), (500, 900)], [(vocab // 2, vocab)]]
    for runs in cases:
        x = torch.from_numpy((rng.standard_normal(vocab) * 3.0).astype(np.float32))
        keep = allow_mask(vocab, runs)
        proc = SuppressTokensLogitsProcessor(torch.nonzero(~keep).flatten().tolist())
        want = proc(torch.zeros((1, 1), dtype=torch.long), x[None].clone())[0]
        got = constrain(x, runs)
        assert torch.equal(got, want), runs
        assert torch.isinf(got[~keep]).all() and torch.equal(got[keep], x[keep])


def test_stage0_comes_before_the_penalties():
    rng = np.random.Generator(np.random.PCG64(3))
    V = 1003
    x = torch.from_numpy(rng.standard_normal(V).astype(np.float32))
    runs = [(10, 60), (700, 720)]
    hist = history(V, [11, 12, 701], [13, 13, 705])
    rec = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.5, min_new_tokens=4)
    got = process(x, runs, hist, rec, 2, [15])
    want = penalize(constrain(x, runs), hist, rec, 2, [15])
    assert torch.equal(got, want)
    assert torch.isinf(got[~allow_mask(V, runs)]).all() and got[15] == -float("inf")


def test_ids_merge_into_sorted_runs():
    assert allow_ranges([5, 3, 4, 9, 3, 10, 0], 20) == [(0, 1), (3, 6), (9, 11)]
    assert allow_ranges(range(151643, 166000), 166000) == [(151643, 166000)]
    assert allow_ranges(np.arange(7, 9, dtype=np.int64), 10) == [(7, 9)]
    assert allow_ranges(iter([2]), 3) == [(2, 3)]
    assert allow_ranges(list(range(0, 32, 2)), 32) == [(i, i + 1) for i in range(0, 32, 2)]   # 16 runs: the most


@pytest.mark.parametrize("ids, msg", [
    ([], "empty"),
    ([3, 40], "outside"),
    ([-1], "outside"),
    (list(range(0, 34, 2)), "at most 16"),
    ([1.5], "not an integer"),
    ([True], "not an integer"),
    ("abc", "iterable"),
    (7, "iterable"),
])
def test_bad_sets_are_refused(ids, msg):
    with pytest.raises(ValueError, match=msg):
        allow_ranges(ids, 40)
    with pytest.raises(ValueError, match=msg):
        allow_records([{ALLOW_KEY: ids}], 1, 40)


def test_records_from_request_dicts():
    assert allow_records(None, 2, 100) is None
    assert allow_records([None, {"do_sample": True}], 2, 100) is None        # no request carries the key: the old route
    assert allow_records([{ALLOW_KEY: None}], 1, 100) is None
    recs = allow_records([None, {ALLOW_KEY: [50, 51, 52, 90]}, {ALLOW_KEY: range(100)}], 3, 100)
    assert recs[0].n_ranges == 0 and recs[0].reserved == 0
    assert recs[1].n_ranges == 2 and list(recs[1].lo[:2]) == [50, 90] and list(recs[1].hi[:2]) == [53, 91]
    assert recs[2].n_ranges == 1 and (recs[2].lo[0], recs[2].hi[0]) == (0, 100)   # neutral: the library keeps the old route
    with pytest.raises(ValueError, match="2 entries for 3"):
        allow_records([None, None], 3, 100)
    # the key alone leaves token selection to the handle, and is a known key
    assert sampling_records([{ALLOW_KEY: [1]}], 1, HANDLE) is None


def test_forked_takes_share_a_one_shot_set():
    from sparkmi.llm import expand_takes
    takes = expand_takes([{ALLOW_KEY: iter([4, 5, 6])}, None], [3, 1])
    assert [t[ALLOW_KEY] for t in takes[:3]] == [(4, 5, 6)] * 3 and takes[3] is None


def test_allow_record_layout_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "sparkmi.h")).read()
    assert re.search(r"#define SMI_MAX_ALLOW_RANGES 16\b", txt)
    body = re.search(r"typedef struct smi_allow_params \{(.*?)\} smi_allow_params;", txt, re.S).group(1)
    fields = re.findall(r"int32_t (\w+)(?:\[SMI_MAX_ALLOW_RANGES\])?;", body)
    assert fields == ["n_ranges", "reserved", "lo", "hi"]
    assert [f[0] for f in _lib.AllowParams._fields_] == fields
    assert ctypes.sizeof(_lib.AllowParams) == 8 + 2 * 16 * 4
    assert _lib.AllowParams.lo.offset == 8 and _lib.AllowParams.hi.offset == 72
    assert _lib.SMI_MAX_ALLOW_RANGES == 16
    assert "smi_llm_admit_constrained" in _lib.SYMBOLS
    assert re.search(r"#define SMI_ABI_VERSION 4\b", txt)


def test_speech_tokens_only_set_of_a_synthetic_tokenizer(tmp_path):
    from transformers import AutoTokenizer
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS, SPEECH_ONLY_KEY, _request_sampling
    synthetic.make_model_dir(tmp_path, with_prompt_encoder=False)
    tok = AutoTokenizer.from_pretrained(str(tmp_path / "LLM"))
    eos = [int(tok.eos_token_id)]
    fake = SparkTTS.__new__(SparkTTS)            # the set needs the tokenizer and the eos list alone
    fake.tokenizer, fake._eos = tok, eos
    got = fake.speech_token_ids()
    want = sorted(set(tok.get_added_vocab().values()) | set(eos))
    assert got == want
    text_ids = set(range(len(tok))) - set(tok.get_added_vocab().values())
    assert text_ids and not (set(got) & text_ids - set(eos))
    d = _request_sampling({SPEECH_ONLY_KEY: True}, fake.speech_token_ids)
    assert list(d[ALLOW_KEY]) == want
    d = _request_sampling({SPEECH_ONLY_KEY: True, ALLOW_KEY: [0, 1, want[0], want[3]]}, fake.speech_token_ids)
    assert list(d[ALLOW_KEY]) == [want[0], want[3]]                 # both: their intersection
    assert _request_sampling({SPEECH_ONLY_KEY: False}, fake.speech_token_ids) is None
    with pytest.raises(ValueError, match="bool"):
        _request_sampling({SPEECH_ONLY_KEY: 1}, fake.speech_token_ids)
