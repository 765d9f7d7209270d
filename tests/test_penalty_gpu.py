"""Per-request logits penalties (smi_llm_admit_penalized; TensorRT-LLM's per-request repetition_penalty / presence_penalty /
frequency_penalty / min_length inputs): k_penalize against transformers' processors bit for bit, greedy decoding against a
CPU oracle, penalised rows of any mix next to unpenalised ones without changing their bits, a bad record changes nothing."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle.llm_ref import Qwen2Ref
from oracle.sampling_ref import sampling_probs
from penalty_ref import greedy_generate
from sparkmi import config as C, weights as W
from test_penalty_cpu import fixture_cases

pytestmark = pytest.mark.gpu


def _llm(cfg, syn, **kw):
    from sparkmi.llm import SparkLLM
    kw.setdefault("diag", any(k.startswith("SPARKMI_") for k in os.environ))
    return SparkLLM(cfg, syn, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def tiny():
    cfg = C.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


def _prompts(cfg, seed, n, lo=3, hi=30):
    rng = np.random.Generator(np.random.PCG64(seed))
    return [rng.integers(0, cfg.vocab_size, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


# 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1003, 166000])   # the scalar path (V % 4 != 0) and the float4 path
def test_kernel_is_bit_equal_to_transformers(golden_dir, vocab):
    cfg = C.tiny_llm()
    if cfg.vocab_size != vocab:
        cfg = dataclasses.replace(cfg, vocab_size=vocab)
    llm = _llm(cfg, W.SyntheticLLM(cfg), max_slots=4, max_positions=256, diag=True)   # (min_new_tokens <= max_positions)
    n = 0
    for name, x, y, hist, rec, emitted, eos in fixture_cases(golden_dir):
        if len(x) != vocab:
            continue
        llm.session_begin(eos)
        for rows in (1, 3):   # one row, and the row among others (each row has its own history and record)
            got, am = llm.debug_penalize(np.stack([x] * rows), np.stack([hist] * rows), [rec] * rows, [emitted] * rows)
            for r in range(rows):
                bad = np.nonzero(got[r].view(np.uint32) != y.view(np.uint32))[0]
                assert bad.size == 0, f"{name}: {bad.size} logits differ, first id {bad[:5]}: {got[r][bad[:5]]} vs {y[bad[:5]]}"
                assert int(am[r]) == int(torch.argmax(torch.from_numpy(y))), name
        n += 1
    assert n >= 3


# 2 -------------------------------------------------------------------------------------------------------------------
def test_greedy_penalties_match_the_cpu_oracle(tiny):
    cfg, syn = tiny
    prompt = _prompts(cfg, 5, 1, 12, 13)[0]
    N = 64
    llm = _llm(cfg, syn, max_slots=2, max_positions=128, kv_dtype="f32")
    oracle = Qwen2Ref(cfg, syn, kv_dtype="f32")
    base = llm.generate_ragged([prompt], [N])[0]
    assert base == oracle.generate_greedy(prompt, N)
    assert len(set(base)) < len(base), "the unpenalised run must repeat tokens for this test to mean anything"
    for rec in (dict(repetition_penalty=1.3), dict(repetition_penalty=1.3, penalize_prompt=False),
                dict(presence_penalty=0.6, frequency_penalty=0.4), dict(presence_penalty=-0.5, frequency_penalty=1.5)):
        got = llm.generate_ragged([prompt], [N], sampling=[rec])[0]
        assert got == greedy_generate(oracle, prompt, N, rec), rec
        assert got != base, rec
    # min_new_tokens: the eos list is a token the unpenalised run emits early
    eos = [base[2]]
    stop = llm.generate_ragged([prompt], [N], eos)[0]
    assert len(stop) <= 3 and stop[-1] == eos[0]
    rec = dict(min_new_tokens=20)
    got = llm.generate_ragged([prompt], [N], eos, sampling=[rec])[0]
    assert got == greedy_generate(oracle, prompt, N, rec, eos)
    assert len(got) > 20 and eos[0] not in got[:20]


# 3 -------------------------------------------------------------------------------------------------------------------
RECORDS = [
    {"do_sample": False, "repetition_penalty": 1.3},                                                  # penalised greedy
    {"do_sample": True, "temperature": 0.8, "top_k": 40, "top_p": 0.95, "seed": 11,
     "presence_penalty": 0.5, "frequency_penalty": 0.3, "penalize_prompt": False},                    # penalised, seeded
    {"do_sample": False},                                                                             # plain greedy
    None,                                                                                             # inherit (greedy handle)
    {"repetition_penalty": 1.0, "presence_penalty": 0.0, "min_new_tokens": 0},                        # neutral record
    {"do_sample": False, "min_new_tokens": 12, "frequency_penalty": 0.4},                             # penalised greedy
    {"do_sample": True, "temperature": 1.1, "top_k": 256, "top_p": 1.0, "seed": 12, "repetition_penalty": 0.8},
    None,
]
PLAIN = (2, 3, 4, 7)


def _serve(llm, reqs, order, max_live, recs):
    llm.set_sampling(False)
    return dict(llm.serve(iter([reqs[i][:4] + (recs[i],) for i in order]), max_live=max_live, decode_stride=3))


def test_rows_are_independent_in_one_session(tiny):
    cfg, syn = tiny
    rng = np.random.Generator(np.random.PCG64(93))
    eos = [int(rng.integers(0, cfg.vocab_size))]
    reqs = [(i, p, int(rng.integers(12, 40)), eos) for i, p in enumerate(_prompts(cfg, 94, len(RECORDS)))]
    llm = _llm(cfg, syn, max_slots=4, max_positions=128)
    base = _serve(llm, reqs, range(len(reqs)), 4, RECORDS)
    alone = _serve(llm, reqs, range(len(reqs)), 1, RECORDS)
    perm = [5, 2, 7, 0, 6, 3, 1, 4]
    shuffled = _serve(llm, reqs, perm, 4, RECORDS)
    fresh = _serve(_llm(cfg, syn, max_slots=8, max_positions=128), reqs, perm, 8, RECORDS)
    for i in range(len(reqs)):
        assert alone[i] == base[i] and shuffled[i] == base[i] and fresh[i] == base[i], f"request {i}"
    unpen = [r if i in PLAIN else None for i, r in enumerate(RECORDS)]
    plain = _serve(llm, reqs, [i for i in range(len(reqs)) if i in PLAIN], 4, unpen)
    for i in PLAIN:
        assert plain[i] == base[i], f"plain request {i} changed by its penalised neighbours"
    no_pen = _serve(llm, reqs, [0, 5], 4, [{"do_sample": False}] * len(RECORDS))
    assert any(no_pen[i] != base[i] for i in (0, 5)), "the penalties must change the penalised rows"


# 4 -------------------------------------------------------------------------------------------------------------------
def test_admitting_a_penalised_request_into_a_live_session(tiny):
    cfg, syn = tiny
    ps = _prompts(cfg, 95, 5)
    pen = {"repetition_penalty": 1.4, "frequency_penalty": 0.5}
    llm = _llm(cfg, syn, max_slots=4, max_positions=256)
    solo = lambda p, rec=None: llm.generate_ragged([p], [40], sampling=[rec])[0]   # noqa: E731
    want = [solo(ps[0]), solo(ps[1]), solo(ps[2], pen), solo(ps[3]), solo(ps[4], pen)]
    assert want[2] != solo(ps[2])
    llm.session_begin()
    s01 = llm.admit(ps[:2])
    llm.decode(6)                                  # unpenalised graph
    s2 = llm.admit([ps[2]], [pen])[0]              # the penalty bit: another graph, the live rows unchanged
    llm.decode(40)
    toks = [t for t, _ in llm.slots_tokens(s01 + [s2], 64)]
    assert toks[0][:40] == want[0] and toks[1][:40] == want[1] and toks[2][:40] == want[2]
    llm.retire(s2)                                 # its slot again: an unpenalised sequence, then a penalised one
    s3 = llm.admit([ps[3]])[0]
    assert s3 == s2
    llm.decode(40)
    assert llm.slots_tokens([s3], 64)[0][0][:40] == want[3]
    llm.retire(s3)
    s4 = llm.admit([ps[4]], [pen])[0]
    assert s4 == s2
    llm.decode(40)
    assert llm.slots_tokens([s4], 64)[0][0][:40] == want[4], "stale history in a reused slot"


# 5 -------------------------------------------------------------------------------------------------------------------
def test_sampling_after_penalties(golden_dir):
    cfg = C.tiny_llm()
    llm = _llm(cfg, W.SyntheticLLM(cfg), max_slots=64, max_positions=32, diag=True)
    case = {c[0]: c for c in fixture_cases(golden_dir)}["argmax_moves"]
    _, x, y, hist, rec, emitted, eos = case
    llm.session_begin(eos)
    row = llm.debug_penalize(x[None], hist[None], [rec], [emitted])[0][0]
    assert np.array_equal(row.view(np.uint32), y.view(np.uint32))
    T, k, p = 1.0, 50, 0.95
    want = sampling_probs(torch.from_numpy(row), T, k, p).numpy().astype(np.float64)
    llm.set_sampling(True, T, k, p, 0)
    counts = np.zeros(len(row))
    for seed in range(320):   # 20 480 draws
        np.add.at(counts, llm.debug_sample(row if seed == 0 else None, 64, 5000 + seed), 1)
    assert (counts[want == 0] == 0).all()
    tv = 0.5 * np.abs(counts / counts.sum() - want).sum()
    assert tv < 0.03, f"total variation distance {tv:.4f}"


# 6 -------------------------------------------------------------------------------------------------------------------
BAD = [dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
       dict(repetition_penalty=float("inf")), dict(presence_penalty=2.5), dict(presence_penalty=float("nan")),
       dict(frequency_penalty=-2.01), dict(frequency_penalty=float("inf")), dict(min_new_tokens=-1), dict(min_new_tokens=97),
       dict(penalize_prompt=2), dict(reserved=1)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_a_bad_record_fails_the_admission_and_changes_nothing(tiny, bad):
    from sparkmi import _lib
    cfg, syn = tiny
    ps = _prompts(cfg, 44, 6, 5, 40)
    llm = _llm(cfg, syn, max_slots=8, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)   # unseeded rows: their streams are keyed by admission numbers

    def admit_raw(prompts, k_bad):
        n, pmax = len(prompts), max(len(p) for p in prompts)
        ids = np.zeros((n, pmax), dtype=np.int64)
        for b, p in enumerate(prompts):
            ids[b, : len(p)] = p
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        pens = (_lib.PenaltyParams * n)()
        for b in range(n):
            pens[b].repetition_penalty, pens[b].penalize_prompt = 1.2, 1
        r = pens[k_bad]
        for key, v in bad.items():
            if key == "reserved":
                r.reserved[1] = v
            else:
                setattr(r, key, v)
        slots = np.zeros(n, dtype=np.int32)
        return llm._lib.smi_llm_admit_penalized(llm._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, pmax, None, pens,
                                                slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), llm._stream())

    def run(fail):
        llm.session_begin()
        first = llm.admit(ps[:2])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            assert admit_raw(ps[2:], 1) == -1   # SMI_EINVAL
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        slots = first + llm.admit(ps[2:])          # takes the slots and admission numbers the failed call did not
        llm.decode(10)
        return [t for t, _ in llm.slots_tokens(slots, 16)]

    assert run(True) == run(False)


# 7 -------------------------------------------------------------------------------------------------------------------
def test_penalised_rows_past_k_lm32_at_full_size(full_llm):
    """0.5B shape, bf16 KV, captured steps: a session that grows to 40+ live rows through small admissions, every other
    sequence penalised (greedy and seeded sampling), so steps of more than 16 rows take k_lm32 and k_penalize's 256-set
    partition; every sequence equals its solo run."""
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, _, arena = full_llm
    prompts = _prompts(cfg, 3400, 44, 3, 60)
    recs = []
    for b in range(44):
        if b % 4 == 0:
            # (random weights seldom repeat a token within 20 steps; r < 1 multiplies the prompt ids' positive logits, so the
            # arg-max certainly moves)
            recs.append({"do_sample": False, "repetition_penalty": 0.2, "presence_penalty": 0.3})
        elif b % 4 == 2:
            recs.append({"do_sample": True, "temperature": 0.9, "top_k": 50, "top_p": 0.95, "seed": 100 + b,
                         "frequency_penalty": 0.5, "penalize_prompt": False})
        else:
            recs.append(None)
    n = 20
    llm = SparkLLM(cfg, None, "cuda:0", max_slots=48, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    llm.session_begin()
    slots = []
    for g0 in range(0, 44, 6):
        slots += llm.admit(prompts[g0:g0 + 6], recs[g0:g0 + 6])
        llm.decode(2)
    llm.decode(n)
    got = [t[:n] for t, _ in llm.slots_tokens(slots, 64)]
    one = SparkLLM(cfg, None, "cuda:0", max_slots=1, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    differ = [b for b in range(44) if got[b] != one.generate_ragged([prompts[b]], [n], sampling=[recs[b]])[0]]
    assert differ == [], f"sequences that differ from their solo run: {differ}"
    plain = [one.generate_ragged([prompts[b]], [n])[0] for b in (0, 4, 8)]
    assert any(got[b] != w for b, w in zip((0, 4, 8), plain)), "the penalties must change the penalised rows"


# 8 -------------------------------------------------------------------------------------------------------------------
def test_pipeline_requests_with_penalty_keys(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_pen")
    lcfg, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(12))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    req = dict(text="utterance number one " * 2, prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    kw = dict(do_sample=False, max_new_tokens=40)
    # neutral keys: the same route and bits as the request without them
    plain = tts.inference_batch([req], **kw)[0]
    neutral = tts.inference_batch([dict(req, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0,
                                        min_new_tokens=0, penalize_prompt=False)], **kw)[0]
    assert np.array_equal(neutral, plain)
    assert np.array_equal(tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], repetition_penalty=1.0, **kw), plain)
    # a penalised request: the tokens generate_ragged gives for the same record (captured at the LLM boundary)
    calls = []
    inner = tts.model.generate_ragged

    def spy(ids, budgets, eos=None, **k):
        out = inner(ids, budgets, eos, **k)
        calls.append((ids, budgets, eos, k.get("sampling"), out))
        return out

    tts.model.generate_ragged = spy
    # (the random-weight model repeats no token in 40, so only r < 1 on the prompt ids moves its arg-max; 0.7 does so at token 8
    # and still leaves semantic tokens to vocode)
    pen = dict(repetition_penalty=0.7, penalize_prompt=True)
    wav = tts.inference_batch([dict(req, **pen)], **kw)[0]
    assert calls, "a penalised request must take the admission path"
    ids, budgets, eos, sampling, out = calls[-1]
    assert sampling == [pen]
    assert out == inner(ids, budgets, eos, sampling=[pen])
    oracle = Qwen2Ref(lcfg, W.load_llm_state(d / "LLM"), kv_dtype="bf16")
    assert out[0] == greedy_generate(oracle, ids[0], budgets[0], pen, eos)
    assert out[0] != greedy_generate(oracle, ids[0], budgets[0], {}, eos)
    wav2 = tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], **pen, **kw)
    assert np.array_equal(wav, wav2)
