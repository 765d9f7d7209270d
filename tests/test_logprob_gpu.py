"""Per-token log-probabilities (smi_llm_admit_logprobs; TensorRT-LLM's return_log_probs -> output_log_probs): k_logprob +
k_finalize's combine against transformers' processors, greedy / sampled / penalised sessions against teacher-forced logits
and the CPU oracle, flagged rows next to unflagged ones without changing any bits, a bad flag changes nothing."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from logprob_ref import fixture_rows, log_softmax64, replay
from oracle.llm_ref import Qwen2Ref
from sparkmi import config as C, weights as W

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
def test_kernel_matches_transformers(golden_dir, vocab):
    cfg = C.tiny_llm()
    if cfg.vocab_size != vocab:
        cfg = dataclasses.replace(cfg, vocab_size=vocab)
    llm = _llm(cfg, W.SyntheticLLM(cfg), max_slots=4, max_positions=64, diag=True)
    cases = [c for c in fixture_rows(golden_dir) if len(c[1]) == vocab]
    assert len(cases) >= 3
    for name, z, T, ids, lp in cases:   # one row
        got = llm.debug_logprob(z[None], [T if T > 0 else 1.0], [int(ids[0])])
        assert abs(float(got[0]) - float(lp[0])) <= 2e-5, f"{name}: {got[0]} vs {lp[0]}"
    for k in range(len(cases)):         # three rows, each with its own row, temperature and token
        trio = [cases[(k + j) % len(cases)] for j in range(3)]
        got = llm.debug_logprob(np.stack([c[1] for c in trio]), [c[2] if c[2] > 0 else 1.0 for c in trio],
                                [int(c[3][0]) for c in trio])
        for j, c in enumerate(trio):
            assert abs(float(got[j]) - float(c[4][0])) <= 2e-5, f"{c[0]} (row {j} of 3): {got[j]} vs {c[4][0]}"


# 2 -------------------------------------------------------------------------------------------------------------------
def test_greedy_logprobs_match_teacher_forcing_and_the_oracle(tiny):
    cfg, syn = tiny
    prompt = _prompts(cfg, 7, 1, 12, 13)[0]
    N = 48
    llm = _llm(cfg, syn, max_slots=2, max_positions=128, kv_dtype="f32")
    plain = llm.generate_ragged([prompt], [N])[0]
    toks, lps = llm.generate_ragged([prompt], [N], return_log_probs=True)[0]
    assert toks == plain, "the flag must not change the tokens"
    assert lps.dtype == np.float32 and lps.shape == (N,)
    assert np.isfinite(lps).all() and (lps <= 0).all()
    rows = llm.forward_logits(prompt + toks[:-1]).cpu()     # (after the session: it resets slot 0)
    want = replay(rows, prompt, toks)
    assert np.abs(lps - want).max() <= 1e-4, np.abs(lps - want).max()
    oracle = Qwen2Ref(cfg, syn, kv_dtype="f32")
    orows = oracle.forward(prompt + toks[:-1]).to(torch.float32)
    owant = replay(orows, prompt, toks)
    assert np.abs(lps - owant).max() <= 2e-3, np.abs(lps - owant).max()
    # a greedy, unpenalised row: the model's own log_softmax at its arg-max
    assert all(int(np.argmax(log_softmax64(rows[len(prompt) - 1 + t].numpy()))) == toks[t] for t in range(N))


# 3 -------------------------------------------------------------------------------------------------------------------
SCORED = [
    {"do_sample": True, "temperature": 0.3, "top_k": 50, "top_p": 0.95, "seed": 21},
    {"do_sample": True, "temperature": 1.7, "top_k": 256, "top_p": 1.0, "seed": 22},
    {"do_sample": False, "repetition_penalty": 1.4, "frequency_penalty": 0.3},
    {"do_sample": False, "min_new_tokens": 12, "penalize_prompt": False, "repetition_penalty": 0.8},
    {"do_sample": True, "temperature": 0.8, "top_k": 40, "top_p": 0.9, "seed": 23, "presence_penalty": 0.5,
     "penalize_prompt": False, "repetition_penalty": 1.2},
]


def test_sampled_and_penalised_rows_match_the_cpu_replay(tiny):
    cfg, syn = tiny
    ps = _prompts(cfg, 8, len(SCORED), 6, 20)
    N = 32
    llm = _llm(cfg, syn, max_slots=2, max_positions=128, kv_dtype="f32")
    # eos: a token the plain greedy run of prompt 3 emits early, so min_new_tokens' mask matters
    eos = [llm.generate_ragged([ps[3]], [N])[0][1]]
    for p, rec in zip(ps, SCORED):
        plain = llm.generate_ragged([p], [N], eos, sampling=[rec])[0]
        toks, lps = llm.generate_ragged([p], [N], eos, sampling=[dict(rec, return_log_probs=True)])[0]
        assert toks == plain, rec
        assert len(lps) == len(toks) and np.isfinite(lps).all(), rec
        rows = llm.forward_logits(p + toks[:-1]).cpu()
        T = rec["temperature"] if rec.get("do_sample") else 0.0
        want = replay(rows, p, toks, rec, eos, T)
        assert np.abs(lps - want).max() <= 2e-4, (rec, np.abs(lps - want).max())
    # the handle's sampler settings for an inheriting row
    llm.set_sampling(True, 0.6, 30, 0.9, seed=9)
    toks, lps = llm.generate_ragged([ps[0]], [N], return_log_probs=True)[0]
    want = replay(llm.forward_logits(ps[0] + toks[:-1]).cpu(), ps[0], toks, None, (), 0.6)
    assert np.abs(lps - want).max() <= 2e-4


# 4 -------------------------------------------------------------------------------------------------------------------
RECORDS = [
    {"do_sample": False, "return_log_probs": True},
    {"do_sample": True, "temperature": 0.8, "top_k": 40, "top_p": 0.95, "seed": 11, "return_log_probs": True},
    {"do_sample": False},
    None,
    {"do_sample": False, "repetition_penalty": 1.3, "min_new_tokens": 6, "return_log_probs": True},
    {"return_log_probs": False, "seed": 12},
    {"do_sample": True, "temperature": 1.3, "top_k": 256, "top_p": 1.0, "seed": 13, "frequency_penalty": 0.4,
     "penalize_prompt": False, "return_log_probs": True},
    {"return_log_probs": True},
]


def _serve(llm, reqs, order, max_live, recs):
    llm.set_sampling(False)
    return dict(llm.serve(iter([reqs[i][:4] + (recs[i],) for i in order]), max_live=max_live, decode_stride=3))


def test_flagged_rows_are_independent_in_one_session(tiny):
    cfg, syn = tiny
    rng = np.random.Generator(np.random.PCG64(193))
    eos = [int(rng.integers(0, cfg.vocab_size))]
    reqs = [(i, p, int(rng.integers(12, 40)), eos) for i, p in enumerate(_prompts(cfg, 194, len(RECORDS)))]
    llm = _llm(cfg, syn, max_slots=4, max_positions=128, kv_dtype="f32")
    mixed = _serve(llm, reqs, range(len(reqs)), 4, RECORDS)     # mid-session admissions into reused slots
    perm = [6, 3, 0, 5, 7, 2, 4, 1]
    shuffled = _serve(llm, reqs, perm, 3, RECORDS)
    unflagged = [{k: v for k, v in r.items() if k != "return_log_probs"} if r else r for r in RECORDS]
    for i, rec in enumerate(RECORDS):
        alone = _serve(llm, reqs, [i], 1, RECORDS)[i]
        flagged = bool(rec and rec.get("return_log_probs"))
        for got in (mixed[i], shuffled[i]):
            if flagged:
                assert got[0] == alone[0], f"request {i}: tokens"
                assert np.array_equal(got[1].view(np.uint32), alone[1].view(np.uint32)), f"request {i}: log-probs"
            else:
                assert got == alone, f"request {i}"
        plain = _serve(llm, reqs, [i], 1, unflagged)[i]
        assert (mixed[i][0] if flagged else mixed[i]) == plain, f"request {i}: the flag changed the tokens"


def test_slot_reuse_and_reading_a_slot_without_the_flag(tiny):
    from sparkmi import _lib
    cfg, syn = tiny
    ps = _prompts(cfg, 95, 3)
    llm = _llm(cfg, syn, max_slots=2, max_positions=128)
    llm.session_begin()
    a, b = llm.admit(ps[:2], [{"return_log_probs": True}, None])
    llm.decode(10)
    la = llm.slots_logprobs([a], 64)[0]
    assert len(la) == 11 and np.isfinite(la).all()
    with pytest.raises(_lib.SparkMIError):
        llm.slots_logprobs([b], 64)
    out, n = (ctypes.c_float * 8)(), (ctypes.c_int32 * 1)()
    sl = (ctypes.c_int32 * 1)(b)
    assert llm._lib.smi_llm_slots_logprobs(llm._h, sl, 1, out, 8, n, llm._stream()) == -4   # SMI_ESTATE
    llm.retire(a)                                  # still readable until reused
    assert np.array_equal(llm.slots_logprobs([a], 64)[0], la)
    c = llm.admit([ps[2]])[0]                      # the slot again, unflagged: no longer readable
    assert c == a
    with pytest.raises(_lib.SparkMIError):
        llm.slots_logprobs([c], 64)


# 5 -------------------------------------------------------------------------------------------------------------------
BAD = [2, -1, 7]


@pytest.mark.parametrize("bad", BAD)
def test_a_bad_flag_fails_the_admission_and_changes_nothing(tiny, bad):
    cfg, syn = tiny
    ps = _prompts(cfg, 44, 6, 5, 40)
    llm = _llm(cfg, syn, max_slots=8, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)   # unseeded rows: their streams are keyed by admission numbers

    def admit_raw(prompts):
        n, pmax = len(prompts), max(len(p) for p in prompts)
        ids = np.zeros((n, pmax), dtype=np.int64)
        for k, p in enumerate(prompts):
            ids[k, : len(p)] = p
        lens = np.asarray([len(p) for p in prompts], dtype=np.int32)
        flags = np.ones(n, dtype=np.int32)
        flags[1] = bad
        slots = np.zeros(n, dtype=np.int32)
        return llm._lib.smi_llm_admit_logprobs(llm._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                               lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, pmax, None, None,
                                               flags.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               slots.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), llm._stream())

    def run(fail):
        llm.session_begin()
        first = llm.admit(ps[:2])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            assert admit_raw(ps[2:]) == -1   # SMI_EINVAL
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        slots = first + llm.admit(ps[2:])    # takes the slots and admission numbers the failed call did not
        llm.decode(10)
        return [t for t, _ in llm.slots_tokens(slots, 16)]

    assert run(True) == run(False)


# 6 -------------------------------------------------------------------------------------------------------------------
def test_flagged_rows_past_k_lm32_at_full_size(full_llm, full_llm_oracle):
    """0.5B shape, bf16 KV, captured steps: a session that grows to 44 live rows through small admissions, every other
    sequence flagged (greedy, seeded sampling, penalised), so steps of more than 16 rows take k_lm32; every sequence equals
    its solo run bit for bit, log-probabilities included, and the first greedy rows match the fp32 oracle."""
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, syn, arena = full_llm
    prompts = _prompts(cfg, 4400, 44, 3, 60)
    recs = []
    for b in range(44):
        if b % 4 == 0:
            recs.append({"do_sample": False, "return_log_probs": True})
        elif b % 4 == 1:
            recs.append({"do_sample": True, "temperature": 0.9, "top_k": 50, "top_p": 0.95, "seed": 100 + b,
                         "return_log_probs": True})
        elif b % 4 == 2:
            recs.append({"do_sample": False, "repetition_penalty": 1.2, "return_log_probs": True} if b % 8 == 2 else None)
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
    flagged = [b for b in range(44) if recs[b] and recs[b].get("return_log_probs")]
    lps = dict(zip(flagged, (x[:n] for x in llm.slots_logprobs([slots[b] for b in flagged], 64))))
    one = SparkLLM(cfg, None, "cuda:0", max_slots=1, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    differ = []
    for b in range(44):
        solo = one.generate_ragged([prompts[b]], [n], sampling=[recs[b]])[0]
        if b in lps:
            ok = solo[0] == got[b] and np.array_equal(solo[1].view(np.uint32), lps[b].view(np.uint32))
        else:
            ok = solo == got[b]
        if not ok:
            differ.append(b)
    assert differ == [], f"sequences that differ from their solo run: {differ}"
    oracle = full_llm_oracle
    oracle.kv_dtype = "bf16"
    for b in (0, 4):
        oracle.reset()
        rows = oracle.forward(prompts[b] + got[b][:-1]).to(torch.float32)
        want = replay(rows, prompts[b], got[b])
        assert np.abs(lps[b] - want).max() <= 5e-3, (b, np.abs(lps[b] - want).max())


# 7 -------------------------------------------------------------------------------------------------------------------
def test_pipeline_returns_logprobs_with_the_same_waveform(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_lp")
    _, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(12))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    pt = (glob, torch.zeros((1, 0), dtype=torch.long))
    kw = dict(do_sample=False, max_new_tokens=40)
    text = "utterance number one " * 2
    plain = tts.inference(text, prompt_tokens=pt, **kw)
    assert isinstance(plain, np.ndarray)
    wav, info = tts.inference(text, prompt_tokens=pt, return_log_probs=True, **kw)
    assert np.array_equal(wav, plain)
    ids, lp = info["token_ids"], info["output_log_probs"]
    assert len(ids) >= 1 and lp.dtype == np.float32 and lp.shape == (len(ids),) and np.isfinite(lp).all()
    assert info["cum_log_prob"] == float(np.sum(lp, dtype=np.float64))
    # the batch and the per-request key give the same
    out = tts.inference_batch([dict(text=text, prompt_tokens=pt, return_log_probs=True), dict(text=text, prompt_tokens=pt)], **kw)
    assert isinstance(out[0], tuple) and isinstance(out[1], np.ndarray)
    assert np.array_equal(out[0][0], plain) and out[0][1]["token_ids"] == ids
    assert np.array_equal(out[0][1]["output_log_probs"], lp)
