"""Per-request sampling records (smi_llm_admit_sampled; TensorRT-LLM's per-request temperature / runtime_top_k / runtime_top_p /
random_seed inputs): greedy, inheriting and sampling rows of any mix share one decode step, a seeded row's tokens depend on its
seed alone, a bad record changes nothing."""
import os

import numpy as np
import pytest
import torch

from oracle.llm_ref import Qwen2Ref
from sparkmi import config as C, weights as W

pytestmark = pytest.mark.gpu


def _llm(cfg, syn, **kw):
    from sparkmi.llm import SparkLLM
    kw.setdefault("diag", any(k.startswith("SPARKMI_") for k in os.environ))   # A/B switches live in the diagnostics build
    return SparkLLM(cfg, syn, device="cuda:0", **kw)


@pytest.fixture(scope="module")
def tiny():
    cfg = C.tiny_llm()
    return cfg, W.SyntheticLLM(cfg)


def _check_draws(counts, want, what):
    n = counts.sum()
    assert (counts[want == 0] == 0).all(), f"{what}: sampled a token outside the top-k / nucleus set"
    tv = 0.5 * np.abs(counts / n - want).sum()
    assert tv < 0.03, f"{what}: total variation distance {tv:.4f} over {int(n)} draws"
    return tv


HANDLE = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=77)
RECORDS = [
    {"do_sample": False},                                                                     # greedy under a sampling handle
    None,                                                                                     # inherit
    {"do_sample": True, "temperature": 0.7, "top_k": 20, "top_p": 0.9, "seed": 1001},
    None,
    {"do_sample": True, "temperature": 1.2, "top_k": 256, "top_p": 1.0, "seed": 1002},
    {"do_sample": False},
    {"do_sample": True, "temperature": 0.9, "top_k": 5, "top_p": 0.8, "seed": 1003},
    {"do_sample": True, "temperature": 1.0, "top_k": 60, "top_p": 0.95},                      # own T / k / p, the handle's stream
]
GREEDY, INHERIT, SEEDED = (0, 5), (1, 3), (2, 4, 6)


def _serve(llm, reqs, order, max_live, recs):
    llm.set_sampling(**HANDLE)
    return dict(llm.serve(iter([reqs[i][:4] + (recs[i],) for i in order]), max_live=max_live, decode_stride=3))


def test_mixed_records_in_one_session(tiny):
    cfg, syn = tiny
    rng = np.random.Generator(np.random.PCG64(91))
    reqs = [(i, rng.integers(0, cfg.vocab_size, size=int(rng.integers(3, 30))).tolist(), int(rng.integers(8, 30)), None)
            for i in range(len(RECORDS))]
    llm = _llm(cfg, syn, max_slots=4, max_positions=96)
    base = _serve(llm, reqs, range(8), 4, RECORDS)
    for i, _, n, _ in reqs:
        assert len(base[i]) == n and all(0 <= t < cfg.vocab_size for t in base[i]), f"request {i}"
    # greedy rows: the CPU oracle's arg-max and the handle-level greedy run, although the handle samples
    oracle = Qwen2Ref(cfg, syn, kv_dtype="bf16")
    for i in GREEDY:
        _, p, n, _ = reqs[i]
        assert base[i] == oracle.generate_greedy(np.asarray(p), n), f"greedy request {i} vs oracle"
    llm.set_sampling(False)
    for i in GREEDY:
        _, p, n, _ = reqs[i]
        assert base[i] == llm.generate_ids([p], n)[0], f"greedy request {i} vs handle-level greedy"
    # seeded rows: alone, in another order and slot, on another handle -- the same tokens
    alone = _serve(llm, reqs, range(8), 1, RECORDS)
    perm = [5, 2, 7, 0, 6, 3, 1, 4]
    shuffled = _serve(llm, reqs, perm, 4, RECORDS)
    fresh = _serve(_llm(cfg, syn, max_slots=8, max_positions=96), reqs, perm, 8, RECORDS)
    for i in SEEDED + GREEDY:
        assert alone[i] == base[i] and shuffled[i] == base[i] and fresh[i] == base[i], f"request {i}"
    # the same order: every sequence has the same admission number, so the unseeded rows repeat too
    for i in INHERIT + (7,):
        assert alone[i] == base[i], f"request {i} (same admission order)"
    # inherit rows: exactly the run in which every request inherits
    every = _serve(llm, reqs, range(8), 4, [None] * 8)
    for i in INHERIT:
        assert base[i] == every[i], f"inheriting request {i}"
    # another seed moves that row and only that row
    recs = [dict(r) if r else r for r in RECORDS]
    recs[2]["seed"] = 2001
    moved = _serve(llm, reqs, range(8), 4, recs)
    assert moved[2] != base[2]
    for i in range(8):
        if i != 2:
            assert moved[i] == base[i], f"request {i} moved with another row's seed"


def test_per_row_distributions_in_one_step(tiny):
    """64 rows of one prompt in ONE admission, three configurations side by side: top_k 12 (at most the lm_head's 16 blocks:
    the block-maxima bound path), top_k 256 and top_k 40 (above it: exact radix selection) -- each configuration's first-token
    draws against oracle/sampling_ref.py.  The top_k-256 configuration gets half the rows: over its 112 nucleus tokens the
    sampling noise alone leaves a total variation near 0.017 at 41 600 draws (0.039 at 21 000 draws over 256 flat tokens)."""
    from oracle.sampling_ref import sampling_probs
    cfg, syn = tiny
    prompt = [5, 17, 200, 33, 9, 410, 77]
    confs = [(0.8, 12, 0.95), (0.7, 256, 0.9), (1.3, 40, 0.8)]
    logits = Qwen2Ref(cfg, syn, kv_dtype="bf16").forward(prompt, last_only=True)[0]
    llm = _llm(cfg, syn, max_slots=64, max_positions=64)
    llm.set_sampling(False)
    counts = np.zeros((len(confs), cfg.vocab_size))
    rows = [(0, 1, 2, 1)[r % 4] for r in range(64)]
    for a in range(1300):   # 16 / 32 / 16 rows per admission: 20 800 / 41 600 / 20 800 draws
        recs = [dict(do_sample=True, temperature=confs[c][0], top_k=confs[c][1], top_p=confs[c][2], seed=a * 64 + r)
                for r, c in enumerate(rows)]
        got = llm.generate_ragged([prompt] * 64, [1] * 64, sampling=recs)
        for r, t in enumerate(got):
            counts[rows[r], t[0]] += 1
    for c, (T, K, P) in enumerate(confs):
        _check_draws(counts[c], sampling_probs(logits, T, K, P).numpy(), f"T {T} / k {K} / p {P}")
        assert (counts[c] > 0).sum() > 5


def test_greedy_rows_under_a_sampling_handle_are_exact_at_full_size(full_llm):
    """0.5B shape, bf16 KV cache, 32 rows in one admission, every other row greedy and the rest sampling (the handle's
    settings): each greedy row equals its own greedy run alone, bit for bit."""
    from conftest import FULL_MAX_POS
    from sparkmi.llm import SparkLLM
    cfg, _, arena = full_llm
    rng = np.random.Generator(np.random.PCG64(3300))
    prompts = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(3, 200))).tolist() for _ in range(32)]
    n = 24
    llm = SparkLLM(cfg, None, "cuda:0", max_slots=32, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    llm.set_sampling(True, 0.8, 50, 0.95, seed=3)
    got = llm.generate_ragged(prompts, [n] * 32, sampling=[{"do_sample": False} if b % 2 == 0 else None for b in range(32)])
    one = SparkLLM(cfg, None, "cuda:0", max_slots=1, max_positions=FULL_MAX_POS, arena=arena, kv_dtype="bf16")
    for b in range(0, 32, 2):
        assert got[b] == one.generate_ids([prompts[b]], n)[0], f"greedy row {b}"
    assert any(got[b] != one.generate_ids([prompts[b]], n)[0] for b in range(1, 32, 2))


@pytest.mark.parametrize("bad", [dict(top_k=0), dict(top_k=300), dict(temperature=0.0), dict(temperature=-1.0),
                                 dict(top_p=1.5), dict(top_p=0.0)])
def test_a_bad_record_fails_the_admission_and_changes_nothing(tiny, bad):
    from sparkmi._lib import SparkMIError
    cfg, syn = tiny
    rng = np.random.Generator(np.random.PCG64(44))
    ps = [rng.integers(0, cfg.vocab_size, size=int(rng.integers(5, 40))).tolist() for _ in range(6)]
    llm = _llm(cfg, syn, max_slots=8, max_positions=96, kv_page_tokens=16, kv_pages=40)
    llm.set_sampling(True, 0.9, 40, 0.95, seed=5)

    def run(fail):
        llm.session_begin()
        first = llm.admit(ps[:2])
        pages, (cnt, fin) = llm.kv_pages(), llm.status()
        if fail:
            rec = dict(do_sample=True, temperature=0.8, top_k=50, top_p=0.9, seed=9)
            rec.update(bad)
            with pytest.raises(SparkMIError):
                llm.admit(ps[2:], [None, rec, None, None])
            assert llm.kv_pages() == pages
            cnt2, fin2 = llm.status()
            assert np.array_equal(cnt, cnt2) and np.array_equal(fin, fin2)
        slots = first + llm.admit(ps[2:])          # takes the slots and admission numbers the failed call did not
        llm.decode(10)
        return [t for t, _ in llm.slots_tokens(slots, 16)]

    assert run(True) == run(False)


def test_front_end_per_request_keys(tmp_path_factory):
    """SparkTTS.inference_batch / serve with per-request keys: the greedy request equals inference(do_sample=False), the
    seeded one equals itself alone, serve gives the same waveforms."""
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_rows")
    _, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(12))
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"utterance number {i} " * (i + 1), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long))))
    reqs[0]["do_sample"] = False
    reqs[1].update(temperature=0.7, top_k=30, seed=123)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    kw = dict(temperature=0.8, top_k=50, top_p=0.95, max_new_tokens=40, seed=4)
    batch = tts.inference_batch(reqs, **kw)
    greedy = tts.inference(reqs[0]["text"], prompt_tokens=reqs[0]["prompt_tokens"], do_sample=False, max_new_tokens=40)
    assert np.array_equal(batch[0], greedy)
    solo = tts.inference_batch([reqs[1]], **kw)[0]
    assert np.array_equal(batch[1], solo)
    served = dict(tts.serve(iter(reqs), **kw))
    for i in range(3):
        assert np.array_equal(served[i], batch[i]), f"request {i}"
