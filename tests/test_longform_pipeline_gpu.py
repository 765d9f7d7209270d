"""SparkTTS.inference_long / inference_long_stream on the synthetic model directory of tests/test_audio_prep_pipeline_gpu.py
(max_batch=2, max_positions=1024, max_frames=256; prompt_tokens given; the ids kept on semantic tokens and eos).

Yardstick: the sentences as requests of ``serve`` -- their tokens, and their waveforms trimmed and joined by tests/trim_ref.py,
bit for bit.  The synthetic vocoder's level is arbitrary, so every test takes its ``trim_threshold`` from the untrimmed rows, on
the CPU, such that no window's energy lies within 1e-4 relative of the threshold (asserted): the fp32 / fp64 evaluations of a
window differ by far less, so the bounds are decided."""
import numpy as np
import pytest
import torch

import trim_ref as tr

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence of the paragraph is this one. Then a second one follows it, a little longer than the first! "
        "Is the third one a question? The fourth sentence; short. And the fifth sentence closes the paragraph.")
W, S, M = 1600, 160, 3200
PAUSE, FADE = 0.25, 0.005
GAP, FADE_N = 4000, 80
BUDGET = 40


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import longform, synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_long")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    voice = dict(prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                 allowed_token_ids=sorted(tts._map.sem) + list(tts._eos), min_new_tokens=14)   # a sentence may end on its own from 14 ids on
    sentences = longform.split_text(TEXT, 300, 20)
    assert len(sentences) == 5
    # the yardstick, once: the sentences as requests of serve (more requests than rows: admission mid-session)
    rows, toks = {}, {}
    for k, w, info in tts.serve([dict(voice, text=s) for s in sentences], do_sample=False, max_new_tokens=BUDGET, return_log_probs=True):
        rows[k], toks[k] = w, list(info["token_ids"])
    rows = [rows[k] for k in range(5)]
    assert all(r.size >= 14 * 320 - 320 for r in rows)
    return tts, voice, sentences, rows, [toks[k] for k in range(5)]


def _threshold(rows, q):
    """an rms threshold near the ``q`` quantile of all window energies, in the widest gap between two neighbours there; asserts
    the condition that makes exact bounds meaningful"""
    e = np.sort(np.concatenate([tr.energies(r, W, S) for r in rows]))
    lo, hi = int(max(0, (q - 0.05) * e.size)), int(min(e.size - 1, (q + 0.05) * e.size))
    j = lo + int(np.argmax(e[lo + 1: hi + 1] / e[lo: hi]))
    thr = float(np.sqrt(np.sqrt(e[j] * e[j + 1]) / W))
    for r in rows:
        assert tr.closest_to_level(r, W, S, thr) > 1e-4, "a window sits on the threshold: pick another quantile"
    return thr


def _expected(rows, thr, trim=True):
    bounds = [tr.bounds(r, W, S, thr, M) if trim else (0, r.size) for r in rows]
    gaps, spoken = [], False
    for a, b in bounds:
        gaps.append(GAP if b > a and spoken else 0)
        spoken = spoken or b > a
    want, offs, total = tr.concat(rows, bounds, gaps, FADE_N)
    return want, bounds, offs


def test_five_sentences_greedy_equal_serve_trimmed_and_joined(setup):
    tts, voice, sentences, rows, toks = setup
    thr = _threshold(rows, 0.8)
    kw = dict(voice, do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=FADE)
    wav, info = tts.inference_long(TEXT, trim_threshold=thr, return_info=True, **kw)
    want, bounds, offs = _expected(rows, thr)
    print("bounds", bounds, "of", [r.size for r in rows], "thr", thr)
    assert info["sentences"] == sentences and info["token_ids"] == toks
    assert info["bounds"] == bounds and info["offsets"] == offs
    assert info["silent"] == [k for k, (a, b) in enumerate(bounds) if a == b]
    assert info["truncated"] == [k for k, t in enumerate(toks) if len(t) == BUDGET and t[-1] not in tts._eos]
    assert wav.dtype == np.float32 and wav.size == want.size and np.array_equal(wav.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(tts.inference_long(TEXT, trim_threshold=thr, **kw), wav)      # without info: the waveform alone
    plain, _, _ = _expected(rows, thr, trim=False)
    got = tts.inference_long(TEXT, trim=False, **kw)
    assert got.size == sum(r.size for r in rows) + 4 * GAP and np.array_equal(got, plain)


def test_sampled_sentences_carry_seed_plus_k(setup):
    tts, voice, sentences, rows, toks = setup
    kw = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.9, max_new_tokens=BUDGET)
    _, info = tts.inference_long(TEXT, seed=71, trim=False, return_info=True, **dict(voice, **kw))
    for k, s in enumerate(sentences):
        _, one = tts.inference_batch([dict(voice, text=s, seed=71 + k)], return_log_probs=True, **kw)[0]
        assert info["token_ids"][k] == tts._cut_eos(list(one["token_ids"])), k
    assert info["token_ids"] != toks


@pytest.mark.parametrize("sr", [None, 24000])
def test_stream_pieces_concatenate_to_inference_long(setup, sr):
    from sparkmi import audio
    tts, voice, sentences, rows, toks = setup
    thr = _threshold(rows, 0.8)
    kw = dict(voice, do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=FADE, trim_threshold=thr, output_sample_rate=sr)
    whole = tts.inference_long(TEXT, **kw)
    pieces = list(tts.inference_long_stream(TEXT, **kw))
    assert len(pieces) >= 2 and all(p.dtype == np.float32 and p.ndim == 1 and p.size for p in pieces)
    assert np.array_equal(np.concatenate(pieces), whole)
    base, bounds, offs = _expected(rows, thr)
    if sr is None:   # a piece is a sentence's gap + trimmed + faded piece
        assert [p.size for p in pieces] == [b - a + (GAP if k else 0) for k, (a, b) in enumerate(bounds) if b > a]
    else:            # ... and at another rate the whole is resample_rows of the model-rate waveform
        up, down = audio.ratio(16000, sr)
        y, n_out = tts._device_audio().resample_rows(torch.from_numpy(base[None]).cuda(), [base.size], [up], [down])
        assert np.array_equal(whole, y.cpu().numpy()[0, : n_out[0]])


def test_truncated_sentences_are_reported(setup):
    tts, voice, sentences, rows, toks = setup
    wav, info = tts.inference_long(TEXT, do_sample=False, max_new_tokens=6, trim=False, pause=0.0, return_info=True,
                                   **dict(voice, min_new_tokens=0, allowed_token_ids=sorted(tts._map.sem)))
    assert info["truncated"] == [0, 1, 2, 3, 4] and all(len(t) == 6 for t in info["token_ids"])
    assert wav.size == 5 * 6 * 320 and np.isfinite(wav).all()
    _, info = tts.inference_long(TEXT, do_sample=False, max_new_tokens=BUDGET, trim=False, return_info=True, **voice)
    assert info["truncated"] == [k for k, t in enumerate(toks) if len(t) == BUDGET and t[-1] not in tts._eos]


def test_a_silent_sentence_is_listed_and_gets_no_pause(setup):
    tts, voice, sentences, rows, toks = setup
    peak = [tr.energies(r, W, S).max() for r in rows]
    quiet = int(np.argmin(peak))
    thr = float(np.sqrt(1.01 * peak[quiet] / W))     # just above the quietest row's loudest window
    for r in rows:
        assert tr.closest_to_level(r, W, S, thr) > 1e-4
    wav, info = tts.inference_long(TEXT, do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=FADE, trim_threshold=thr,
                                   return_info=True, **voice)
    want, bounds, offs = _expected(rows, thr)
    assert bounds[quiet] == (0, 0) and quiet in info["silent"] and info["silent"] == [k for k, (a, b) in enumerate(bounds) if a == b]
    assert len(info["silent"]) < 5 and info["offsets"] == offs and np.array_equal(wav, want)
    assert wav.size == sum(b - a for a, b in bounds) + GAP * (5 - len(info["silent"]) - 1)


def test_refusals_before_any_device_call(setup):
    tts, voice, sentences, rows, toks = setup
    for bad in ("", " \n "):
        with pytest.raises(ValueError, match="empty"):
            tts.inference_long(bad, **voice)
        with pytest.raises(ValueError, match="empty"):
            next(tts.inference_long_stream(bad, **voice))
    with pytest.raises(ValueError, match="max_width"):
        tts.inference_long(TEXT, max_width=10, min_width=20, **voice)
    with pytest.raises(ValueError, match="pause"):
        tts.inference_long(TEXT, pause=-1.0, **voice)
    with pytest.raises(ValueError, match="voice"):
        tts.inference_long(TEXT)
    with pytest.raises(ValueError, match="output_sample_rate"):
        tts.inference_long(TEXT, output_sample_rate=0, **voice)


def test_created_voice_continues_from_sentence_0(setup):
    """Voice creation: sentence 0 runs alone, the ids before its first semantic id go behind every later control prompt, and all
    sentences are vocoded with its global tokens.  The synthetic generator knows no prompt layout, so for this test the first
    ``ntok`` ids that sentence 0 generates are declared global tokens in the pipeline's id tables; the yardstick is the LLM's own
    ``serve`` on the prompts the plan prescribes."""
    import copy
    from sparkmi import longform
    from sparkmi.pipeline import _request_sampling
    tts, voice, sentences, rows, toks = setup
    ntok, hop = tts.audio_tokenizer.model.cfg.spk_token_num, tts.audio_tokenizer.model.hop
    style = dict(gender="female", pitch="low", speed="high")
    keys = dict(allowed_token_ids=voice["allowed_token_ids"], min_new_tokens=14)
    samp = _request_sampling(dict(keys), tts.speech_token_ids, tts._eos, tts.model.cfg.vocab_size)
    tokenize = lambda p: tts.tokenizer([p], return_tensors="pt").input_ids[0].tolist()   # noqa: E731
    budget = lambda ids: min(BUDGET, 1024 - len(ids) - 8, 256)   # noqa: E731
    ids0 = longform.control_prompt_ids(tokenize, sentence=sentences[0], **style)
    tts.model.set_sampling(False)
    first = tts._cut_eos(dict(tts.model.serve([(0, ids0, budget(ids0), tts._eos, samp)], max_live=2))[0])
    saved = tts._map
    try:
        # with the real tables sentence 0 has no global block: inference_batch's error
        with pytest.raises(ValueError, match=f"global tokens generated, the speaker encoder needs {ntok}"):
            tts.inference_long(TEXT, do_sample=False, max_new_tokens=BUDGET, **style, **keys)
        tts._map = copy.copy(saved)
        head = first[:ntok]
        tts._map.glob = {t: j for j, t in enumerate(dict.fromkeys(head))}
        tts._map.sem = {t: v for t, v in saved.sem.items() if t not in tts._map.glob}
        assert first[ntok] in tts._map.sem, "the id behind the declared block must be a semantic one for this test"
        prefix, glob = longform.control_prefix(first, tts._map.sem, tts._map.glob, ntok)
        assert prefix == head
        later = [(k, longform.control_prompt_ids(tokenize, sentence=sentences[k], prefix=prefix, **style)) for k in range(1, 5)]
        tts.model.set_sampling(False)
        want = {0: first}
        for k, t in tts.model.serve([(k, ids, budget(ids), tts._eos, samp) for k, ids in later], max_live=2):
            want[k] = tts._cut_eos(t)
        wav, info = tts.inference_long(TEXT, do_sample=False, max_new_tokens=BUDGET, trim=False, pause=PAUSE, fade=0.0, return_info=True,
                                       **style, **keys)
        assert info["token_ids"] == [want[k] for k in range(5)]
        g = torch.tensor(glob, dtype=torch.long)
        parts = []
        for k in range(5):
            w, lens = tts._vocode_rows([tts._speech_row(k, want[k], g)])
            parts += ([np.zeros(GAP, np.float32)] if k else []) + [w[0, : lens[0] * hop].cpu().numpy()]
        assert np.array_equal(wav, np.concatenate(parts))
        assert np.array_equal(np.concatenate(list(tts.inference_long_stream(TEXT, do_sample=False, max_new_tokens=BUDGET, trim=False, pause=PAUSE,
                                                                            fade=0.0, **style, **keys))), wav)
    finally:
        tts._map = saved
