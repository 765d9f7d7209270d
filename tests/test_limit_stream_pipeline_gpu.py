"""``stream_limiter`` through SparkTTS.inference_stream and serve_stream with ``joined=True`` on a synthetic model directory (the
recipe of tests/test_loud_stream_pipeline_gpu.py: clone-mode requests, first chunk 25 frames, overlap 5, budget 48, greedy).

Yardstick per request: tests/limit_ref.py at g = 1 applied to the concatenated pieces of the same call without the limiter, bit for
bit, samples and stats.  The limiter is feed-forward, so the streaming form defines nothing: it is the batch limiter of the whole
stream.  At another output rate the pieces are ``DeviceAudio.resample_rows`` of the limited stream at the model's rate, bit for
bit.  A call without the keyword keeps its bits, ``joined=False`` refuses it, and ``limiter=`` stays refused."""
import math

import numpy as np
import pytest
import torch

import limit_ref as LR

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48
A, R = LR.A0, LR.R0
DELAY = A + R + LR.HALO


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_limit_stream")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=512, max_frames=256)
    assert tts.sample_rate == 16000
    rng = np.random.Generator(np.random.PCG64(31))
    sem_ids = sorted(tts._map.sem)
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"utterance number {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                         allowed_token_ids=list(sem_ids)))
    plain = _serve(tts, reqs)       # today's pieces: joined=True, no limiter anywhere
    return tts, reqs, plain


def _serve(tts, reqs, **kw):
    """{request: [pieces]} of a joined serve_stream call"""
    pieces = {i: [] for i in range(len(reqs))}
    lasts = {i: 0 for i in range(len(reqs))}
    for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, max_new_tokens=BUDGET, joined=True, **dict(STREAM, **kw)):
        assert w.dtype == np.float32 and w.ndim == 1 and not lasts[i], f"request {i}: a piece after its last one"
        pieces[i].append(w)
        lasts[i] += bool(last)
    assert all(v == 1 for v in lasts.values()), "last is on exactly one piece of every request"
    return pieces


def _limit(x, ceiling, mode="true"):
    from sparkmi import audio
    return LR.limit(x, 1.0, ceiling, LR.taps() if mode == "true" else None, A, R, audio.limiter_window(A, R))


def _info(want):
    peak, _, smin, count = want["stats"]
    return dict(true_peak=peak, reduction_db=0.0 if smin >= 1.0 else -20.0 * math.log10(smin), limited_samples=int(count))


def _resampled(tts, x, sr):
    from sparkmi import audio
    up, down = audio.ratio(tts.sample_rate, sr)
    y, n_out = tts._device_audio().resample_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], [up], [down])
    return y.cpu().numpy()[0, : n_out[0]].copy()


@pytest.fixture()
def solo(setup):
    """inference_stream of request 2 with every generated id read as a semantic token (the recipe's greedy stream)"""
    tts, reqs, _ = setup
    r = reqs[2]
    kw = dict(prompt_tokens=r["prompt_tokens"], do_sample=False, max_new_tokens=BUDGET, joined=True, **STREAM)
    size = tts.audio_tokenizer.model.cfg.codebook_size
    parse, eos = tts._parse, tts._eos
    tts._parse, tts._eos = (lambda ids: ([int(t) % size for t in ids], [])), None
    try:
        yield tts, (lambda **more: list(tts.inference_stream(r["text"], **dict(kw, **more))))
    finally:
        tts._parse, tts._eos = parse, eos


def test_inference_stream_with_the_limiter_alone_and_its_first_piece(solo):
    tts, run = solo
    plain = run()
    x = np.concatenate(plain)
    c = float(np.abs(x).max()) / 4.0            # a quarter of the plain run's peak: overs are certain
    for mode in ("true", "sample"):
        want = _limit(x, c, mode)
        tts.last_limiter = "stale"
        got = run(stream_limiter=mode, peak_ceiling=c)
        assert all(w.dtype == np.float32 and w.size for w in got)
        y = np.concatenate(got)
        assert np.array_equal(_bits(y), _bits(want["out"]))
        assert tts.last_limiter == _info(want) and tts.last_limiter["limited_samples"] > 0
        assert float(np.abs(y).max()) <= c
        # the same chunk, A + R + 10 samples shorter: the stage never waits for another chunk
        assert plain[0].size > DELAY and got[0].size == plain[0].size - DELAY
    # another reach: 1 ms and 10 ms
    from sparkmi import audio
    a, r = audio.limiter_reach(16000, 1.0, 10.0)
    want = LR.limit(x, 1.0, c, LR.taps(), a, r, audio.limiter_window(a, r))
    got = run(stream_limiter="true", peak_ceiling=c, limiter_lookahead_ms=1.0, limiter_release_ms=10.0)
    assert np.array_equal(_bits(np.concatenate(got)), _bits(want["out"])) and got[0].size == plain[0].size - (a + r + 10)


def test_inference_stream_with_a_loudness_in_front(solo):
    from sparkmi.pipeline import NO_CEILING
    tts, run = solo
    x = np.concatenate(run())
    c = 10 ** (-1 / 20)
    T = -23.0
    while True:                                  # a target whose gain drives the peak over the ceiling
        z = np.concatenate(run(loudness=T, peak_ceiling=NO_CEILING, max_gain_db=60.0))
        if float(np.abs(z).max()) > 1.5 * c:
            break
        T += 6.0
        assert T < 40.0
    want = _limit(z, c)
    y = np.concatenate(run(loudness=T, max_gain_db=60.0, stream_limiter="true", peak_ceiling=c))
    assert np.array_equal(_bits(y), _bits(want["out"]))
    assert tts.last_limiter == _info(want) and tts.last_limiter["limited_samples"] > 0
    assert tts.last_loudness is not None and float(np.abs(y).max()) <= c


def test_inference_stream_with_a_tempo_at_24_khz(solo):
    tts, run = solo
    xt = np.concatenate(run(tempo=1.25))
    c = float(np.abs(xt).max()) / 4.0
    want = _limit(xt, c)
    y = np.concatenate(run(tempo=1.25, stream_limiter="true", peak_ceiling=c))
    assert np.array_equal(_bits(y), _bits(want["out"]))
    got = np.concatenate(run(tempo=1.25, stream_limiter="true", peak_ceiling=c, output_sample_rate=24000))
    assert np.array_equal(_bits(got), _bits(_resampled(tts, y, 24000)))


@pytest.mark.parametrize("parking", [False, True])
def test_serve_stream_with_three_requests(setup, parking):
    """request 0 takes the call's limiter, request 1 brings its own, request 2 switches it off and is copied through the stage;
    with ``max_open`` above the rows a request parks and keeps its slot"""
    tts, reqs, plain = setup
    c = min(float(np.abs(np.concatenate(plain[i])).max()) for i in plain) / 4.0
    mine = [dict(r) for r in reqs]
    mine[1]["stream_limiter"] = "sample"
    mine[2]["stream_limiter"] = None
    kw = dict(stream_limiter="true", peak_ceiling=c)
    pacer = None
    if parking:
        from sparkmi.streaming import Pacer
        pacer = Pacer(2, 3, 0.05, frame_rate=50, clock=lambda: 0.0)     # the listeners never catch up: the leads only grow
        kw.update(pacer=pacer)
    else:
        kw.update(decode_stride=5)
    got = _serve(tts, mine, **kw)
    assert pacer is None or (pacer.parks >= 1 and pacer.parks == pacer.resumes), (pacer.parks, pacer.resumes)
    for i, mode in ((0, "true"), (1, "sample")):
        want = _limit(np.concatenate(plain[i]), c, mode)
        assert np.array_equal(_bits(np.concatenate(got[i])), _bits(want["out"])), i
        assert tts.last_limiter[i] == _info(want) and tts.last_limiter[i]["limited_samples"] > 0
    assert np.array_equal(_bits(np.concatenate(got[2])), _bits(np.concatenate(plain[2])))
    assert tts.last_limiter[2] is None


def test_a_call_without_the_keyword_keeps_its_bits(setup):
    tts, reqs, plain = setup
    tts._limits = None
    again = _serve(tts, reqs, stream_limiter=None)
    assert all(len(again[i]) == len(plain[i]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[i], plain[i]))
               for i in plain)
    assert tts._limits is None                  # nothing of the stage was built


def test_refusals(setup):
    tts, reqs, _ = setup
    one = [dict(reqs[0])]
    kw = dict(do_sample=False, max_new_tokens=BUDGET, **STREAM)
    with pytest.raises(ValueError, match="stream_limiter"):
        next(tts.inference_stream(reqs[0]["text"], stream_limiter="true", prompt_tokens=reqs[0]["prompt_tokens"], joined=False, **kw))
    with pytest.raises(ValueError, match="joined=True"):
        next(tts.serve_stream(one, stream_limiter="true", **kw))
    with pytest.raises(ValueError, match="stream_limiter"):
        next(tts.serve_stream([dict(one[0], stream_limiter="true")], joined=False, **kw))
    for bad in ("peak", True, 1, 0.5):
        with pytest.raises(ValueError, match="stream_limiter"):
            next(tts.serve_stream(one, stream_limiter=bad, joined=True, **kw))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], stream_limiter=bad)], joined=True, **kw))
        with pytest.raises(ValueError, match="stream_limiter"):
            next(tts.inference_stream(reqs[0]["text"], stream_limiter=bad, prompt_tokens=reqs[0]["prompt_tokens"], joined=True, **kw))
    with pytest.raises(ValueError):
        next(tts.serve_stream(one, stream_limiter="true", limiter_release_ms=1000.0, joined=True, **kw))
    with pytest.raises(ValueError, match="peak_ceiling"):
        next(tts.serve_stream(one, stream_limiter="true", peak_ceiling=0.0, joined=True, **kw))
    with pytest.raises(ValueError, match="list"):        # a limiter of its own from an iterator, in a call that began without the stage
        list(tts.serve_stream(iter([dict(one[0], stream_limiter="true")]), joined=True, **kw))
    # limiter= names the limiter of whole utterances and stays refused, joined or not; the message names the new keyword
    for joined in (False, True):
        with pytest.raises(ValueError, match="stream_limiter="):
            next(tts.inference_stream(reqs[0]["text"], limiter="true", prompt_tokens=reqs[0]["prompt_tokens"], joined=joined, **kw))
        with pytest.raises(ValueError, match="limiter"):
            next(tts.serve_stream(one, limiter="true", joined=joined, **kw))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], limiter="sample")], joined=joined, **kw))
