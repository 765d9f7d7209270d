"""``loudness`` through SparkTTS.inference_stream and serve_stream with ``joined=True`` on a synthetic model directory (the recipe of
tests/test_tempo_stream_pipeline_gpu.py: clone-mode requests, first chunk 25 frames, overlap 5, budget 48).

Yardstick per request: tests/loud_stream_ref.py (longdouble knots, the header's sample formula) applied to the concatenated pieces
of the same call without ``loudness``.  The knot gains agree within ``TOL_GAIN`` = 1e-12 relative, far below half an fp32 ulp, so
a sample can differ from the yardstick's by one fp32 ulp at most, and only where fl64(x) g lies within 1e-12 of a rounding
boundary.  At another output rate the pieces are ``DeviceAudio.resample_rows`` of the same call's pieces at the model's rate, bit
for bit.  A call without any loudness keeps its bits, and ``joined=False`` refuses one."""
import numpy as np
import pytest
import torch

import loud_stream_ref as S

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_loud_stream")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=512, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(29))
    sem_ids = sorted(tts._map.sem)
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"utterance number {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                         allowed_token_ids=list(sem_ids)))
    plain = _serve(tts, reqs)       # today's pieces: joined=True, no loudness anywhere
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


def _yardstick(tts, x, target, **kw):
    from sparkmi import audio
    block = audio.loudness_block(tts.sample_rate)
    coef = audio.k_weighting(tts.sample_rate)
    r = S.stream(x, coef, block, target, dt=np.longdouble, **kw)
    return S.apply(x, r["G"], block // 4), r


def _close(got, want):
    """equal up to one fp32 ulp (the module's docstring), and almost everywhere bit for bit"""
    assert got.size == want.size
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(d <= np.spacing(np.abs(want)).astype(np.float64)), float(d.max())
    assert np.count_nonzero(d) <= max(1, got.size // 1000)


def _resampled(tts, x, sr):
    from sparkmi import audio
    up, down = audio.ratio(tts.sample_rate, sr)
    y, n_out = tts._device_audio().resample_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], [up], [down])
    return y.cpu().numpy()[0, : n_out[0]].copy()


def _batch_measure(tts, x):
    st = tts._device_audio().loudness_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], sr=tts.sample_rate)
    return st.cpu().numpy()[0]


def test_inference_stream_with_a_loudness(setup):
    tts, reqs, _ = setup
    r = reqs[2]
    kw = dict(prompt_tokens=r["prompt_tokens"], do_sample=False, max_new_tokens=BUDGET, joined=True, **STREAM)
    size = tts.audio_tokenizer.model.cfg.codebook_size
    parse, eos = tts._parse, tts._eos
    tts._parse, tts._eos = (lambda ids: ([int(t) % size for t in ids], [])), None
    try:
        x = np.concatenate(list(tts.inference_stream(r["text"], **kw)))
        want, ref = _yardstick(tts, x, -23.0)
        got = list(tts.inference_stream(r["text"], loudness=-23.0, **kw))
        assert all(w.dtype == np.float32 and w.size for w in got)
        y = np.concatenate(got)
        _close(y, want)
        info = tts.last_loudness
        batch = _batch_measure(tts, x)
        assert info["loudness"] == batch[0] and info["peak"] == batch[1]          # the whole utterance's, the batch measure
        assert abs(info["gain"] / float(ref["G"][-1]) - 1) <= S.TOL_GAIN and info["flags"] == int(np.bitwise_or.reduce(ref["flags"]))
        assert float(np.abs(y).max()) <= 10 ** (-1 / 20) * (1 + 2.0 ** -23)
        # behind the tempo stage and before the resampler with state
        from sparkmi import audio
        import tempo_ref as tr
        xt = tr.tempo(x, *audio.tempo_ratio(1.25), *audio.tempo_frame(tts.sample_rate))[0]
        yt = np.concatenate(list(tts.inference_stream(r["text"], loudness=-23.0, tempo=1.25, **kw)))
        _close(yt, _yardstick(tts, xt, -23.0)[0])
        got = np.concatenate(list(tts.inference_stream(r["text"], loudness=-23.0, tempo=1.25, output_sample_rate=24000, **kw)))
        assert np.array_equal(_bits(got), _bits(_resampled(tts, yt, 24000)))
        got = np.concatenate(list(tts.inference_stream(r["text"], loudness=-23.0, output_sample_rate=24000, **kw)))
        assert np.array_equal(_bits(got), _bits(_resampled(tts, y, 24000)))
    finally:
        tts._parse, tts._eos = parse, eos


def test_serve_stream_with_three_requests(setup):
    """the call's target for request 0, request 1 brings its own, request 2 switches its target off and is measured and copied;
    the call's ``max_slew_db`` holds for all"""
    tts, reqs, plain = setup
    mine = [dict(r) for r in reqs]
    mine[1]["loudness"] = -16.0
    mine[2]["loudness"] = None
    got = _serve(tts, mine, loudness=-23.0, max_slew_db=2.0, decode_stride=5)
    for i, target in ((0, -23.0), (1, -16.0)):
        x = np.concatenate(plain[i])
        want, ref = _yardstick(tts, x, target, max_slew_db=2.0)
        _close(np.concatenate(got[i]), want)
        info = tts.last_loudness[i]
        assert info["loudness"] == _batch_measure(tts, x)[0]
        assert abs(info["gain"] / float(ref["G"][-1]) - 1) <= S.TOL_GAIN and info["flags"] == int(np.bitwise_or.reduce(ref["flags"]))
    assert np.array_equal(_bits(np.concatenate(got[2])), _bits(np.concatenate(plain[2])))
    assert tts.last_loudness[2]["gain"] == 1.0 and tts.last_loudness[2]["flags"] == 0
    assert tts.last_loudness[2]["loudness"] == _batch_measure(tts, np.concatenate(plain[2]))[0]


def test_a_call_without_any_loudness_keeps_its_bits(setup):
    tts, reqs, plain = setup
    tts._louds = None
    again = _serve(tts, reqs, loudness=None)
    assert all(len(again[i]) == len(plain[i]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[i], plain[i]))
               for i in plain)
    assert tts._louds is None                   # nothing of the stage was built


def test_refusals(setup):
    tts, reqs, _ = setup
    one = [dict(reqs[0])]
    kw = dict(do_sample=False, max_new_tokens=BUDGET, **STREAM)
    with pytest.raises(ValueError, match="loudness"):
        next(tts.inference_stream(reqs[0]["text"], loudness=-23.0, prompt_tokens=reqs[0]["prompt_tokens"], joined=False, **kw))
    with pytest.raises(ValueError, match="joined=True"):
        next(tts.serve_stream(one, loudness=-23.0, **kw))
    with pytest.raises(ValueError, match="loudness"):
        next(tts.serve_stream([dict(one[0], loudness=-23.0)], joined=False, **kw))
    for bad in (float("nan"), float("inf"), "loud", True):
        with pytest.raises(ValueError):
            next(tts.serve_stream(one, loudness=bad, joined=True, **kw))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], loudness=bad)], joined=True, **kw))
        with pytest.raises(ValueError):
            next(tts.inference_stream(reqs[0]["text"], loudness=bad, prompt_tokens=reqs[0]["prompt_tokens"], joined=True, **kw))
    with pytest.raises(ValueError, match="max_slew_db"):
        next(tts.serve_stream(one, loudness=-23.0, max_slew_db=-1.0, joined=True, **kw))
    with pytest.raises(ValueError, match="list"):        # a loudness of its own from an iterator, in a call that began without the stage
        list(tts.serve_stream(iter([dict(one[0], loudness=-23.0)]), joined=True, **kw))
