"""``stream_pitch_shift`` through SparkTTS.inference_stream and serve_stream with ``joined=True`` on a synthetic model directory
(the recipe of tests/test_tempo_stream_pipeline_gpu.py: clone-mode requests, first chunk 25 frames, overlap 5, budget 48).

Yardstick per request: ``pitch_ref.pitch`` of the concatenated ``joined=True`` pieces of the same call without the keyword, at
``audio.tempo_frame(sr)`` -- the pieces' concatenation with it must equal that bit for bit --; with a tempo in the same pass, at
another output rate (``DeviceAudio.resample_rows`` of that), with the loudness and limiter stages behind it, with parking on and
with a request that brings its own key.  A call without any shift keeps its bits and builds nothing."""
import numpy as np
import pytest
import torch

import pitch_ref as pr

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_pitch_stream")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=512, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(29))
    sem_ids = sorted(tts._map.sem)
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"utterance number {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                         allowed_token_ids=list(sem_ids)))
    plain = _serve(tts, reqs)       # today's pieces: joined=True, no shift anywhere
    hop = tts.audio_tokenizer.model.hop
    assert all(np.concatenate(p).size == BUDGET * hop for p in plain.values())
    return tts, reqs, plain


_YARD = {}


def _shifted(tts, x, semitones, tempo=None):
    """``pitch_ref.pitch`` of ``x``, computed once per (signal, shift, tempo)"""
    from sparkmi import audio
    key = (_bits(x).tobytes(), semitones, tempo)
    if key not in _YARD:
        N, D = audio.tempo_frame(tts.sample_rate)
        _YARD[key] = pr.pitch(x, (1, 1) if tempo is None else audio.tempo_ratio(tempo), audio.pitch_ratio(semitones), N, D)[0]
    return _YARD[key]


def _resampled(tts, x, sr):
    from sparkmi import audio
    up, down = audio.ratio(tts.sample_rate, sr)
    y, n_out = tts._device_audio().resample_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], [up], [down])
    return y.cpu().numpy()[0, : n_out[0]].copy()


def test_inference_stream_with_a_shift_a_tempo_and_a_rate(setup):
    from sparkmi import audio
    tts, reqs, _ = setup
    r = reqs[2]
    kw = dict(prompt_tokens=r["prompt_tokens"], do_sample=False, max_new_tokens=BUDGET, joined=True, **STREAM)
    size = tts.audio_tokenizer.model.cfg.codebook_size
    # (inference_stream takes no allowed_token_ids: every id is read as a semantic token, as in the joined test)
    parse, eos = tts._parse, tts._eos
    tts._parse, tts._eos = (lambda ids: ([int(t) % size for t in ids], [])), None
    try:
        plain = list(tts.inference_stream(r["text"], **kw))
        x = np.concatenate(plain)
        tts._pitchs = None
        for none in (None, 0, 0.05):          # nothing is built and no bit moves
            again = list(tts.inference_stream(r["text"], stream_pitch_shift=none, **kw))
            assert len(again) == len(plain) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again, plain))
        assert tts._pitchs is None
        got = list(tts.inference_stream(r["text"], stream_pitch_shift=2, **kw))
        assert len(got) >= 2 and all(w.dtype == np.float32 and w.size for w in got)
        assert np.array_equal(_bits(np.concatenate(got)), _bits(_shifted(tts, x, 2)))
        assert sum(w.size for w in got) == x.size                               # the length is unchanged
        # with a tempo: one pass, and the length is the one tempo alone gives
        want = _shifted(tts, x, 2, 1.25)
        got = np.concatenate(list(tts.inference_stream(r["text"], stream_pitch_shift=2, tempo=1.25, **kw)))
        alone = np.concatenate(list(tts.inference_stream(r["text"], tempo=1.25, **kw)))
        assert got.size == alone.size == audio.tempo_len(x.size, 5, 4) and np.array_equal(_bits(got), _bits(want))
        got = np.concatenate(list(tts.inference_stream(r["text"], stream_pitch_shift=2, tempo=1.25, output_sample_rate=24000, **kw)))
        assert np.array_equal(_bits(got), _bits(_resampled(tts, want, 24000)))
    finally:
        tts._parse, tts._eos = parse, eos


def test_the_loudness_and_limiter_stages_see_the_shifted_stream(setup):
    """the stages run in order: the limiter's pieces are tests/limit_ref.py of the shifted stream, the loudness stage's those of
    tests/loud_stream_ref.py on it and its measure the batch measure of the shifted utterance, and with both the limiter works
    behind the running gain"""
    import limit_ref as LR
    import loud_stream_ref as S
    from sparkmi import audio
    from sparkmi.pipeline import NO_CEILING
    tts, reqs, plain = setup
    one = [reqs[0]]
    run = lambda **kw: np.concatenate(_serve(tts, one, stream_pitch_shift=-2, **kw)[0])   # noqa: E731
    limit = lambda x, c: LR.limit(x, 1.0, c, LR.taps(), LR.A0, LR.R0, audio.limiter_window(LR.A0, LR.R0))   # noqa: E731
    x = run()
    assert np.array_equal(_bits(x), _bits(_shifted(tts, np.concatenate(plain[0]), -2)))
    c = float(np.abs(x).max()) / 4.0            # a quarter of the shifted run's peak: overs are certain
    want = limit(x, c)
    assert np.array_equal(_bits(run(stream_limiter="true", peak_ceiling=c)), _bits(want["out"]))
    assert tts.last_limiter[0]["limited_samples"] == int(want["stats"][3]) > 0
    # the loudness stage: the running gain of the shifted stream, and the batch measure of the shifted utterance
    block, coef = audio.loudness_block(tts.sample_rate), audio.k_weighting(tts.sample_rate)
    ref = S.stream(x, coef, block, -23.0, dt=np.longdouble)
    y, yard = run(loudness=-23.0), S.apply(x, ref["G"], block // 4)
    d = np.abs(y.astype(np.float64) - yard.astype(np.float64))
    assert y.size == yard.size and np.all(d <= np.spacing(np.abs(yard)).astype(np.float64))   # one fp32 ulp, as that stage's own test
    st = tts._device_audio().loudness_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], sr=tts.sample_rate)
    batch = st.cpu().numpy()[0]
    assert tts.last_loudness[0]["loudness"] == batch[0] and tts.last_loudness[0]["peak"] == batch[1]
    # all three: the limiter behind the gain behind the shift
    z = run(loudness=-10.0, peak_ceiling=NO_CEILING, max_gain_db=60.0)
    cz = float(np.abs(z).max()) / 2.0
    both = run(loudness=-10.0, max_gain_db=60.0, stream_limiter="true", peak_ceiling=cz)
    assert np.array_equal(_bits(both), _bits(limit(z, cz)["out"])) and float(np.abs(both).max()) <= cz


def test_serve_stream_with_shifts_and_parking(setup):
    """three requests on two rows, all three open, a request parked as soon as it is 50 ms ahead of its listener; request 1
    brings its own shift -2 under the call's +2, request 2 its own 0: its bits are those of the call without the keyword"""
    from sparkmi.streaming import Pacer
    tts, reqs, plain = setup
    mine = [dict(r) for r in reqs]
    mine[1]["stream_pitch_shift"] = -2
    mine[2]["stream_pitch_shift"] = 0
    want = {0: _shifted(tts, np.concatenate(plain[0]), 2), 1: _shifted(tts, np.concatenate(plain[1]), -2), 2: np.concatenate(plain[2])}

    class Clock:
        t = 0.0

        def __call__(self):
            return self.t

    clk = Clock()
    pacer = Pacer(2, 3, 0.05, frame_rate=50, clock=clk)
    pieces = {i: [] for i in plain}
    heard = {}
    for i, w, last in tts.serve_stream([dict(r) for r in mine], do_sample=False, max_new_tokens=BUDGET, joined=True, stream_pitch_shift=2,
                                       pacer=pacer, **STREAM):
        pieces[i].append(w)
        if not last:
            heard[i] = pacer.lead(i, pacer._first[i])     # the seconds counted for request i so far
        clk.t += 0.01
    assert pacer.parks >= 1 and pacer.parks == pacer.resumes, (pacer.parks, pacer.resumes)
    for i in plain:
        got = np.concatenate(pieces[i])
        assert got.size == want[i].size and np.array_equal(_bits(got), _bits(want[i])), i
    for i, lead in heard.items():   # the pacer counted what the listener received: the pieces behind stage 1
        assert lead == pytest.approx(sum(w.size for w in pieces[i][:-1]) / tts.sample_rate)


def test_a_request_with_its_own_key_beside_others_and_a_call_without_any(setup):
    tts, reqs, plain = setup
    mine = [dict(r) for r in reqs]
    mine[0]["stream_pitch_shift"] = 7
    mine[1]["tempo"] = 0.8
    got = _serve(tts, mine, decode_stride=5)             # no call shift: request 2 copies through at 1/1 and 1/1
    assert np.array_equal(_bits(np.concatenate(got[0])), _bits(_shifted(tts, np.concatenate(plain[0]), 7)))
    alone = _serve(tts, [dict(reqs[1], tempo=0.8)])[0]   # the tempo stream's bits
    assert np.array_equal(_bits(np.concatenate(got[1])), _bits(np.concatenate(alone)))
    assert np.array_equal(_bits(np.concatenate(got[2])), _bits(np.concatenate(plain[2])))
    assert [w.size for w in got[2]] == [w.size for w in plain[2]]       # with no latency
    # None, 0 and a ratio of 1/1 everywhere: today's pieces, piece by piece, and nothing of the pitch stage is built
    tts._pitchs = None
    for kw in (dict(stream_pitch_shift=None), dict(stream_pitch_shift=0), dict(stream_pitch_shift=0.05)):
        again = _serve(tts, reqs, **kw)
        assert all(len(again[i]) == len(plain[i]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[i], plain[i]))
                   for i in plain)
    assert tts._pitchs is None


def test_refusals(setup):
    tts, reqs, _ = setup
    one = [dict(reqs[0])]
    kw = dict(do_sample=False, max_new_tokens=BUDGET, **STREAM)
    with pytest.raises(ValueError, match="stream_pitch_shift"):
        next(tts.inference_stream(reqs[0]["text"], stream_pitch_shift=2, prompt_tokens=reqs[0]["prompt_tokens"], joined=False, **kw))
    with pytest.raises(ValueError, match="stream_pitch_shift.*joined=True"):
        next(tts.serve_stream(one, stream_pitch_shift=2, **kw))
    with pytest.raises(ValueError, match="stream_pitch_shift.*joined=True"):
        next(tts.serve_stream([dict(one[0], stream_pitch_shift=2)], joined=False, **kw))
    for bad in (12.5, -13, float("nan"), "high", True):
        with pytest.raises(ValueError, match="stream_pitch_shift"):
            next(tts.serve_stream(one, stream_pitch_shift=bad, joined=True, **kw))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], stream_pitch_shift=bad)], joined=True, **kw))
        with pytest.raises(ValueError, match="stream_pitch_shift"):
            next(tts.inference_stream(reqs[0]["text"], stream_pitch_shift=bad, prompt_tokens=reqs[0]["prompt_tokens"], joined=True, **kw))
    with pytest.raises(ValueError, match="list"):        # a shift of its own from an iterator, in a call that began without the stage
        list(tts.serve_stream(iter([dict(one[0], stream_pitch_shift=2)]), joined=True, **kw))
    with pytest.raises(ValueError, match="the batch calls take it"):   # the batch keyword stays refused on the streams
        next(tts.serve_stream(one, pitch_shift=2, joined=True, **kw))
