"""``tempo`` through SparkTTS.inference_stream and serve_stream with ``joined=True`` on a synthetic model directory (the recipe of
tests/test_stream_join_pipeline_gpu.py: clone-mode requests, first chunk 25 frames, overlap 5, budget 48).

Yardstick per request: ``tempo_ref.tempo`` of the concatenated ``joined=True`` pieces without tempo at ``audio.tempo_frame(sr)`` --
the pieces' concatenation with tempo must equal it bit for bit -- and, at another output rate, ``DeviceAudio.resample_rows`` of
that; with parking on and a request that brings its own tempo.  A call without any tempo keeps its bits, and ``joined=False``
still refuses one."""
import numpy as np
import pytest
import torch

import tempo_ref as tr

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_tempo_stream")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=512, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    sem_ids = sorted(tts._map.sem)
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"utterance number {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                         allowed_token_ids=list(sem_ids)))
    plain = _serve(tts, reqs)       # today's pieces: joined=True, no tempo anywhere
    hop = tts.audio_tokenizer.model.hop
    assert all(np.concatenate(p).size == BUDGET * hop for p in plain.values())
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


def _scaled(tts, x, tempo):
    from sparkmi import audio
    N, D = audio.tempo_frame(tts.sample_rate)
    return tr.tempo(x, *audio.tempo_ratio(tempo), N, D)[0]


def _resampled(tts, x, sr):
    from sparkmi import audio
    up, down = audio.ratio(tts.sample_rate, sr)
    y, n_out = tts._device_audio().resample_rows(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(), [x.size], [up], [down])
    return y.cpu().numpy()[0, : n_out[0]].copy()


def test_inference_stream_with_a_tempo(setup):
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
        assert np.array_equal(_bits(np.concatenate(list(tts.inference_stream(r["text"], tempo=1.0, **kw)))), _bits(x))
        want = _scaled(tts, x, 1.25)
        got = list(tts.inference_stream(r["text"], tempo=1.25, **kw))
        assert len(got) >= 2 and all(w.dtype == np.float32 and w.size for w in got)
        assert np.array_equal(_bits(np.concatenate(got)), _bits(want))
        got = np.concatenate(list(tts.inference_stream(r["text"], tempo=1.25, output_sample_rate=24000, **kw)))
        assert np.array_equal(_bits(got), _bits(_resampled(tts, want, 24000)))
    finally:
        tts._parse, tts._eos = parse, eos


def test_serve_stream_with_tempos_and_parking(setup):
    """three requests on two rows, all three open, a request parked as soon as it is 50 ms ahead of its listener; request 1
    brings its own tempo 0.8 under the call's 1.25"""
    from sparkmi.streaming import Pacer
    tts, reqs, plain = setup
    mine = [dict(r) for r in reqs]
    mine[1]["tempo"] = 0.8
    want = {i: _scaled(tts, np.concatenate(plain[i]), 0.8 if i == 1 else 1.25) for i in plain}

    class Clock:
        t = 0.0

        def __call__(self):
            return self.t

    for sr in (None, 24000):
        clk = Clock()
        pacer = Pacer(2, 3, 0.05, frame_rate=50, clock=clk)
        pieces = {i: [] for i in plain}
        heard = {}
        for i, w, last in tts.serve_stream([dict(r) for r in mine], do_sample=False, max_new_tokens=BUDGET, joined=True, tempo=1.25,
                                           pacer=pacer, output_sample_rate=sr, **STREAM):
            pieces[i].append(w)
            if not last:
                heard[i] = pacer.lead(i, pacer._first[i])     # the seconds counted for request i so far
            clk.t += 0.01
        assert pacer.parks >= 1 and pacer.parks == pacer.resumes, (pacer.parks, pacer.resumes)
        for i in plain:
            yard = want[i] if sr is None else _resampled(tts, want[i], sr)
            got = np.concatenate(pieces[i])
            assert got.size == yard.size and np.array_equal(_bits(got), _bits(yard)), (i, sr)
        if sr is None:       # the pacer counted what the listener received: the scaled pieces at the model's rate
            for i, lead in heard.items():
                assert lead == pytest.approx(sum(w.size for w in pieces[i][:-1]) / tts.sample_rate)


def test_a_request_without_tempo_beside_others_and_a_call_without_any(setup):
    tts, reqs, plain = setup
    mine = [dict(r) for r in reqs]
    mine[0]["tempo"] = 1.5
    got = _serve(tts, mine, decode_stride=5)             # no call tempo: requests 1 and 2 copy through streams at 1/1
    assert np.array_equal(_bits(np.concatenate(got[0])), _bits(_scaled(tts, np.concatenate(plain[0]), 1.5)))
    for i in (1, 2):
        assert np.array_equal(_bits(np.concatenate(got[i])), _bits(np.concatenate(plain[i])))
    # tempo=None (and 1.0) everywhere: today's pieces, piece by piece, and nothing of the tempo stage is built
    tts._tempos = None
    for kw in (dict(tempo=None), dict(tempo=1.0)):
        again = _serve(tts, reqs, **kw)
        assert all(len(again[i]) == len(plain[i]) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(again[i], plain[i]))
                   for i in plain)
    assert tts._tempos is None


def test_refusals(setup):
    tts, reqs, _ = setup
    one = [dict(reqs[0])]
    kw = dict(do_sample=False, max_new_tokens=BUDGET, **STREAM)
    with pytest.raises(ValueError, match="tempo"):
        next(tts.inference_stream(reqs[0]["text"], tempo=1.25, prompt_tokens=reqs[0]["prompt_tokens"], joined=False, **kw))
    with pytest.raises(ValueError, match="joined=True"):
        next(tts.serve_stream(one, tempo=1.25, **kw))
    with pytest.raises(ValueError, match="tempo"):
        next(tts.serve_stream([dict(one[0], tempo=1.25)], joined=False, **kw))
    for bad in (0.4, 2.5, float("nan"), "fast", True):
        with pytest.raises(ValueError):
            next(tts.serve_stream(one, tempo=bad, joined=True, **kw))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], tempo=bad)], joined=True, **kw))
        with pytest.raises(ValueError):
            next(tts.inference_stream(reqs[0]["text"], tempo=bad, prompt_tokens=reqs[0]["prompt_tokens"], joined=True, **kw))
    with pytest.raises(ValueError, match="list"):        # a tempo of its own from an iterator, in a call that began without the stages
        list(tts.serve_stream(iter([dict(one[0], tempo=1.25)]), joined=True, **kw))
