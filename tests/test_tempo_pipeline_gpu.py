"""``tempo`` through SparkTTS on the synthetic model directory (max_batch=2, max_positions=1024, max_frames=256; prompt_tokens
given; greedy; the ids kept on semantic tokens and eos).

Yardstick: the same call without ``tempo`` -- with it, every row is tests/tempo_ref.py's result on that row bit for bit, at the
frame and radius ``audio.tempo_frame`` gives for the model's rate; with ``loudness`` too, the result is the loudness stage's on
those scaled rows."""
import numpy as np
import pytest
import torch

import loud_ref as L
import tempo_ref as R

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence of the paragraph is this one. Then a second one follows it, a little longer than the first! "
        "Is the third one really a question? And the fourth sentence closes the paragraph.")
BUDGET = 40
SR = 16000
PAUSE = 0.25
GAP = 4000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import audio, longform, synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_tempo")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    voice = dict(prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                 allowed_token_ids=sorted(tts._map.sem) + list(tts._eos), min_new_tokens=14)
    sentences = longform.split_text(TEXT, 300, 20)
    assert len(sentences) == 4 and int(tts.sample_rate) == SR
    N, D = audio.tempo_frame(SR)
    reqs = [dict(voice, text=sentences[0]), dict(voice, text=sentences[1])]
    kw = dict(do_sample=False, max_new_tokens=BUDGET)
    plain = tts.inference_batch(reqs, **kw)          # the rows every test scales, once
    return dict(tts=tts, voice=voice, sentences=sentences, reqs=reqs, kw=kw, plain=plain, N=N, D=D)


def _scaled(s, row, tempo):
    from sparkmi.audio import tempo_ratio
    return R.tempo(row, *tempo_ratio(tempo), s["N"], s["D"])[0]


def test_a_batch_at_a_tempo_and_a_request_with_its_own(setup):
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    assert (s["N"], s["D"]) == (512, 240) and p0.size > 4 * s["N"] and p1.size > 4 * s["N"]
    q0, q1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], tempo=0.8)], tempo=1.25, **s["kw"])
    w0, w1 = _scaled(s, p0, 1.25), _scaled(s, p1, 0.8)
    assert q0.size == w0.size == -((-p0.size * 4) // 5) and q1.size == w1.size == -((-p1.size * 5) // 4)
    assert q0.dtype == np.float32 and np.array_equal(_bits(q0), _bits(w0)) and np.array_equal(_bits(q1), _bits(w1))
    assert not np.array_equal(q0, p0[: q0.size])
    # the single-utterance call and serve scale their own rows the same way
    alone = tts.inference(s["sentences"][0], **dict(s["voice"], **s["kw"]))
    assert np.array_equal(_bits(tts.inference(s["sentences"][0], tempo=1.25, **dict(s["voice"], **s["kw"]))), _bits(_scaled(s, alone, 1.25)))
    plain = dict(tts.serve(s["reqs"], **s["kw"]))
    served = dict(tts.serve([s["reqs"][0], dict(s["reqs"][1], tempo=0.8)], tempo=1.25, **s["kw"]))
    assert np.array_equal(_bits(served[0]), _bits(_scaled(s, plain[0], 1.25)))
    assert np.array_equal(_bits(served[1]), _bits(_scaled(s, plain[1], 0.8)))
    # behind the output resampler: the scaled rows resampled
    r0, r1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], tempo=0.8)], tempo=1.25, output_sample_rate=24000, **s["kw"])
    assert r0.size == -((-w0.size * 3) // 2) and r1.size == -((-w1.size * 3) // 2)


def test_loudness_measures_the_scaled_rows(setup):
    from sparkmi import audio
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    q0, q1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], tempo=0.8)], tempo=1.25, loudness=-23.0, **s["kw"])
    coef, block = audio.k_weighting(SR), audio.loudness_block(SR)
    for q, w, d in ((q0, _scaled(s, p0, 1.25), tts.last_loudness[0]), (q1, _scaled(s, p1, 0.8), tts.last_loudness[1])):
        want = L.loudness(w, coef, block, np.longdouble)
        print(f"loudness {d['loudness']!r} (ref on the scaled row {float(want)!r}) gain {d['gain']!r}")
        assert abs(np.longdouble(d["loudness"]) - want) <= L.TOL_LU
        assert np.array_equal(_bits(q), _bits(L.apply_gain(w, d["gain"])))


def test_one_and_none_leave_every_bit(setup):
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    from sparkmi.audio import DeviceAudio
    calls = []
    real = DeviceAudio.tempo_rows
    DeviceAudio.tempo_rows = lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1]
    try:
        for t in (None, 1.0, 1, 0.999):
            q0, q1 = tts.inference_batch(s["reqs"], tempo=t, **s["kw"])
            assert np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(p1))
        q0, q1 = tts.inference_batch([dict(s["reqs"][0], tempo=1.0), s["reqs"][1]], **s["kw"])
        assert np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(p1))
        assert not calls                            # no launch was added
        # one row at 1.0 beside a scaled one goes through the stage at 1/1: still every bit
        q0, q1 = tts.inference_batch([dict(s["reqs"][0], tempo=1.0), s["reqs"][1]], tempo=1.5, **s["kw"])
        assert calls and np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(_scaled(s, p1, 1.5)))
    finally:
        DeviceAudio.tempo_rows = real


def test_inference_long_scales_every_piece_on_its_own(setup):
    s = setup
    tts = s["tts"]
    kw = dict(s["voice"], do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=0.0, trim=False)
    A, ia = tts.inference_long(TEXT, return_info=True, **kw)
    B, ib = tts.inference_long(TEXT, return_info=True, tempo=1.25, **kw)
    assert "tempo_lengths" not in ia and ib["bounds"] == ia["bounds"] and ib["token_ids"] == ia["token_ids"]
    covered = np.zeros(B.size, dtype=bool)
    end = 0
    for k, ((a, b), oa, ob, m) in enumerate(zip(ia["bounds"], ia["offsets"], ib["offsets"], ib["tempo_lengths"])):
        want = _scaled(s, A[oa: oa + b - a], 1.25)
        assert m == want.size == -((-(b - a) * 4) // 5)
        assert ob == end + (GAP if k else 0)        # the pause is seconds of the joined waveform: not scaled
        assert np.array_equal(_bits(B[ob: ob + m]), _bits(want)), k
        covered[ob: ob + m] = True
        end = ob + m
    assert B.size == end and not B[~covered].any() and (~covered).sum() == 3 * GAP
    # the stream's pieces are those of inference_long, and the faded, trimmed, levelled form runs too
    pieces = list(tts.inference_long_stream(TEXT, tempo=1.25, **kw))
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(B))
    full = dict(kw, trim=True, fade=0.005, loudness=-23.0, tempo=0.8)
    C_, ic = tts.inference_long(TEXT, return_info=True, **full)
    assert [m for m in ic["tempo_lengths"]] == [-((-(b - a) * 5) // 4) for a, b in ic["bounds"]]
    assert C_.size == ic["offsets"][-1] + ic["tempo_lengths"][-1]
    assert np.array_equal(_bits(np.concatenate(list(tts.inference_long_stream(TEXT, **full)) + [np.zeros(0, dtype=np.float32)])), _bits(C_))


def test_refusals(setup):
    s = setup
    tts, voice = s["tts"], s["voice"]
    one = [dict(voice, text=s["sentences"][0])]
    with pytest.raises(ValueError, match="tempo"):
        next(tts.inference_stream(s["sentences"][0], tempo=1.25, prompt_tokens=voice["prompt_tokens"]))
    with pytest.raises(ValueError, match="tempo"):
        next(tts.serve_stream(one, tempo=1.25))
    with pytest.raises(ValueError, match="tempo"):
        next(tts.serve_stream([dict(one[0], tempo=1.25)]))
    for bad in (0.4, 2.5, float("nan"), "fast", True):
        with pytest.raises(ValueError):
            tts.inference_batch(one, do_sample=False, tempo=bad)
        with pytest.raises(ValueError):
            tts.inference(s["sentences"][0], do_sample=False, tempo=bad, **voice)
        with pytest.raises(ValueError):
            tts.inference_long(TEXT, tempo=bad, **voice)
        with pytest.raises(ValueError):
            next(tts.inference_long_stream(TEXT, tempo=bad, **voice))
        with pytest.raises(ValueError):
            next(tts.serve(one, do_sample=False, tempo=bad))
    with pytest.raises(ValueError, match="request 0"):
        tts.inference_batch([dict(one[0], tempo=3.0)], do_sample=False)
    with pytest.raises(ValueError, match="request 0"):
        next(tts.serve([dict(one[0], tempo=3.0)], do_sample=False))
