"""``pitch_shift`` through SparkTTS on the synthetic model directory (max_batch=2, max_positions=1024, max_frames=256;
prompt_tokens given; greedy; the ids kept on semantic tokens and eos).

Yardstick: the same call without ``pitch_shift`` -- with it, every row is tests/pitch_ref.py's result on that row bit for bit, at
the frame and radius ``audio.tempo_frame`` gives for the model's rate and at the call's tempo, in one stretch pass; with
``loudness`` too, the result is the loudness stage's on those shifted rows."""
import numpy as np
import pytest
import torch

import loud_ref as L
import pitch_ref as R

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
    d = tmp_path_factory.mktemp("spark_synth_pitch")
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
    plain = tts.inference_batch(reqs, **kw)          # the rows every test shifts, once
    return dict(tts=tts, voice=voice, sentences=sentences, reqs=reqs, kw=kw, plain=plain, N=N, D=D)


def _shifted(s, row, semitones, tempo=None):
    from sparkmi.audio import pitch_ratio, tempo_ratio
    t = (1, 1) if tempo is None else tempo_ratio(tempo)
    r = (1, 1) if semitones is None else pitch_ratio(semitones)
    return R.pitch(row, t, r, s["N"], s["D"])[0]


def test_a_batch_at_a_shift_and_a_request_with_its_own(setup):
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    assert (s["N"], s["D"]) == (512, 240) and p0.size > 4 * s["N"] and p1.size > 4 * s["N"]
    q0, q1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], pitch_shift=-2)], pitch_shift=2.0, **s["kw"])
    w0, w1 = _shifted(s, p0, 2.0), _shifted(s, p1, -2)
    assert q0.size == w0.size == p0.size and q1.size == w1.size == p1.size      # the length stays
    assert q0.dtype == np.float32 and np.array_equal(_bits(q0), _bits(w0)) and np.array_equal(_bits(q1), _bits(w1))
    assert not np.array_equal(q0, p0)
    # the single-utterance call and serve shift their own rows the same way
    alone = tts.inference(s["sentences"][0], **dict(s["voice"], **s["kw"]))
    assert np.array_equal(_bits(tts.inference(s["sentences"][0], pitch_shift=7, **dict(s["voice"], **s["kw"]))), _bits(_shifted(s, alone, 7)))
    plain = dict(tts.serve(s["reqs"], **s["kw"]))
    served = dict(tts.serve([s["reqs"][0], dict(s["reqs"][1], pitch_shift=-2)], pitch_shift=2.0, **s["kw"]))
    assert np.array_equal(_bits(served[0]), _bits(_shifted(s, plain[0], 2.0)))
    assert np.array_equal(_bits(served[1]), _bits(_shifted(s, plain[1], -2)))
    # behind the output resampler: the shifted rows resampled
    r0, r1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], pitch_shift=-2)], pitch_shift=2.0, output_sample_rate=24000, **s["kw"])
    assert r0.size == -((-w0.size * 3) // 2) and r1.size == -((-w1.size * 3) // 2)


def test_with_tempo_in_one_pass(setup):
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    # row 0: the call's tempo and shift; row 1: its own tempo and no shift -- tempo_rows' row, through the pitch stage
    q0, q1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], tempo=0.8, pitch_shift=0)], tempo=1.25, pitch_shift=3, **s["kw"])
    w0, w1 = _shifted(s, p0, 3, 1.25), _shifted(s, p1, None, 0.8)
    assert q0.size == w0.size == -((-p0.size * 4) // 5) and q1.size == w1.size == -((-p1.size * 5) // 4)
    assert np.array_equal(_bits(q0), _bits(w0)) and np.array_equal(_bits(q1), _bits(w1))
    assert not np.array_equal(_bits(q0), _bits(R.pitch(p0, (5, 4), (119, 100), s["N"], s["D"], wrong="two_pass")[0]))
    served = dict(tts.serve([s["reqs"][0]], tempo=1.25, pitch_shift=3, **s["kw"]))
    assert np.array_equal(_bits(served[0]), _bits(w0))


def test_loudness_measures_the_shifted_rows(setup):
    from sparkmi import audio
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    q0, q1 = tts.inference_batch([s["reqs"][0], dict(s["reqs"][1], pitch_shift=-2)], pitch_shift=2.0, loudness=-23.0, **s["kw"])
    coef, block = audio.k_weighting(SR), audio.loudness_block(SR)
    for q, w, d in ((q0, _shifted(s, p0, 2.0), tts.last_loudness[0]), (q1, _shifted(s, p1, -2), tts.last_loudness[1])):
        want = L.loudness(w, coef, block, np.longdouble)
        print(f"loudness {d['loudness']!r} (ref on the shifted row {float(want)!r}) gain {d['gain']!r}")
        assert abs(np.longdouble(d["loudness"]) - want) <= L.TOL_LU
        assert np.array_equal(_bits(q), _bits(L.apply_gain(w, d["gain"])))


def test_zero_and_none_leave_every_bit(setup):
    s = setup
    tts, (p0, p1) = s["tts"], s["plain"]
    from sparkmi.audio import DeviceAudio
    calls = []
    real = DeviceAudio.pitch_rows, DeviceAudio.tempo_rows
    DeviceAudio.pitch_rows = lambda self, *a, **k: (calls.append("pitch"), real[0](self, *a, **k))[1]
    DeviceAudio.tempo_rows = lambda self, *a, **k: (calls.append("tempo"), real[1](self, *a, **k))[1]
    try:
        for v in (None, 0, 0.0, 0.05, -0.05):      # (a twentieth of a semitone is below the ratio's resolution: 1/1)
            q0, q1 = tts.inference_batch(s["reqs"], pitch_shift=v, **s["kw"])
            assert np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(p1))
        q0, q1 = tts.inference_batch([dict(s["reqs"][0], pitch_shift=0), s["reqs"][1]], **s["kw"])
        assert np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(p1))
        assert not calls                            # no launch was added
        # a call with a tempo and no shift goes through the tempo stage, as before
        tts.inference_batch(s["reqs"], tempo=1.25, pitch_shift=0, **s["kw"])
        assert calls == ["tempo"]
        # one row at 0 beside a shifted one goes through the pitch stage at 1/1: still every bit
        del calls[:]
        q0, q1 = tts.inference_batch([dict(s["reqs"][0], pitch_shift=0), s["reqs"][1]], pitch_shift=4, **s["kw"])
        assert calls == ["pitch"] and np.array_equal(_bits(q0), _bits(p0)) and np.array_equal(_bits(q1), _bits(_shifted(s, p1, 4)))
    finally:
        DeviceAudio.pitch_rows, DeviceAudio.tempo_rows = real


def test_inference_long_shifts_every_piece_on_its_own(setup):
    s = setup
    tts = s["tts"]
    kw = dict(s["voice"], do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=0.0, trim=False)
    A, ia = tts.inference_long(TEXT, return_info=True, **kw)
    B, ib = tts.inference_long(TEXT, return_info=True, pitch_shift=-3, **kw)
    assert "tempo_lengths" not in ib and ib["bounds"] == ia["bounds"] and ib["token_ids"] == ia["token_ids"]
    assert ib["offsets"] == ia["offsets"] and B.size == A.size      # the pieces keep their lengths and their places
    covered = np.zeros(B.size, dtype=bool)
    for k, ((a, b), o) in enumerate(zip(ia["bounds"], ia["offsets"])):
        assert np.array_equal(_bits(B[o: o + b - a]), _bits(_shifted(s, A[o: o + b - a], -3))), k
        covered[o: o + b - a] = True
    assert not B[~covered].any() and (~covered).sum() == 3 * GAP
    # the stream's pieces are those of inference_long
    pieces = list(tts.inference_long_stream(TEXT, pitch_shift=-3, **kw))
    assert np.array_equal(_bits(np.concatenate(pieces)), _bits(B))
    # with a tempo: one pass a piece, the lengths the tempo alone gives
    C_, ic = tts.inference_long(TEXT, return_info=True, tempo=1.25, pitch_shift=2, **kw)
    for k, ((a, b), oa, oc, m) in enumerate(zip(ia["bounds"], ia["offsets"], ic["offsets"], ic["tempo_lengths"])):
        want = _shifted(s, A[oa: oa + b - a], 2, 1.25)
        assert m == want.size == -((-(b - a) * 4) // 5)
        assert np.array_equal(_bits(C_[oc: oc + m]), _bits(want)), k
    # the faded, trimmed, levelled form runs too, and its stream gives the same bits
    full = dict(kw, trim=True, fade=0.005, loudness=-23.0, tempo=0.8, pitch_shift=5)
    E, ie = tts.inference_long(TEXT, return_info=True, **full)
    assert [m for m in ie["tempo_lengths"]] == [-((-(b - a) * 5) // 4) for a, b in ie["bounds"]]
    assert E.size == ie["offsets"][-1] + ie["tempo_lengths"][-1]
    assert np.array_equal(_bits(np.concatenate(list(tts.inference_long_stream(TEXT, **full)) + [np.zeros(0, dtype=np.float32)])), _bits(E))


def test_refusals(setup):
    s = setup
    tts, voice = s["tts"], s["voice"]
    one = [dict(voice, text=s["sentences"][0])]
    for joined in (False, True):
        with pytest.raises(ValueError, match="pitch_shift.*the batch calls take it"):
            next(tts.inference_stream(s["sentences"][0], pitch_shift=2, joined=joined, prompt_tokens=voice["prompt_tokens"]))
        with pytest.raises(ValueError, match="pitch_shift.*the batch calls take it"):
            next(tts.serve_stream(one, pitch_shift=2, joined=joined))
        with pytest.raises(ValueError, match="request 0.*pitch_shift.*the batch calls take it"):
            next(tts.serve_stream([dict(one[0], pitch_shift=2)], joined=joined))
    for bad in (-12.5, 13, float("nan"), "high", True):
        with pytest.raises(ValueError):
            tts.inference_batch(one, do_sample=False, pitch_shift=bad)
        with pytest.raises(ValueError):
            tts.inference(s["sentences"][0], do_sample=False, pitch_shift=bad, **voice)
        with pytest.raises(ValueError):
            tts.inference_long(TEXT, pitch_shift=bad, **voice)
        with pytest.raises(ValueError):
            next(tts.inference_long_stream(TEXT, pitch_shift=bad, **voice))
        with pytest.raises(ValueError):
            next(tts.serve(one, do_sample=False, pitch_shift=bad))
    with pytest.raises(ValueError, match="request 0"):
        tts.inference_batch([dict(one[0], pitch_shift=30)], do_sample=False)
    with pytest.raises(ValueError, match="request 0"):
        next(tts.serve([dict(one[0], pitch_shift=30)], do_sample=False))
