"""``limiter`` through SparkTTS on the synthetic model directory (max_batch=2, max_positions=1024, max_frames=256; prompt_tokens
given; the ids kept on semantic tokens and eos).

Yardstick: the same call with ``loudness=None`` and ``limiter=None`` (waveform p) -- the limited row is tests/limit_ref.py applied
to p with the gain the device reported, bit for bit.  The loudness targets are chosen from p so that the gain drives its peak to
twice the ceiling: the limiter has work to do whatever the synthetic vocoder's level is."""
import math

import numpy as np
import pytest
import torch

import limit_ref as L
import loud_ref as R

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence of the paragraph is this one. Then a second one follows it, a little longer than the first! "
        "Is the third one really a question? And the fourth sentence closes the paragraph.")
BUDGET = 40
SR = 16000
MAX_GAIN = 120.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _hot_target(p, coef, block, ceiling, factor=2.0):
    """the LUFS target whose gain brings p's sample peak to ``factor`` times the ceiling"""
    return float(R.loudness(p, coef, block, np.longdouble)) + 20.0 * math.log10(factor * ceiling / float(R.peak(p)))


def _limited(p, g, mode, ceiling=L.CEILING):
    from sparkmi import audio
    return L.limit(p, g, ceiling, L.taps() if mode == "true" else None, L.A0, L.R0, audio.limiter_window(L.A0, L.R0))


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import audio, longform, synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_limit")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    voice = dict(prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                 allowed_token_ids=sorted(tts._map.sem) + list(tts._eos), min_new_tokens=14)
    sentences = longform.split_text(TEXT, 300, 20)
    kw = dict(do_sample=False, max_new_tokens=BUDGET)
    reqs = [dict(voice, text=sentences[0]), dict(voice, text=sentences[1])]
    p0, p1 = tts.inference_batch(reqs, **kw)
    assert tts.last_loudness == [None, None] and tts.last_limiter == [None, None]
    coef, block = audio.k_weighting(SR), audio.loudness_block(SR)
    assert audio.limiter_reach(SR) == (L.A0, L.R0)
    targets = [_hot_target(p, coef, block, L.CEILING) for p in (p0, p1)]
    return dict(tts=tts, voice=voice, sentences=sentences, kw=kw, reqs=reqs, p=(p0, p1), targets=targets, coef=coef, block=block)


def _check_row(name, out, p, loud, lim, mode, target):
    """out is limit_ref of p with the reported gain; the gain is the loudness stage's, unbounded by the ceiling"""
    g = loud["gain"]
    want = _limited(p, g, mode)
    print(f"{name}: gain {g!r} limited {loud['limited']} limiter {lim} (ref stats {want['stats'].tolist()})")
    assert loud["limited"] in (None, "max_gain")
    assert abs(g / float(10 ** ((target - np.longdouble(loud["loudness"])) / 20)) - 1) <= R.TOL_GAIN
    assert np.array_equal(_bits(out), _bits(want["out"])), name
    assert (np.abs(out.astype(np.float64)) <= L.CEILING).all()
    assert lim["true_peak"] == want["stats"][0] and lim["limited_samples"] == int(want["stats"][3]) and lim["limited_samples"] > 0
    assert lim["reduction_db"] == -20.0 * math.log10(want["stats"][2]) and lim["reduction_db"] > 3.0
    assert lim["true_peak"] > 1.9 * L.CEILING


def test_batch_with_loudness_and_limiter_is_the_reference_on_the_plain_waveform(setup):
    s = setup
    tts, reqs = s["tts"], s["reqs"]
    both = [dict(r, loudness=t) for r, t in zip(reqs, s["targets"])]
    q = tts.inference_batch(both, limiter="true", max_gain_db=MAX_GAIN, **s["kw"])
    for b in (0, 1):
        _check_row(f"request {b}", q[b], s["p"][b], tts.last_loudness[b], tts.last_limiter[b], "true", s["targets"][b])
    free = [d["gain"] for d in tts.last_loudness]
    # without the limiter the ceiling binds in the loudness stage and holds the whole row down, at half the gain: today's bits
    r = tts.inference_batch(both, max_gain_db=MAX_GAIN, **s["kw"])
    assert tts.last_limiter == [None, None]
    for b in (0, 1):
        d = tts.last_loudness[b]
        assert d["limited"] == "ceiling" and abs(d["gain"] / (0.5 * free[b]) - 1) < 1e-6
        assert np.array_equal(_bits(r[b]), _bits(R.apply_gain(s["p"][b], d["gain"])))
    # the limiter alone: g = 1 and the vocoder's output bounded
    u = tts.inference_batch(reqs, limiter="true", peak_ceiling=0.5 * float(R.peak(s["p"][0])), **s["kw"])
    assert tts.last_loudness == [None, None]
    c = 0.5 * float(R.peak(s["p"][0]))
    from sparkmi import audio
    want = L.limit(s["p"][0], 1.0, c, L.taps(), L.A0, L.R0, audio.limiter_window(L.A0, L.R0))
    assert np.array_equal(_bits(u[0]), _bits(want["out"])) and np.abs(u[0]).max() <= c
    assert tts.last_limiter[0]["limited_samples"] == int(want["stats"][3]) > 0
    # the single call is the batch of one
    one = tts.inference(s["sentences"][0], loudness=s["targets"][0], limiter="true", max_gain_db=MAX_GAIN, **dict(s["voice"], **s["kw"]))
    assert np.array_equal(_bits(one), _bits(q[0]))


def test_a_requests_own_limiter_key_overrides_the_calls(setup):
    s = setup
    tts, reqs, (t0, t1) = s["tts"], s["reqs"], s["targets"]
    q = tts.inference_batch([dict(reqs[0], loudness=t0, limiter="sample"), dict(reqs[1], loudness=t1, limiter=None)], limiter="true",
                            max_gain_db=MAX_GAIN, **s["kw"])
    assert tts.last_limiter[1] is None and tts.last_loudness[1]["limited"] == "ceiling"
    assert np.array_equal(_bits(q[1]), _bits(R.apply_gain(s["p"][1], tts.last_loudness[1]["gain"])))
    _check_row("request 0, sample mode", q[0], s["p"][0], tts.last_loudness[0], tts.last_limiter[0], "sample", t0)
    # the other way round, and through serve
    q = tts.inference_batch([dict(reqs[0], loudness=t0), dict(reqs[1], loudness=t1, limiter="true")], max_gain_db=MAX_GAIN, **s["kw"])
    assert tts.last_limiter[0] is None and tts.last_loudness[0]["limited"] == "ceiling"
    _check_row("request 1", q[1], s["p"][1], tts.last_loudness[1], tts.last_limiter[1], "true", t1)
    served = dict(tts.serve([dict(reqs[0], loudness=t0), dict(reqs[1], loudness=t1, limiter="true")], max_gain_db=MAX_GAIN, **s["kw"]))
    assert sorted(tts.last_limiter) == [1] and sorted(tts.last_loudness) == [0, 1]
    assert np.array_equal(_bits(served[0]), _bits(q[0])) and np.array_equal(_bits(served[1]), _bits(q[1]))
    served = dict(tts.serve(reqs, limiter="sample", peak_ceiling=0.5 * float(R.peak(s["p"][1])), **s["kw"]))
    assert sorted(tts.last_limiter) == [0, 1] and tts.last_loudness == {}
    assert np.abs(served[1]).max() <= 0.5 * float(R.peak(s["p"][1])) and tts.last_limiter[1]["limited_samples"] > 0


def test_inference_long_limits_every_piece_on_its_own(setup):
    s = setup
    tts = s["tts"]
    kw = dict(s["voice"], do_sample=False, max_new_tokens=BUDGET, pause=0.25, fade=0.0, trim=False)
    A, ia = tts.inference_long(TEXT, return_info=True, **kw)
    assert "limiter" not in ia
    pieces = [A[o: o + b - a] for o, (a, b) in zip(ia["offsets"], ia["bounds"])]
    target = min(_hot_target(p, s["coef"], s["block"], L.CEILING) for p in pieces if p.size)
    B, ib = tts.inference_long(TEXT, return_info=True, loudness=target, limiter="true", max_gain_db=MAX_GAIN, **kw)
    assert ib["bounds"] == ia["bounds"] and ib["offsets"] == ia["offsets"] and len(ib["limiter"]) == len(pieces) == 4
    assert (np.abs(B.astype(np.float64)) <= L.CEILING).all()
    for k, (p, off) in enumerate(zip(pieces, ia["offsets"])):
        want = _limited(p, ib["gain"][k], "true")
        print(f"sentence {k}: gain {ib['gain'][k]!r} limited {ib['limited'][k]} limiter {ib['limiter'][k]}")
        assert ib["limited"][k] in (None, "max_gain")
        assert np.array_equal(_bits(B[off: off + p.size]), _bits(want["out"])), k
        assert ib["limiter"][k]["limited_samples"] == int(want["stats"][3]) and ib["limiter"][k]["true_peak"] == want["stats"][0]
    assert sum(d["limited_samples"] > 0 for d in ib["limiter"]) >= 1
    got = list(tts.inference_long_stream(TEXT, loudness=target, limiter="true", max_gain_db=MAX_GAIN, **kw))
    assert np.array_equal(_bits(np.concatenate(got)), _bits(B))
    # the limiter alone
    C, ic = tts.inference_long(TEXT, return_info=True, limiter="sample", peak_ceiling=0.25 * float(np.abs(A).max()), **kw)
    assert np.abs(C).max() <= 0.25 * float(np.abs(A).max()) and "loudness" not in ic and len(ic["limiter"]) == 4


def test_streams_and_bad_parameters_are_refused_before_any_device_work(setup):
    s = setup
    tts, voice = s["tts"], s["voice"]
    one = [dict(voice, text=s["sentences"][0])]
    for joined in (False, True):
        with pytest.raises(ValueError, match="limiter"):
            next(tts.inference_stream(s["sentences"][0], limiter="true", joined=joined))
        with pytest.raises(ValueError, match="limiter"):
            next(tts.serve_stream(one, limiter="sample", joined=joined))
        with pytest.raises(ValueError, match="request 0"):
            next(tts.serve_stream([dict(one[0], limiter="true")], joined=joined))
    for bad in (dict(limiter="peak"), dict(limiter=True), dict(limiter=1), dict(limiter="true", limiter_lookahead_ms=-1.0),
                dict(limiter="true", limiter_release_ms=200.0), dict(limiter="true", limiter_lookahead_ms=math.nan),
                dict(limiter="true", peak_ceiling=0.0)):
        with pytest.raises(ValueError):
            tts.inference_batch(one, do_sample=False, **bad)
        with pytest.raises(ValueError):
            tts.inference(s["sentences"][0], do_sample=False, **dict(voice, **bad))
        with pytest.raises(ValueError):
            next(tts.serve(one, do_sample=False, **bad))
        with pytest.raises(ValueError):
            tts.inference_long(TEXT, do_sample=False, **dict(voice, **bad))
        with pytest.raises(ValueError):
            next(tts.inference_long_stream(TEXT, do_sample=False, **dict(voice, **bad)))
    with pytest.raises(ValueError, match="request 0"):
        tts.inference_batch([dict(one[0], limiter="loud")], do_sample=False)
    with pytest.raises(ValueError, match="request 0"):
        next(tts.serve([dict(one[0], limiter="loud")], do_sample=False))
