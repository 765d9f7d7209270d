"""``loudness`` through SparkTTS on the synthetic model directory (max_batch=2, max_positions=1024, max_frames=256; prompt_tokens
given; the ids kept on semantic tokens and eos): every sentence of ``inference_long`` reaches the target on its own trimmed
piece, the stream's pieces stay those of ``inference_long``, and a request of a batch carries its own target.

Yardstick: the same call with ``loudness=None`` (waveform A) -- B's pieces are fl32(fl64(A's piece) * gain) bit for bit with the
gain the device reported, and the reported loudness is tests/loud_ref.py's on A's piece within the derived tolerance."""
import math

import numpy as np
import pytest
import torch

import loud_ref as R
import trim_ref as tr

pytestmark = pytest.mark.gpu

TEXT = ("The first sentence of the paragraph is this one. Then a second one follows it, a little longer than the first! "
        "Is the third one really a question? And the fourth sentence closes the paragraph.")
W, S = 1600, 160
PAUSE = 0.25
GAP = 4000
BUDGET = 40
TARGET = -23.0
SR = 16000


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import audio, longform, synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_loud")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    voice = dict(prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                 allowed_token_ids=sorted(tts._map.sem) + list(tts._eos), min_new_tokens=14)
    sentences = longform.split_text(TEXT, 300, 20)
    assert len(sentences) == 4
    kw = dict(voice, do_sample=False, max_new_tokens=BUDGET, pause=PAUSE, fade=0.0)
    # a trim threshold that no window sits on, from the untrimmed rows (the synthetic vocoder's level is arbitrary)
    raw, info0 = tts.inference_long(TEXT, trim=False, return_info=True, **kw)
    rows = [raw[o: o + b - a] for o, (a, b) in zip(info0["offsets"], info0["bounds"])]
    e = np.sort(np.concatenate([tr.energies(r, W, S) for r in rows]))
    lo, hi = int(0.75 * e.size), int(0.85 * e.size)
    j = lo + int(np.argmax(e[lo + 1: hi + 1] / e[lo: hi]))
    thr = float(np.sqrt(np.sqrt(e[j] * e[j + 1]) / W))
    kw["trim_threshold"] = thr
    # the two runs every test compares, once
    A, info_a = tts.inference_long(TEXT, return_info=True, **kw)
    B, info_b = tts.inference_long(TEXT, return_info=True, loudness=TARGET, **kw)
    coef, block = audio.k_weighting(SR), audio.loudness_block(SR)
    return dict(tts=tts, voice=voice, sentences=sentences, kw=kw, A=A, B=B, info_a=info_a, info_b=info_b, coef=coef, block=block,
                ceiling=audio.PEAK_CEILING)


def test_every_sentence_reaches_the_target_on_its_own_piece(setup):
    s = setup
    ia, ib, A, B = s["info_a"], s["info_b"], s["A"], s["B"]
    for key in ("sentences", "token_ids", "bounds", "offsets", "silent", "truncated"):
        assert ia[key] == ib[key], key
    assert "loudness" not in ia and "gain" not in ia and "limited" not in ia
    assert A.size == B.size and B.dtype == np.float32
    covered = np.zeros(A.size, dtype=bool)
    spoken = 0
    for k, ((a, b), off) in enumerate(zip(ia["bounds"], ia["offsets"])):
        piece = A[off: off + b - a]
        covered[off: off + b - a] = True
        if b == a:
            assert ib["loudness"][k] == -math.inf and ib["gain"][k] == 1.0 and ib["limited"][k] is None
            continue
        spoken += 1
        want = R.loudness(piece, s["coef"], s["block"], np.longdouble)
        g, limit = R.gain(ib["loudness"][k], R.peak(piece), TARGET, 20.0, s["ceiling"])
        print(f"sentence {k}: {b - a} samples, loudness {ib['loudness'][k]!r} (ref {float(want)!r}), gain {ib['gain'][k]!r}, "
              f"limited {ib['limited'][k]}, peak {R.peak(piece)!r}")
        if want == -math.inf:
            assert ib["loudness"][k] == -math.inf and ib["gain"][k] == 1.0 and ib["limited"][k] is None
        else:
            assert abs(np.longdouble(ib["loudness"][k]) - want) <= R.TOL_LU
            assert abs(ib["gain"][k] / float(g) - 1) <= R.TOL_GAIN and ib["limited"][k] == (None, "max_gain", "ceiling")[limit]
        assert np.array_equal(_bits(B[off: off + b - a]), _bits(R.apply_gain(piece, ib["gain"][k])))
    assert spoken >= 2
    assert not B[~covered].any() and (~covered).sum() == (spoken - 1) * GAP      # the pauses are zeros
    assert not np.array_equal(A, B)


@pytest.mark.parametrize("sr", [None, 24000])
def test_stream_pieces_concatenate_to_inference_long(setup, sr):
    s = setup
    tts, kw = s["tts"], dict(s["kw"], loudness=TARGET, output_sample_rate=sr)
    whole = s["B"] if sr is None else tts.inference_long(TEXT, **kw)
    pieces = list(tts.inference_long_stream(TEXT, **kw))
    assert len(pieces) >= 2 and np.array_equal(_bits(np.concatenate(pieces)), _bits(whole))
    if sr is not None:
        assert whole.size == -((-s["B"].size * 3) // 2)


def test_a_request_of_a_batch_carries_its_own_target(setup):
    s = setup
    tts, voice, (t0, t1) = s["tts"], s["voice"], s["sentences"][:2]
    kw = dict(do_sample=False, max_new_tokens=BUDGET)
    p0, p1 = tts.inference_batch([dict(voice, text=t0), dict(voice, text=t1)], **kw)
    assert tts.last_loudness == [None, None]
    q0, q1 = tts.inference_batch([dict(voice, text=t0, loudness=-16.0), dict(voice, text=t1)], **kw)
    got = tts.last_loudness
    assert got[1] is None and np.array_equal(_bits(q1), _bits(p1))
    want = R.loudness(p0, s["coef"], s["block"], np.longdouble)
    g, limit = R.gain(got[0]["loudness"], R.peak(p0), -16.0, 20.0, s["ceiling"])
    print(f"request 0: loudness {got[0]['loudness']!r} (ref {float(want)!r}) gain {got[0]['gain']!r} limited {got[0]['limited']}")
    assert abs(np.longdouble(got[0]["loudness"]) - want) <= R.TOL_LU
    assert abs(got[0]["gain"] / float(g) - 1) <= R.TOL_GAIN and got[0]["limited"] == (None, "max_gain", "ceiling")[limit]
    assert np.array_equal(_bits(q0), _bits(R.apply_gain(p0, got[0]["gain"])))
    # the call's own target reaches every request without a key, and serve gives the same waveforms
    r0, r1 = tts.inference_batch([dict(voice, text=t0, loudness=-16.0), dict(voice, text=t1)], loudness=-30.0, max_gain_db=6.0, **kw)
    both = tts.last_loudness
    assert both[0]["loudness"] == got[0]["loudness"] and both[1]["loudness"] > -math.inf
    for r, p, d, t in ((r0, p0, both[0], -16.0), (r1, p1, both[1], -30.0)):
        g, limit = R.gain(d["loudness"], R.peak(p), t, 6.0, s["ceiling"])
        assert abs(d["gain"] / float(g) - 1) <= R.TOL_GAIN and d["limited"] == (None, "max_gain", "ceiling")[limit]
        assert np.array_equal(_bits(r), _bits(R.apply_gain(p, d["gain"])))
    plain = dict(tts.serve([dict(voice, text=t0), dict(voice, text=t1)], **kw))
    assert tts.last_loudness == {}
    served = dict(tts.serve([dict(voice, text=t0, loudness=-16.0), dict(voice, text=t1)], loudness=-30.0, max_gain_db=6.0, **kw))
    assert sorted(tts.last_loudness) == [0, 1]
    for i in (0, 1):
        assert np.array_equal(_bits(served[i]), _bits(R.apply_gain(plain[i], tts.last_loudness[i]["gain"])))


def test_bad_parameters_raise_before_any_device_work(setup):
    s = setup
    tts, voice, kw = s["tts"], s["voice"], s["kw"]
    one = [dict(voice, text=s["sentences"][0])]
    for bad in (dict(loudness=math.nan), dict(loudness=math.inf), dict(loudness="-23"), dict(loudness=True),
                dict(loudness=-23.0, peak_ceiling=0.0), dict(loudness=-23.0, peak_ceiling=math.nan),
                dict(loudness=-23.0, max_gain_db=-1.0), dict(max_gain_db=math.inf)):
        with pytest.raises(ValueError):
            tts.inference_long(TEXT, **dict(kw, **bad))
        with pytest.raises(ValueError):
            next(tts.inference_long_stream(TEXT, **dict(kw, **bad)))
        with pytest.raises(ValueError):
            tts.inference_batch(one, do_sample=False, **bad)
        with pytest.raises(ValueError):
            tts.inference(s["sentences"][0], do_sample=False, **dict(voice, **bad))
        with pytest.raises(ValueError):
            next(tts.serve(one, do_sample=False, **bad))
    with pytest.raises(ValueError, match="request 0"):
        tts.inference_batch([dict(one[0], loudness=math.nan)], do_sample=False)
    with pytest.raises(ValueError, match="request 0"):
        next(tts.serve([dict(one[0], loudness="loud")], do_sample=False))
    for call in (tts.inference_stream, tts.serve_stream):   # the chunked streams do not take it
        with pytest.raises(TypeError):
            next(call(one if call is tts.serve_stream else TEXT, loudness=-23.0))
