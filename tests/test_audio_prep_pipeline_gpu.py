"""The device audio path through the Python surface, on the tiny synthetic configs: BiCodecEncoder.tokenize_rows_device,
SparkTTS.inference_batch(prompt_audio=...) and output_sample_rate.

No id equality between prompt_audio="host" and "device" is claimed or tested: the device rows differ from the host's by fp32
rounding.  What is tested is the plumbing -- the ids of the device path are those of tokenize_arrays on the device-prepared
rows -- and the output resampler against the float64 formula of tests/resample_ref.py."""
import wave

import numpy as np
import pytest
import torch

import resample_ref as rr
from sparkmi import audio, config as C, config_tok as T, weights as W

pytestmark = pytest.mark.gpu


def _tone(i, f0, secs, sr):
    t = np.arange(int(sr * secs)) / float(sr)
    x = 0.3 * np.sin(2 * np.pi * f0 * t) * (0.5 + 0.5 * np.sin(2 * np.pi * 2.0 * t)) + 0.01 * np.random.default_rng(i).standard_normal(len(t))
    return x.astype(np.float32)


def _write_wav(path, x, sr):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767.0).astype("<i2").tobytes())


def test_tokenize_rows_device_gives_the_ids_of_its_own_rows():
    from sparkmi.encoder import BiCodecEncoder
    wcfg, tcfg, vcfg = T.tiny_wav2vec2(), T.tiny_tok(), C.tiny_bicodec()
    wf = W.fold_pos_conv_weight_norm(W.wav2vec2_state(wcfg))
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    enc = BiCodecEncoder(wcfg, tcfg, wf, tsd, "cuda:0", max_seconds=3.0, ref_seconds=1.0)
    rates = [48000, 44100, 16000]
    raws = [_tone(0, 150.0, 1.2, 48000), _tone(1, 210.0, 0.4, 44100), _tone(2, 180.0, 0.7, 16000)]
    ref_len = 16000 // vcfg.hop * vcfg.hop
    got = enc.tokenize_rows_device(raws, rates, ref_len)
    plan, wav, ref, gain = enc.prepare_rows_device(raws, rates, ref_len)
    assert plan["n_samples"] == sorted(audio.out_len(r.size, *audio.ratio(sr, 16000)) for r, sr in zip(raws, rates))
    wav, ref, gain = wav.cpu().numpy(), ref.cpu().numpy(), gain.cpu().numpy()
    assert ((gain > 0.1) & (gain < 10)).all()
    for i in range(3):
        j = plan["inverse"][i]
        n = plan["n_samples"][j]
        assert not wav[j, n:].any() and ref.shape[1] == ref_len
        g, s = enc.tokenize_arrays(wav[j, :n], ref[j])
        assert torch.equal(g, got[i][0]) and torch.equal(s, got[i][1]), i
        assert np.array_equal(ref[j], rr.ref_clip(wav[j, :n], ref_len))
    # the 16 kHz row took the copy path: its samples are the raw row times the gain, rounded once
    j = plan["inverse"][2]
    assert np.array_equal(wav[j, : raws[2].size], (raws[2].astype(np.float64) * gain[j]).astype(np.float32))
    enc.close()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_audio")
    synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=1024, max_frames=256)
    # the synthetic LLM's greedy tokens are arbitrary: keep every request on semantic tokens, so that each has audio to vocode
    sem0 = tts.tokenizer.convert_tokens_to_ids("<|bicodec_semantic_0|>")
    allowed = list(range(sem0, sem0 + tts.audio_tokenizer.model.cfg.codebook_size))
    paths = {}
    for i, (f0, secs, sr) in enumerate(((150.0, 1.3, 48000), (210.0, 0.9, 44100), (150.0, 1.3, 16000), (210.0, 0.9, 16000))):
        p = d / f"prompt{i}_{sr}.wav"
        _write_wav(p, _tone(i, f0, secs, sr), sr)
        paths[i] = str(p)
    return tts, allowed, paths


def test_inference_batch_with_device_prepared_prompts(model):
    tts, allowed, paths = model
    kw = dict(do_sample=False, max_new_tokens=24)
    reqs = [dict(text="First speaker.", prompt_speech_path=paths[0], prompt_text="one", allowed_token_ids=allowed),
            dict(text="Second speaker, a little longer.", prompt_speech_path=paths[1], prompt_text=None, allowed_token_ids=allowed)]
    dev = tts.inference_batch(reqs, prompt_encode="rows", prompt_audio="device", **kw)
    again = tts.inference_batch(reqs, prompt_encode="rows", prompt_audio="device", **kw)
    hop = tts.audio_tokenizer.model.hop
    for a, b in zip(dev, again):
        assert a.dtype == np.float32 and a.size == 24 * hop and np.isfinite(a).all() and np.array_equal(a, b)
    one = tts.inference_batch(reqs[:1], prompt_encode="rows", prompt_audio="device", **kw)      # a single prompt takes the device path too
    assert np.array_equal(one[0], dev[0])
    # the ids behind it are tokenize_rows(..., "device")'s, which are those of the encoder's device path
    toks = tts.audio_tokenizer.tokenize_rows([paths[0], paths[1]], prompt_audio="device")
    assert toks[0][1].shape[1] > toks[1][1].shape[1] > 0
    # the host path is untouched: naming it changes nothing
    for pe in ("rows", "streams"):
        a = tts.inference_batch(reqs, prompt_encode=pe, prompt_audio="host", **kw)
        b = tts.inference_batch(reqs, prompt_encode=pe, **kw)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    with pytest.raises(ValueError, match="prompt_encode='rows'"):
        tts.inference_batch(reqs, prompt_audio="device", **kw)
    with pytest.raises(ValueError, match="prompt_audio"):
        tts.inference_batch(reqs, prompt_encode="rows", prompt_audio="gpu", **kw)
    with pytest.raises(ValueError, match="prompt_audio"):
        tts.audio_tokenizer.tokenize_rows([paths[0]], prompt_audio="gpu")


def test_output_sample_rate(model):
    tts, allowed, paths = model
    kw = dict(do_sample=False, prompt_encode="rows")
    # the second request ends after 9 semantic tokens (its eos is pushed as soon as min_new_tokens lets it): rows of two lengths
    reqs = [dict(text="First speaker.", prompt_speech_path=paths[2], prompt_text="one", allowed_token_ids=allowed),
            dict(text="Second speaker, a little longer.", prompt_speech_path=paths[3], prompt_text=None,
                 allowed_token_ids=sorted(set(allowed) | set(tts._eos)), eos_bias=1e4, min_new_tokens=9)]
    base = tts.inference_batch(reqs, max_new_tokens=17, **kw)
    hop = tts.audio_tokenizer.model.hop
    assert [b.size for b in base] == [17 * hop, 9 * hop]
    for same in (None, 16000):
        for x, y in zip(base, tts.inference_batch(reqs, max_new_tokens=17, output_sample_rate=same, **kw)):
            assert x.shape == y.shape and np.array_equal(x, y)
    for sr in (24000, 44100):
        up, down = audio.ratio(16000, sr)
        taps = audio.resample_taps(up, down)
        out = tts.inference_batch(reqs, max_new_tokens=17, output_sample_rate=sr, **kw)
        for x, y in zip(base, out):
            want, absum, N = rr.direct(x, up, down, taps)
            assert y.dtype == np.float32 and y.size == audio.out_len(x.size, up, down) == want.size
            err, bound = np.abs(y.astype(np.float64) - want), rr.bound(absum, N)
            print(f"{sr} Hz, {x.size} samples: worst error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
            assert (err <= bound).all()
    one = tts.inference("First speaker.", prompt_speech_path=paths[2], prompt_text="one", allowed_token_ids=allowed, do_sample=False,
                        max_new_tokens=17, output_sample_rate=24000)
    assert one.size == audio.out_len(17 * tts.audio_tokenizer.model.hop, 3, 2)
    with pytest.raises(ValueError, match="output_sample_rate"):
        tts.inference_batch(reqs, max_new_tokens=17, output_sample_rate=0, **kw)
    # streamed chunks keep the model's rate: the option is refused there
    with pytest.raises(ValueError, match="output_sample_rate"):
        next(tts.inference_stream("hello", gender="male", pitch="low", speed="high", do_sample=False, max_new_tokens=8, output_sample_rate=24000))
    with pytest.raises(ValueError, match="output_sample_rate"):
        next(tts.serve_stream([dict(text="hello", gender="male", pitch="low", speed="high")], do_sample=False, max_new_tokens=8,
                              output_sample_rate=24000))
