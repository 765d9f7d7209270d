"""speech_tokens_only / allowed_token_ids through SparkTTS on a synthetic model directory: every generated id lies in the
added vocabulary plus eos, inference / inference_batch / serve agree, and calls without the keys are unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_speech_tokens_only_through_the_pipeline(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_allow")
    lcfg, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(13))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    req = dict(text="utterance number one " * 2, prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    kw = dict(do_sample=False, max_new_tokens=40)
    calls = []
    inner = tts.model.generate_ragged

    def spy(ids, budgets, eos=None, **k):
        out = inner(ids, budgets, eos, **k)
        calls.append((k.get("sampling"), out))
        return out

    tts.model.generate_ragged = spy
    plain = tts.inference_batch([req], **kw)[0]
    assert not calls, "a request without the keys keeps its route"
    speech = set(tts.speech_token_ids())
    assert speech == set(tts.tokenizer.get_added_vocab().values()) | set(tts._eos)
    wav = tts.inference_batch([dict(req, speech_tokens_only=True)], **kw)[0]
    assert calls, "a constrained request takes the admission path"
    toks = calls[-1][1][0]
    assert toks and all(t in speech for t in toks)
    wav1 = tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], speech_tokens_only=True, **kw)
    assert np.array_equal(wav, wav1)
    served = dict(tts.serve([dict(req, speech_tokens_only=True)], **kw))
    assert np.array_equal(served[0], wav)
    # an explicit set equal to the speech set gives the same waveform
    wav2 = tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], allowed_token_ids=sorted(speech), **kw)
    assert np.array_equal(wav2, wav)
    # and the unconstrained calls are unchanged afterwards
    assert np.array_equal(tts.inference_batch([req], **kw)[0], plain)
    assert np.array_equal(tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], **kw), plain)
