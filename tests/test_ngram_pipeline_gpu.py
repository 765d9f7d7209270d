"""no_repeat_ngram_size through SparkTTS on a synthetic model directory: the inference argument and the request key of
inference_batch, serve and serve_stream reach the LLM (no 4-gram is generated twice), malformed values raise before anything
reaches the device, and a request without the key gives the bytes it gives without the feature."""
import numpy as np
import pytest
import torch

from ngram_ref import repeats

pytestmark = pytest.mark.gpu


def test_the_key_through_the_pipeline(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_ngram")
    lcfg, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(13))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    # (an n-gram request needs max_positions selectable ids: the 256 semantic ids of the synthetic tokenizer bound max_positions)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=192, max_frames=256)
    hop, eos = tts.audio_tokenizer.model.hop, list(tts._eos)
    sem = sorted(i for name, i in tts.tokenizer.get_added_vocab().items() if "bicodec_semantic" in name)
    # a strong bias towards two ids makes the plain run loop (16 possible 4-grams); only semantic tokens can be generated, eos never
    loop = [((sem[3],), 30.0), ((sem[7],), 30.0)]
    req = dict(text="utterance number one " * 2, prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
               allowed_token_ids=sem + eos, eos_bias=float("-inf"), sequence_bias=loop)
    N = 48
    kw = dict(do_sample=False, max_new_tokens=N)

    def tokens(r):
        wav, info = tts.inference_batch([dict(r, return_log_probs=True)], **kw)[0]
        return list(info["token_ids"]), wav

    # the prompt's own text repeats: what counts is a repeat that ends in a generated id
    pids = tts.tokenizer([tts.process_prompt(req["text"], None, None, req["prompt_tokens"])[0]], return_tensors="pt").input_ids[0].tolist()
    base, wav0 = tokens(req)
    assert len(base) == N and repeats(pids + base, 4, len(pids)), "the request without the key repeats a 4-gram"
    got, wav4 = tokens(dict(req, no_repeat_ngram_size=4))
    assert len(got) == N and len(wav4) == hop * N and not repeats(pids + got, 4, len(pids)) and got != base
    assert tokens(dict(req, no_repeat_ngram_size=0))[0] == base
    # the inference argument
    wav, info = tts.inference(req["text"], prompt_tokens=req["prompt_tokens"], allowed_token_ids=sem, no_repeat_ngram_size=4,
                              return_log_probs=True, **kw)
    assert len(info["token_ids"]) == N and not repeats(pids + list(info["token_ids"]), 4, len(pids))
    # inference_batch, serve and serve_stream take it per request, and agree
    reqs = [dict(req, no_repeat_ngram_size=4), req, dict(req, no_repeat_ngram_size=2)]
    batch = tts.inference_batch(reqs, return_log_probs=True, **kw)
    ids = [list(info["token_ids"]) for _, info in batch]
    assert ids[0] == got and ids[1] == base and not repeats(pids + ids[2], 2, len(pids))
    served = {i: (w, info) for i, w, info in tts.serve(reqs, return_log_probs=True, **kw)}
    for i in range(3):
        assert list(served[i][1]["token_ids"]) == ids[i]
        assert np.allclose(served[i][0], batch[i][0], atol=1e-4)
    admitted = []
    inner = tts.model.admit
    tts.model.admit = lambda *a, **kws: admitted.append(inner(*a, **kws)) or admitted[-1]
    chunks = list(tts.serve_stream(reqs, decode_stride=4, **kw))
    tts.model.admit = inner
    assert {i for i, _, last in chunks if last} == {0, 1, 2}
    slots = [s for call in admitted for s in call]
    assert [t for t, _ in tts.model.slots_tokens(slots, N)] == ids
    # malformed values raise before the request reaches the device
    for bad in (True, -1, 65, 2.0):
        for call in (lambda r: tts.inference_batch([r], **kw), lambda r: list(tts.serve([r], **kw)),
                     lambda r: list(tts.serve_stream([r], **kw))):
            with pytest.raises(ValueError):
                call(dict(req, no_repeat_ngram_size=bad))
    # and the request without the key gives the same bytes afterwards
    again, wav1 = tokens(req)
    assert again == base and np.array_equal(wav0, wav1)
