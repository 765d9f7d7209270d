"""sequence_bias / bad_words_ids / stop_sequences / eos_bias through SparkTTS on a synthetic model directory: inference_batch,
serve and serve_stream take the keys per request, eos_bias steers where an utterance ends, two requests of one serve_stream
session stop on different ids, and malformed keys raise before anything reaches the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_sequence_keys_through_the_pipeline(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_seq")
    lcfg, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(13))
    glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    hop, eos = tts.audio_tokenizer.model.hop, list(tts._eos)
    assert eos
    # only semantic tokens and eos can be generated: the waveform's length counts the tokens before the end
    sem = sorted(i for name, i in tts.tokenizer.get_added_vocab().items() if "bicodec_semantic" in name)
    req = dict(text="utterance number one " * 2, prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
               allowed_token_ids=sem + eos)
    N = 40
    kw = dict(do_sample=False, max_new_tokens=N)

    def tokens(r):
        wav, info = tts.inference_batch([dict(r, return_log_probs=True)], **kw)[0]
        return list(info["token_ids"]), wav

    base, wav0 = tokens(req)
    base_sem = [t for t in base if t not in eos]
    assert len(wav0) == hop * len(base_sem)
    # eos_bias = -inf with a token budget runs to the budget
    toks, wav = tokens(dict(req, eos_bias=float("-inf")))
    assert len(toks) == N and not set(toks) & set(eos) and len(wav) == hop * N
    # a large positive eos_bias ends at the first token after min_new_tokens
    for n in (3, 9):
        toks, wav = tokens(dict(req, eos_bias=1e4, min_new_tokens=n))
        assert len(toks) == n + 1 and toks[n] in eos and not set(toks[:n]) & set(eos) and len(wav) == hop * n
    # a stop sequence ends the utterance like an eos id; a banned token leaves the output; a bias moves it
    long_ = tokens(dict(req, eos_bias=float("-inf")))[0]
    k = next(i for i in range(4, N) if long_[i] not in long_[:i])          # the first appearance of an id, at index k
    r_stop = dict(req, eos_bias=float("-inf"), stop_sequences=[[long_[k]], [long_[1], long_[0]]])
    toks, wav = tokens(r_stop)
    assert toks == long_[:k + 1] and len(wav) == hop * (k + 1)
    r_ban = dict(req, eos_bias=float("-inf"), bad_words_ids=[[long_[2]], [long_[4], long_[5]]])
    toks_ban, _ = tokens(r_ban)
    assert long_[2] not in toks_ban and toks_ban[:2] == long_[:2] and len(toks_ban) == N
    assert not any(toks_ban[i:i + 2] == [long_[4], long_[5]] for i in range(N - 1))
    r_bias = dict(req, eos_bias=float("-inf"), sequence_bias=[((sem[0],), 1e4)])
    assert tokens(r_bias)[0] == [sem[0]] * N
    # inference_batch, serve and serve_stream agree, request by request
    reqs = [r_stop, r_ban, dict(req, eos_bias=1e4, min_new_tokens=5)]
    batch = tts.inference_batch(reqs, return_log_probs=True, **kw)
    assert [len(w) // hop for w, _ in batch] == [k + 1, N, 5]
    assert [list(info["token_ids"]) for _, info in batch] == [long_[:k + 1], toks_ban, batch[2][1]["token_ids"]]
    served = {i: (w, info) for i, w, info in tts.serve(reqs, return_log_probs=True, **kw)}
    for i in range(3):   # the same tokens (the vocoder's batch shape differs between the two calls: waveforms agree to rounding)
        assert list(served[i][1]["token_ids"]) == list(batch[i][1]["token_ids"]) and len(served[i][0]) == len(batch[i][0])
        assert np.allclose(served[i][0], batch[i][0], atol=1e-4)
    # two requests of one serve_stream session stop on different ids
    k2 = next(i for i in range(k + 1, N) if long_[i] not in long_[:i])
    two = [dict(req, eos_bias=float("-inf"), stop_sequences=[[long_[k]]]), dict(req, eos_bias=float("-inf"), stop_sequences=[[long_[k2]]])]
    admitted = []
    inner = tts.model.admit
    tts.model.admit = lambda *a, **kws: admitted.append(inner(*a, **kws)) or admitted[-1]
    chunks = list(tts.serve_stream(two, decode_stride=4, **kw))
    tts.model.admit = inner
    assert {i for i, _, last in chunks if last} == {0, 1}
    slots = [s for call in admitted for s in call]
    got = tts.model.slots_tokens(slots, N)
    assert got[0] == (long_[:k + 1], True) and got[1] == (long_[:k2 + 1], True)
    # malformed keys raise before the request reaches the device
    for bad in (dict(stop_sequences=5), dict(eos_bias=float("nan")), dict(eos_bias=float("inf")), dict(bad_words_ids=[[-1]]),
                dict(sequence_bias=[((sem[0],), 1.0), ((sem[0],), 2.0)]), dict(stop_sequences=[list(range(9))]), dict(eos_bias="x")):
        for call in (lambda r: tts.inference_batch([r], **kw), lambda r: list(tts.serve([r], **kw)),
                     lambda r: list(tts.serve_stream([r], **kw))):
            with pytest.raises(ValueError):
                call(dict(req, **bad))
    # and requests without the keys are unchanged afterwards
    assert tokens(req)[0] == base
