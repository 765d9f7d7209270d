"""SparkTTS with num_return_sequences on a synthetic model directory (voice-clone mode, prompt tokens given): n takes of one
request equal inference_batch of the request n times, a request's own seed gives take j the seed + j, each take has its own
log-probability info, and serve gives what inference_batch gives."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_fork")
    _, vcfg = synthetic.make_model_dir(d)
    rng = np.random.Generator(np.random.PCG64(21))
    reqs = []
    for i in range(3):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"take number {i} " * (i + 1), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long))))
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=4, max_positions=512, max_frames=256)
    return tts, reqs


KW = dict(temperature=0.8, top_k=50, top_p=0.95, max_new_tokens=40)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_takes_equal_the_request_repeated(setup):
    tts, reqs = setup
    r = reqs[0]
    takes = tts.inference(r["text"], prompt_tokens=r["prompt_tokens"], seed=7, num_return_sequences=3, **KW)
    assert isinstance(takes, list) and len(takes) == 3 and all(isinstance(w, np.ndarray) for w in takes)
    assert _same(takes, tts.inference_batch([r] * 3, seed=7, **KW))
    assert not all(np.array_equal(takes[0], w) for w in takes[1:])   # the takes differ
    one = tts.inference(r["text"], prompt_tokens=r["prompt_tokens"], seed=7, num_return_sequences=1, **KW)
    assert isinstance(one, np.ndarray)
    assert np.array_equal(one, tts.inference(r["text"], prompt_tokens=r["prompt_tokens"], seed=7, **KW))


def test_a_seeded_request_gives_take_j_seed_plus_j(setup):
    tts, reqs = setup
    r = dict(reqs[1], seed=40, temperature=0.7)
    takes = tts.inference_batch([dict(r, num_return_sequences=3)], seed=1, **KW)[0]
    assert isinstance(takes, list) and len(takes) == 3
    for j in range(3):
        alone = tts.inference_batch([dict(r, seed=40 + j)], seed=1, **KW)[0]
        assert np.array_equal(takes[j], alone), f"take {j}"


def test_each_take_has_its_own_info(setup):
    tts, reqs = setup
    r = reqs[0]
    takes = tts.inference(r["text"], prompt_tokens=r["prompt_tokens"], seed=7, num_return_sequences=3, return_log_probs=True, **KW)
    assert len(takes) == 3
    plain = tts.inference(r["text"], prompt_tokens=r["prompt_tokens"], seed=7, num_return_sequences=3, **KW)
    for (w, info), p in zip(takes, plain):
        assert np.array_equal(w, p)
        lp = info["output_log_probs"]
        assert lp.dtype == np.float32 and lp.shape == (len(info["token_ids"]),) and np.isfinite(lp).all()
        assert info["cum_log_prob"] == float(np.sum(lp, dtype=np.float64))
    assert len({tuple(info["token_ids"]) for _, info in takes}) > 1


def test_serve_mixes_forked_and_plain_requests(setup):
    tts, reqs = setup
    mixed = [dict(reqs[0], num_return_sequences=2), dict(reqs[1]), dict(reqs[2], num_return_sequences=3, seed=5),
             dict(reqs[1], do_sample=False)]
    batch = tts.inference_batch(mixed[:2], seed=11, **KW) + tts.inference_batch(mixed[2:], seed=11, **KW)
    served = dict(tts.serve(iter(mixed), seed=11, **KW))
    assert sorted(served) == [0, 1, 2, 3]
    for i, want in enumerate(batch):
        got = served[i]
        if "num_return_sequences" in mixed[i]:
            assert isinstance(got, list) and _same(got, want), f"request {i}"
        else:
            assert np.array_equal(got, want), f"request {i}"
