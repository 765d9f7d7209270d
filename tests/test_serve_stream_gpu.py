"""SparkTTS.serve_stream on a synthetic model directory: six clone-mode requests through three slots.  Yardstick per request: its
tokens from the admission path alone (``generate_ragged`` of that request; include/sparkmi.h promises they do not depend on what
else is live), cut into chunks by one ChunkScheduler, each chunk vocoded on its own with ``detokenize`` -- every streamed chunk
must equal that bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 16 kHz / hop 320 = 50 frames per second: audio_chunk_duration=0.5 makes the first chunk 25 frames, the overlap 5; every request
# generates at least 30 semantic tokens (its budget, or min_new_tokens where eos is allowed), so it has at least two chunks
STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    d = tmp_path_factory.mktemp("spark_synth_stream")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=3, max_positions=512, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(17))
    sem_ids = sorted(tts._map.sem)
    eos = list(tts._eos)
    reqs = []
    for i in range(6):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        r = dict(text=f"utterance number {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                 allowed_token_ids=list(sem_ids))
        if i in (1, 4):   # these two may stop on their own, not before 30 + i tokens
            r["allowed_token_ids"] = list(sem_ids) + eos
            r["min_new_tokens"] = 30 + i
        reqs.append(r)
    return tts, vcfg, reqs


def _yardstick(tts, r, do_sample, seed, budget=BUDGET):
    """[chunk waveforms] of one request: the admission path alone, one scheduler, every chunk vocoded on its own."""
    from sparkmi.pipeline import _request_sampling
    from sparkmi.streaming import ChunkScheduler
    prompt, g = tts.process_prompt(r["text"], None, None, r["prompt_tokens"])
    ids = tts.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
    tts.model.set_sampling(do_sample, 0.8, 50, 0.95, seed)
    toks = tts.model.generate_ragged([ids], [budget], tts._eos, sampling=[_request_sampling(r, tts.speech_token_ids)])[0]
    stops = [toks.index(e) for e in tts._eos if e in toks]
    if stops:
        toks = toks[: min(stops) + 1]
    assert all(t in tts._map.sem or t in tts._eos for t in toks), "every generated id is a semantic token (or eos) by construction"
    sem, _ = tts._parse(toks)
    sched = ChunkScheduler(STREAM["audio_chunk_duration"], 30.0, 8.0, STREAM["audio_chunk_overlap_duration"], 50)
    chunks = sched.push(sem) + sched.flush()
    voc, hop = tts.audio_tokenizer.model, tts.audio_tokenizer.model.hop
    g = torch.as_tensor(g).reshape(1, 1, -1)
    return [voc.detokenize(torch.tensor([c], dtype=torch.long), g).reshape(-1)[: len(c) * hop].cpu().numpy().copy() for c in chunks], len(toks)


def _streamed(tts, reqs, **kw):
    out = {i: [] for i in range(len(reqs))}
    order = []
    for i, w, last in tts.serve_stream(reqs, **dict(STREAM, max_new_tokens=BUDGET, **kw)):
        assert not out[i] or not out[i][-1][1], f"request {i}: a chunk after its last one"
        out[i].append((w, last))
        order.append(i)
    return out, order


def _compare(got, want, n_req):
    compared = 0
    for i in range(n_req):
        assert len(got[i]) == len(want[i]) >= 2, f"request {i}: {len(got[i])} chunks streamed, {len(want[i])} expected"
        for j, ((w, last), ref) in enumerate(zip(got[i], want[i])):
            assert w.dtype == np.float32 and np.array_equal(w, ref), f"request {i} chunk {j}"
            assert last == (j == len(want[i]) - 1)
            compared += 1
    assert compared == sum(len(w) for w in want.values())


def test_streamed_chunks_equal_the_chunks_of_each_request_alone(setup):
    tts, vcfg, reqs = setup
    want, ntoks = {}, {}
    for i, r in enumerate(reqs):
        want[i], ntoks[i] = _yardstick(tts, r, False, None)
    assert all(ntoks[i] == BUDGET for i in (0, 2, 3, 5)), ntoks   # no eos in their sets: they run to their budget
    got, order = _streamed(tts, reqs, do_sample=False, decode_stride=8)
    _compare(got, want, len(reqs))
    assert set(order[:3]) <= {0, 1, 2} and order.index(3) > 0       # three slots: the first three requests speak first
    # another stride polls at other steps and groups other chunks into its vocoder calls: the same chunks
    got3, _ = _streamed(tts, reqs, do_sample=False, decode_stride=3)
    _compare(got3, want, len(reqs))
    # and serve, the no-streaming front end, is what it was: it still answers, with one waveform per request
    served = dict(tts.serve([dict(r) for r in reqs[:2]], do_sample=False, max_new_tokens=BUDGET))
    assert sorted(served) == [0, 1] and all(len(w) > 0 for w in served.values())


def test_per_request_seeds(setup):
    """do_sample=True for the call, every request with its own seed: its chunks are those of the request sampled alone with it."""
    tts, vcfg, reqs = setup
    seeded = [dict(r, seed=100 + 7 * i) for i, r in enumerate(reqs)]
    want = {i: _yardstick(tts, r, True, None)[0] for i, r in enumerate(seeded)}
    got, _ = _streamed(tts, seeded, do_sample=True, decode_stride=5)
    _compare(got, want, len(seeded))
    greedy = {i: _yardstick(tts, r, False, None)[0] for i, r in enumerate(reqs)}
    assert any(len(want[i]) != len(greedy[i]) or not np.array_equal(want[i][0], greedy[i][0]) for i in want), "sampling changed nothing"


def test_refused_keys_raise_before_any_device_call(setup):
    tts, vcfg, reqs = setup
    calls = []
    inner = tts.model.admit
    tts.model.admit = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    begin = tts.model.session_begin
    tts.model.session_begin = lambda *a, **k: (calls.append(1), begin(*a, **k))[1]
    try:
        for bad in (dict(num_return_sequences=2), dict(return_log_probs=True)):
            with pytest.raises(ValueError):
                list(tts.serve_stream([dict(reqs[0]), dict(reqs[1], **bad)], do_sample=False, max_new_tokens=BUDGET, **STREAM))
        with pytest.raises(ValueError):
            list(tts.serve_stream([dict(reqs[0])], do_sample=False, max_new_tokens=BUDGET, decode_stride=0, **STREAM))
        assert not calls
    finally:
        tts.model.admit, tts.model.session_begin = inner, begin
