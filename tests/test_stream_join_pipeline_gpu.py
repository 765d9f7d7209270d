"""``joined=True`` through SparkTTS.serve_stream and inference_stream on a synthetic model directory (the recipe of
tests/test_serve_stream_gpu.py: six clone-mode requests through three slots, first chunk 25 frames, overlap 5, budget 48).

Yardstick per request: ``streaming.crossfade`` of its ``joined=False`` chunks cast to float32 -- the joined pieces' concatenation
must equal it bit for bit -- and, at another output rate, ``DeviceAudio.resample_rows`` of that joined waveform, bit for bit, with
``out_len(semantic tokens * hop)`` samples; whatever the poll stride, with parking on, and from ``inference_stream``.  The default
calls still yield the chunks of the existing test's yardstick, and ``joined=False`` still refuses an output rate."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1)
BUDGET = 48
OVERLAP_FRAMES = 5


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS
    from sparkmi.streaming import crossfade
    d = tmp_path_factory.mktemp("spark_synth_join")
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
    # the joined=False chunks of the greedy call, once: every other test compares with what they give
    hop = tts.audio_tokenizer.model.hop
    n = OVERLAP_FRAMES * hop
    chunks = {i: [] for i in range(len(reqs))}
    for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, max_new_tokens=BUDGET, **STREAM):
        chunks[i].append(w)
    assert all(len(c) >= 2 and all(w.size >= 2 * n for w in c) for c in chunks.values()), "every chunk holds two overlaps"
    want = {i: crossfade(c, n).astype(np.float32) for i, c in chunks.items()}
    n_sem = {i: (sum(w.size for w in c) - n * (len(c) - 1)) // hop for i, c in chunks.items()}
    assert all(want[i].size == n_sem[i] * hop for i in want)
    return tts, reqs, chunks, want, n_sem


def _resampled(tts, want, sr):
    """DeviceAudio.resample_rows of every request's joined waveform, row by row"""
    from sparkmi import audio
    up, down = audio.ratio(16000, sr)
    out = {}
    for i, x in want.items():
        y, n_out = tts._device_audio().resample_rows(torch.from_numpy(x[None]).cuda(), [x.size], [up], [down])
        out[i] = y.cpu().numpy()[0, : n_out[0]].copy()
    return out, (up, down)


def _joined(tts, reqs, **kw):
    """{request: its pieces' concatenation} of a joined serve_stream call, with the checks every such call must pass"""
    pieces = {i: [] for i in range(len(reqs))}
    lasts = {i: 0 for i in range(len(reqs))}
    for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, max_new_tokens=BUDGET, joined=True, **dict(STREAM, **kw)):
        assert w.dtype == np.float32 and w.ndim == 1 and not lasts[i], f"request {i}: a piece after its last one"
        pieces[i].append(w)
        lasts[i] += bool(last)
    assert all(v == 1 for v in lasts.values()), "last is on exactly one piece of every request"
    return {i: np.concatenate(p) for i, p in pieces.items()}


def _same(got, want):
    for i in want:
        assert got[i].size == want[i].size, f"request {i}: {got[i].size} samples, {want[i].size} expected"
        assert np.array_equal(got[i], want[i]), f"request {i}: {np.count_nonzero(got[i] != want[i])} samples differ"


def test_joined_pieces_are_the_crossfade_of_the_chunks(setup):
    tts, reqs, chunks, want, n_sem = setup
    _same(_joined(tts, reqs, decode_stride=8), want)
    _same(_joined(tts, reqs, decode_stride=8, output_sample_rate=16000), want)   # the model's own rate: the join alone
    _same(_joined(tts, reqs, decode_stride=3), want)                             # other polls, other rows in the calls


@pytest.mark.parametrize("sr", [24000, 44100])
def test_joined_pieces_at_another_rate_are_the_resampled_joined_waveform(setup, sr):
    from sparkmi import audio
    tts, reqs, chunks, want, n_sem = setup
    ref, (up, down) = _resampled(tts, want, sr)
    hop = tts.audio_tokenizer.model.hop
    assert all(ref[i].size == audio.out_len(n_sem[i] * hop, up, down) for i in ref)
    _same(_joined(tts, reqs, decode_stride=8, output_sample_rate=sr), ref)
    _same(_joined(tts, reqs, decode_stride=5, output_sample_rate=sr), ref)


def test_joined_with_parking(setup):
    """six open requests on three rows, a request parked as soon as it is 50 ms ahead of its listener: the joiner's state is
    keyed by request, so the pieces are those of the call without parking"""
    from sparkmi.streaming import Pacer
    tts, reqs, chunks, want, n_sem = setup
    ref, _ = _resampled(tts, want, 24000)

    class Clock:
        t = 0.0

        def __call__(self):
            return self.t

    for rate, yard in ((None, want), (24000, ref)):
        clk = Clock()
        pacer = Pacer(3, 6, 0.05, frame_rate=50, clock=clk)
        pieces = {i: [] for i in range(len(reqs))}
        for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, max_new_tokens=BUDGET, joined=True, pacer=pacer,
                                           output_sample_rate=rate, **STREAM):
            pieces[i].append(w)
            clk.t += 0.01
        assert pacer.parks >= 1 and pacer.parks == pacer.resumes, (pacer.parks, pacer.resumes)
        _same({i: np.concatenate(p) for i, p in pieces.items()}, yard)


def test_inference_stream_joined(setup):
    from sparkmi import audio
    from sparkmi.streaming import crossfade
    tts, reqs, chunks, want, n_sem = setup
    r = reqs[2]
    kw = dict(prompt_tokens=r["prompt_tokens"], do_sample=False, max_new_tokens=BUDGET, **STREAM)
    hop, size = tts.audio_tokenizer.model.hop, tts.audio_tokenizer.model.cfg.codebook_size
    n = OVERLAP_FRAMES * hop
    # inference_stream takes no allowed_token_ids: random weights run to the budget (no eos) and every id is read as a semantic
    # token, for all three calls alike, so the request has its 48 tokens -- chunks of 25 and 28 frames
    parse, eos = tts._parse, tts._eos
    tts._parse, tts._eos = (lambda ids: ([int(t) % size for t in ids], [])), None
    try:
        plain = list(tts.inference_stream(r["text"], **kw))
        assert len(plain) >= 2 and all(w.size >= 2 * n for w in plain)
        x = crossfade(plain, n).astype(np.float32)
        assert x.size == BUDGET * hop
        got = list(tts.inference_stream(r["text"], joined=True, **kw))
        assert all(w.dtype == np.float32 and w.size for w in got) and np.array_equal(np.concatenate(got), x)
        y, n_out = tts._device_audio().resample_rows(torch.from_numpy(x[None]).cuda(), [x.size], [3], [2])
        got = np.concatenate(list(tts.inference_stream(r["text"], joined=True, output_sample_rate=24000, **kw)))
        assert got.size == n_out[0] == audio.out_len(x.size, 3, 2) and np.array_equal(got, y.cpu().numpy()[0, : n_out[0]])
    finally:
        tts._parse, tts._eos = parse, eos


def test_an_empty_last_chunk_flushes_the_resampler(setup):
    """Zero overlap: the join is plain concatenation.  Request a emits 25 semantic tokens -- exactly its first chunk, read in the
    third poll -- and its eos in the fourth, so its last chunk is empty; alone, and beside a request whose flush is ready in
    that same poll."""
    from sparkmi import audio
    tts, reqs, chunks, want, n_sem = setup
    hop = tts.audio_tokenizer.model.hop
    kw = dict(do_sample=False, max_new_tokens=33, decode_stride=8, audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.0)
    a = dict(reqs[1], min_new_tokens=25, eos_bias=1e4)      # (reqs[1] allows eos: it ends at the first token it may)
    for group in ([a], [a, dict(reqs[0])]):
        plain = {i: [] for i in range(len(group))}
        for i, w, last in tts.serve_stream([dict(r) for r in group], **kw):
            plain[i].append(w)
        assert [w.size for w in plain[0]] == [25 * hop, 0], "the premise: a full first chunk, then an empty last one"
        x = {i: np.concatenate(c) for i, c in plain.items()}
        for sr in (None, 24000):
            up, down = (1, 1) if sr is None else audio.ratio(16000, sr)
            pieces, lasts = {i: [] for i in plain}, {i: [] for i in plain}
            for i, w, last in tts.serve_stream([dict(r) for r in group], joined=True, output_sample_rate=sr, **kw):
                pieces[i].append(w)
                lasts[i].append(bool(last))
            for i in plain:
                assert lasts[i] == [False] * (len(lasts[i]) - 1) + [True] and len(pieces[i]) == len(plain[i])
                ref = x[i]
                if sr is not None:
                    y, n_out = tts._device_audio().resample_rows(torch.from_numpy(x[i][None]).cuda(), [x[i].size], [up], [down])
                    ref = y.cpu().numpy()[0, : n_out[0]]
                    assert pieces[0][-1].size > 0, "the empty last chunk carries the filter's latency out"
                assert np.array_equal(np.concatenate(pieces[i]), ref), f"request {i} at {sr}"


def _yardstick(tts, r, budget=BUDGET):
    """[chunk waveforms] of one request: the admission path alone, one scheduler, every chunk vocoded on its own (the yardstick
    of tests/test_serve_stream_gpu.py)."""
    from sparkmi.pipeline import _request_sampling
    from sparkmi.streaming import ChunkScheduler
    prompt, g = tts.process_prompt(r["text"], None, None, r["prompt_tokens"])
    ids = tts.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
    tts.model.set_sampling(False, 0.8, 50, 0.95, None)
    toks = tts.model.generate_ragged([ids], [budget], tts._eos, sampling=[_request_sampling(r, tts.speech_token_ids)])[0]
    stops = [toks.index(e) for e in tts._eos if e in toks]
    if stops:
        toks = toks[: min(stops) + 1]
    sem, _ = tts._parse(toks)
    sched = ChunkScheduler(STREAM["audio_chunk_duration"], 30.0, 8.0, STREAM["audio_chunk_overlap_duration"], 50)
    cut = sched.push(sem) + sched.flush()
    voc, hop = tts.audio_tokenizer.model, tts.audio_tokenizer.model.hop
    g = torch.as_tensor(g).reshape(1, 1, -1)
    return [voc.detokenize(torch.tensor([c], dtype=torch.long), g).reshape(-1)[: len(c) * hop].cpu().numpy().copy() for c in cut]


def test_default_calls_yield_what_they_yielded_before(setup):
    tts, reqs, chunks, want, n_sem = setup
    for i, r in enumerate(reqs):
        yard = _yardstick(tts, r)
        assert len(chunks[i]) == len(yard)
        for j, (a, b) in enumerate(zip(chunks[i], yard)):
            assert a.dtype == np.float32 and np.array_equal(a, b), f"request {i} chunk {j}"
    # the keyword at its default is the call without it, after joined calls have run on this session too
    again = {i: [] for i in range(len(reqs))}
    for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, max_new_tokens=BUDGET, joined=False, **STREAM):
        again[i].append(w)
    assert all(len(again[i]) == len(chunks[i]) and all(np.array_equal(a, b) for a, b in zip(again[i], chunks[i])) for i in chunks)


def test_refusals(setup):
    tts, reqs, chunks, want, n_sem = setup
    calls = []
    inner, begin = tts.model.admit, tts.model.session_begin
    tts.model.admit = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    tts.model.session_begin = lambda *a, **k: (calls.append(1), begin(*a, **k))[1]
    try:
        kw = dict(do_sample=False, max_new_tokens=BUDGET)
        with pytest.raises(ValueError, match="output_sample_rate"):      # joined=False with a rate still raises
            next(tts.serve_stream([dict(reqs[0])], output_sample_rate=24000, **kw, **STREAM))
        with pytest.raises(ValueError, match="output_sample_rate"):
            next(tts.inference_stream(reqs[0]["text"], prompt_tokens=reqs[0]["prompt_tokens"], output_sample_rate=24000, joined=False, **kw))
        # a first chunk of 25 frames cannot hold two overlaps of 13
        short = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.26)
        with pytest.raises(ValueError, match="two overlaps"):
            next(tts.serve_stream([dict(reqs[0])], joined=True, **kw, **short))
        with pytest.raises(ValueError, match="two overlaps"):
            next(tts.inference_stream(reqs[0]["text"], prompt_tokens=reqs[0]["prompt_tokens"], joined=True, **kw, **short))
        with pytest.raises(ValueError, match="output_sample_rate"):
            next(tts.serve_stream([dict(reqs[0])], joined=True, output_sample_rate=0, **kw, **STREAM))
        assert not calls
    finally:
        tts.model.admit, tts.model.session_begin = inner, begin
