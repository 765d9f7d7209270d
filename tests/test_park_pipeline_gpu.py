"""SparkTTS.serve_stream with parking: five requests -- a control-mode one, whose speaker tokens the model generates, and four
clone-from-tokens ones -- through two decode rows with up to five open, under a fake clock.  Every request's chunks -- samples,
boundaries, ``last`` flags -- must equal, bit for bit, those of the same call without the pacing keywords; the default call
must not touch the save / restore entry points at all."""
import math

import numpy as np
import pytest
import torch

from sparkmi.streaming import Pacer

pytestmark = pytest.mark.gpu

STREAM = dict(audio_chunk_duration=0.5, audio_chunk_overlap_duration=0.1, max_new_tokens=64, decode_stride=8)


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    from sparkmi import synthetic
    from sparkmi.pipeline import SparkTTS, _request_sampling
    d = tmp_path_factory.mktemp("spark_synth_park")
    lcfg, vcfg = synthetic.make_model_dir(d)
    tts = SparkTTS(d, torch.device("cuda:0"), max_batch=2, max_positions=512, max_frames=256)
    rng = np.random.Generator(np.random.PCG64(23))
    sem_ids = sorted(tts._map.sem)
    reqs = []
    for i in range(5):
        glob = torch.from_numpy(rng.integers(0, 4096, size=(1, 1, vcfg.spk_token_num)))
        reqs.append(dict(text=f"parked utterance {i} " * (1 + i % 3), prompt_tokens=(glob, torch.zeros((1, 0), dtype=torch.long)),
                         allowed_token_ids=list(sem_ids)))
    # request 0 is a control-mode one: the model itself has to emit the spk_token_num speaker tokens before anything else.  The
    # synthetic weights would not, so a sequence bias makes them: +2B on g[0] after the prompt's last id and on g[i + 1] after
    # g[i] (the prompt counts as bias context), -B on every g[i] wherever it stands, B far above any logit.  At the start of
    # the chain the sum is +B, anywhere else -B: exactly these ids, once, in order, then semantic ids only.
    ntok, B = vcfg.spk_token_num, 1e4
    inv = {v: k for k, v in tts._map.glob.items()}
    want_glob = [int(v) for v in rng.permutation(len(inv))[:ntok]]
    g = [inv[v] for v in want_glob]
    ctl = dict(text="a created voice", gender="female", pitch="high", speed="low", allowed_token_ids=sorted(sem_ids + g))
    prompt = tts.process_prompt_control(ctl["gender"], ctl["pitch"], ctl["speed"], ctl["text"])
    last = tts.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()[-1]
    ctl["sequence_bias"] = ([((last, g[0]), 2 * B)] + [((g[i], g[i + 1]), 2 * B) for i in range(ntok - 1)] + [((t,), -B) for t in g])
    reqs[0] = ctl
    reqs[1].update(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=31)
    # request 2 stops on a pair of ids it emits late: tokens of the request alone (the admission path), then the pair at 40, 41
    r = reqs[2]
    prompt, _ = tts.process_prompt(r["text"], None, None, r["prompt_tokens"])
    ids = tts.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
    tts.model.set_sampling(False)
    toks = tts.model.generate_ragged([ids], [64], tts._eos, sampling=[_request_sampling(r, tts.speech_token_ids)])[0]
    at = next(i for i in range(40, 60) if not any(toks[j: j + 2] == toks[i: i + 2] for j in range(i)))
    r["stop_sequences"] = [toks[at: at + 2]]
    return tts, reqs, at + 2, want_glob


def _streamed(tts, reqs, **kw):
    out = {i: [] for i in range(len(reqs))}
    for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, **dict(STREAM, **kw)):
        assert not out[i] or not out[i][-1][1], f"request {i}: a chunk after its last one"
        out[i].append((w, last))
    return out


class Clock:
    """Advanced by the test: 10 ms per chunk a listener receives."""

    def __init__(self):
        self.t = 0.0

    def __call__(self):
        return self.t


class LoggingPacer(Pacer):
    """Remembers whom it named."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.parked_keys, self.resumed_keys = [], []

    def to_park(self, *a):
        out = super().to_park(*a)
        self.parked_keys += out
        return out

    def to_resume(self, *a):
        out = super().to_resume(*a)
        self.resumed_keys += out
        return out


def test_parked_requests_stream_the_same_chunks(setup):
    tts, reqs, n2, want_glob = setup
    voc = tts.audio_tokenizer.model
    hop, rate = voc.hop, tts.sample_rate // voc.hop
    calls, seen_glob = [], {}
    inner = {n: getattr(tts.model, n) for n in ("save_slots", "restore_slots", "park")}
    for n, f in inner.items():
        setattr(tts.model, n, lambda *a, _f=f, _n=n, **k: (calls.append(_n), _f(*a, **k))[1])
    detok = voc.detokenize_rows

    def spy(sem_t, glob_t, **k):    # the speaker tokens each vocoder row is given
        for row in glob_t.reshape(glob_t.shape[0], -1).tolist():
            seen_glob[tuple(row)] = seen_glob.get(tuple(row), 0) + 1
        return detok(sem_t, glob_t, **k)

    voc.detokenize_rows = spy
    try:
        want = _streamed(tts, reqs)
        assert not calls, "the default call neither saves nor restores"
        assert seen_glob.get(tuple(want_glob), 0) == len(want[0]), "the control request is vocoded with the speaker tokens it generated"
        inert = _streamed(tts, reqs, max_ahead=0.2)          # max_ahead without max_open > max_batch: accepted and inert
        assert not calls
        clk = Clock()
        pacer = LoggingPacer(2, 5, 0.2, frame_rate=rate, clock=clk)
        got = {i: [] for i in range(len(reqs))}
        for i, w, last in tts.serve_stream([dict(r) for r in reqs], do_sample=False, pacer=pacer, **STREAM):
            got[i].append((w, last))
            clk.t += 0.01
    finally:
        voc.detokenize_rows = detok
        for n in inner:
            delattr(tts.model, n)
    parks, resumes = pacer.parks, pacer.resumes
    assert parks >= 2 and resumes >= 2 and parks == resumes, (parks, resumes)
    assert calls.count("park") >= 1 and calls.count("restore_slots") >= 1
    assert sorted(pacer.parked_keys) == sorted(pacer.resumed_keys)
    assert 0 in pacer.parked_keys, f"the control-mode request was never parked: {pacer.parked_keys}"
    assert len(set(pacer.parked_keys) - {0}) >= 1, "a clone request is parked too"
    assert not pacer._first and not pacer._frames, "the pacer forgets a request with its last chunk"
    for res in (inert, got):
        for i in range(len(reqs)):
            assert len(res[i]) == len(want[i]) >= 2, f"request {i}: {len(res[i])} chunks, {len(want[i])} without parking"
            for j, ((w, last), (ref, rlast)) in enumerate(zip(res[i], want[i])):
                assert w.dtype == np.float32 and w.shape == ref.shape and np.array_equal(w, ref), f"request {i} chunk {j}"
                assert last == rlast == (j == len(want[i]) - 1)
    # what each request said: all its semantic tokens, each chunk after the first repeating `overlap` frames of its predecessor
    overlap = math.ceil(STREAM["audio_chunk_overlap_duration"] * rate)
    frames = lambda i: sum(len(w) for w, _ in want[i]) // hop - overlap * (len(want[i]) - 1)
    assert frames(0) == STREAM["max_new_tokens"] - len(want_glob), "the control request: its budget less the speaker tokens"
    assert frames(2) == n2 < STREAM["max_new_tokens"], "the stop sequence ended request 2"
    assert frames(1) == frames(3) == frames(4) == STREAM["max_new_tokens"]


def test_pacing_arguments_are_checked_before_the_device(setup):
    tts, reqs, _, _ = setup
    calls = []
    begin = tts.model.session_begin
    tts.model.session_begin = lambda *a, **k: (calls.append(1), begin(*a, **k))[1]
    try:
        for bad in (dict(max_open=0), dict(max_open=2.5), dict(max_open=5, max_ahead=0), dict(max_open=5, max_ahead=1.0, resume_ahead=2.0),
                    dict(max_open=5, max_ahead=1.0, resume_ahead=-1), dict(pacer=Pacer(2, 5, 1.0), max_open=5),   # one or the other
                    dict(pacer=Pacer(3, 5, 1.0)), dict(pacer=object())):
            with pytest.raises(ValueError):
                list(tts.serve_stream([dict(reqs[0])], do_sample=False, **dict(STREAM, **bad)))
        assert not calls
    finally:
        tts.model.session_begin = begin
