"""streaming.StreamMux on scripted token deltas (no GPU, no torch): whatever the granularity and interleaving of the pushes, a
request's chunks are those of one ChunkScheduler fed its semantic ids in one go; a control-mode request's chunks wait for its
speaker tokens; ``last`` is on exactly one chunk; ``close`` raises what ``SparkTTS.serve`` raises."""
import numpy as np
import pytest

from sparkmi.streaming import ChunkScheduler, StreamMux

NTOK = 8
SEM0, GLOB0, EOS, TEXT = 1000, 5000, 7, 42   # id ranges of a made-up vocabulary: semantic, global, a special id, a text id
SCHED = dict(audio_chunk_duration=0.5, max_audio_chunk_duration=4.0, audio_chunk_size_scale_factor=2.0, audio_chunk_overlap_duration=0.1)


class Tables:
    """What ``pipeline._TokenMap`` offers."""
    usable = True
    sem = {SEM0 + i: i for i in range(512)}
    glob = {GLOB0 + i: i for i in range(512)}
    special = {EOS}


def whole_history_parse(ids):
    return [i - SEM0 for i in ids if SEM0 <= i < SEM0 + 512], [i - GLOB0 for i in ids if GLOB0 <= i < GLOB0 + 512]


def in_one_go(sem):
    s = ChunkScheduler(**SCHED)
    return s.push(sem) + s.flush()


def script(rng, n_sem, control):
    """(generated ids, semantic indices, global indices): a control-mode request generates its speaker tokens first."""
    sem = rng.integers(0, 512, size=n_sem).tolist()
    glob = rng.integers(0, 512, size=NTOK).tolist()
    ids = ([GLOB0 + g for g in glob] if control else []) + [SEM0 + s for s in sem] + [EOS]
    return ids, sem, glob


def run(mux, scripts, steps, rng):
    """Feeds every request its ids in pieces of steps[key] ids (0: a random 1..40 each time), the requests interleaved in a
    random order; returns the chunk tuples in the order they came out."""
    pos = {k: 0 for k in scripts}
    out = []
    while pos:
        for k in rng.permutation(sorted(pos)).tolist():
            ids = scripts[k]
            n = steps[k] or int(rng.integers(1, 41))
            new = ids[pos[k]: pos[k] + n]
            pos[k] += len(new)
            done = pos[k] >= len(ids)
            got = mux.push(k, new, done)
            assert all(c[0] == k for c in got)
            out += got
            if done:
                del pos[k]
                mux.close(k)
    return out


@pytest.mark.parametrize("use_tables", [True, False])
def test_chunks_do_not_depend_on_the_granularity_of_the_pushes(use_tables):
    rng = np.random.Generator(np.random.PCG64(3))
    reqs = {k: script(rng, n, control=False) for k, n in enumerate([26, 25, 130, 31, 77, 400])}
    for steps in ([1] * 6, [7] * 6, [32] * 6, [1, 7, 32, 0, 0, 3], [0] * 6):
        mux = StreamMux(NTOK, Tables if use_tables else None, whole_history_parse, **SCHED)
        for k, (_, _, glob) in reqs.items():
            mux.open(k, glob)
        out = run(mux, {k: r[0] for k, r in reqs.items()}, dict(enumerate(steps)), rng)
        for k, (_, sem, glob) in reqs.items():
            mine = [c for c in out if c[0] == k]
            assert [c[2] for c in mine] == in_one_go(sem), f"request {k}, steps {steps}"
            assert [c[1] for c in mine] == list(range(len(mine)))
            assert [c[3] for c in mine] == [False] * (len(mine) - 1) + [True]
            assert len(mine) >= 2


def test_control_mode_chunks_wait_for_the_speaker_tokens():
    rng = np.random.Generator(np.random.PCG64(4))
    ids, sem, glob = script(rng, 90, control=True)
    mux = StreamMux(NTOK, Tables, None, **SCHED)
    # the model is free to interleave: 3 speaker tokens, 72 semantic tokens (two chunks' worth: 25, then 5 + 45 = 50), the rest
    order = ids[:3] + ids[NTOK: NTOK + 72] + ids[3:NTOK] + ids[NTOK + 72:]
    assert mux.push("c", order[:3], False) == [] and mux.global_ids("c") is None
    assert mux.push("c", order[3:75], False) == [], "two chunks are ready, the speaker tokens are not: nothing is released"
    got = mux.push("c", order[75: 75 + NTOK - 4], False)
    assert got == [] and mux.global_ids("c") is None, "one speaker token short"
    got = mux.push("c", order[75 + NTOK - 4: 75 + NTOK - 3], False)
    want = in_one_go(sem)
    assert [c[2] for c in got] == want[:2] and [c[1] for c in got] == [0, 1] and not any(c[3] for c in got)
    assert mux.global_ids("c") == glob
    got += mux.push("c", order[75 + NTOK - 3:], True)
    assert [c[2] for c in got] == want and [c[3] for c in got] == [False] * (len(want) - 1) + [True]
    mux.close("c")
    # a request that was never opened is a control-mode one
    mux.push("d", ids, True)
    mux.close("d")


def test_interleaved_clone_and_control_requests():
    rng = np.random.Generator(np.random.PCG64(5))
    reqs = {k: script(rng, n, control=bool(k % 2)) for k, n in enumerate([40, 60, 200, 33])}
    mux = StreamMux(NTOK, Tables, whole_history_parse, **SCHED)
    for k, (_, _, glob) in reqs.items():
        if not k % 2:
            mux.open(k, glob)
    out = run(mux, {k: r[0] for k, r in reqs.items()}, {k: 0 for k in reqs}, rng)
    for k, (_, sem, _) in reqs.items():
        mine = [c for c in out if c[0] == k]
        assert [c[2] for c in mine] == in_one_go(sem)
        assert sum(c[3] for c in mine) == 1 and mine[-1][3]


def test_a_text_id_moves_the_request_to_the_whole_history_parser():
    rng = np.random.Generator(np.random.PCG64(6))
    ids, sem, glob = script(rng, 70, control=False)
    ids = ids[:30] + [TEXT] + ids[30:]
    mux = StreamMux(NTOK, Tables, whole_history_parse, **SCHED)
    mux.open(0, glob)
    out = []
    for i in range(0, len(ids), 9):
        out += mux.push(0, ids[i: i + 9], i + 9 >= len(ids))
    assert [c[2] for c in out] == in_one_go(sem)
    with pytest.raises(ValueError):      # no callable to fall back to
        m2 = StreamMux(NTOK, Tables, None, **SCHED)
        m2.open(0, glob)
        m2.push(0, ids, True)


def test_close_raises_what_serve_raises():
    mux = StreamMux(NTOK, Tables, None, **SCHED)
    mux.open("no_sem", list(range(NTOK)))
    assert mux.push("no_sem", [EOS], True) == []
    with pytest.raises(ValueError, match="no semantic tokens"):
        mux.close("no_sem")
    mux.push("few_glob", [GLOB0 + 1, GLOB0 + 2] + [SEM0 + i for i in range(30)], True)   # control mode, 2 of 8 speaker tokens
    with pytest.raises(ValueError, match="global tokens"):
        mux.close("few_glob")
    mux.open("wrong_glob", list(range(NTOK + 1)))
    mux.push("wrong_glob", [SEM0] * 30, True)
    with pytest.raises(ValueError, match="global tokens"):
        mux.close("wrong_glob")
    mux.push("many_glob", [GLOB0 + i for i in range(NTOK + 1)] + [SEM0] * 30, True)      # control mode, one too many
    with pytest.raises(ValueError, match="global tokens"):
        mux.close("many_glob")
    with pytest.raises(ValueError):
        StreamMux(NTOK, None, None)
    with pytest.raises(AssertionError):   # ChunkScheduler's own argument checks, before any request
        StreamMux(NTOK, Tables, None, audio_chunk_duration=0.1)


def test_zero_overlap_ending_on_a_boundary_still_flags_one_chunk():
    kw = dict(SCHED, audio_chunk_overlap_duration=0.0)
    mux = StreamMux(NTOK, Tables, None, **kw)
    mux.open(0, list(range(NTOK)))
    a = mux.push(0, [SEM0 + i for i in range(25)], False)     # exactly the first chunk; nothing is left in the scheduler
    b = mux.push(0, [EOS], True)
    assert [c[2] for c in a] == [list(range(25))] and not a[0][3]
    assert b == [(0, 1, [], True)]
    mux.close(0)
