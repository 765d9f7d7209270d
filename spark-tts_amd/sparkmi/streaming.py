"""Streaming (chunked) vocoding: audio is emitted while the LLM is still generating.

Mirrors the reference's decoupled Triton mode: the server side cuts the growing semantic-token
stream into chunks that overlap by ``audio_chunk_overlap_duration`` and grow by
``audio_chunk_size_scale_factor`` up to ``max_audio_chunk_duration``
(``runtime/triton_trtllm/model_repo/spark_tts/1/model.py:347-385``; defaults
``runtime/triton_trtllm/run.sh:53-56``), each chunk is vocoded on its own, and the client
cross-fades consecutive chunks over the overlap (``runtime/triton_trtllm/client_grpc.py:390-415``).

``ChunkScheduler`` is the pure host logic (no GPU), ``crossfade`` the client-side reconstruction;
``SparkTTS.inference_stream`` (pipeline.py) drives the HIP LLM and vocoder with them.  ``StreamMux`` is the same logic for many
requests at once -- the decoupled chunk loop answering every live request of an in-flight batch (run.sh:49-65) -- and
``SparkTTS.serve_stream`` drives it.  ``join_piece_len``, ``join_history`` and ``split_calls`` are the host arithmetic of the
device-side stream joiner (``joined=True``; include/sparkmi.h, smi_join_*), which does on the device what ``crossfade`` does here;
``tempo_piece_len``, ``tempo_ready``, ``tempo_history_start`` and ``tempo_history`` are that of the tempo stage behind it
(smi_tempos_*): when a frame of a stream that is still arriving is final; ``pitch_plan``, ``pitch_final``, ``pitch_tail_start``
and ``pitch_piece_len`` are that of the pitch stage that takes its place (smi_pitchs_*): when an output of the resampler behind
the stretch is final.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Hashable, Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np


class ChunkScheduler:
    """Feed semantic tokens as they are generated; ``push`` returns the chunks that became ready
    and ``flush`` the final (shorter) one.  Token bookkeeping is exactly the reference loop's:
    a ready chunk is the first ``chunk_size`` buffered tokens, the buffer then keeps the last
    ``overlap`` of them, and ``chunk_size`` grows (model.py:358-375)."""

    def __init__(self, audio_chunk_duration: float = 1.0, max_audio_chunk_duration: float = 30.0,
                 audio_chunk_size_scale_factor: float = 8.0, audio_chunk_overlap_duration: float = 0.1,
                 frame_rate: int = 50):
        # same argument checks as model.py:121-129
        assert float(audio_chunk_duration) >= 0.5, "audio_chunk_duration at least 0.5 seconds"
        assert float(audio_chunk_size_scale_factor) >= 1.0, \
            "audio_chunk_size_scale_factor should be greater than 1, change it according to your actual rtf"
        self.max_chunk_size = math.ceil(max_audio_chunk_duration * frame_rate)
        self.chunk_size = math.ceil(audio_chunk_duration * frame_rate)
        self.overlap = math.ceil(audio_chunk_overlap_duration * frame_rate)
        self.scale = float(audio_chunk_size_scale_factor)
        self.buf: List[int] = []

    def push(self, tokens: Iterable[int]) -> List[List[int]]:
        out = []
        for t in tokens:
            self.buf.append(int(t))
            if len(self.buf) >= self.chunk_size:
                out.append(self.buf[: self.chunk_size])
                self.buf = self.buf[self.chunk_size - self.overlap:]
                self.chunk_size = min(self.max_chunk_size, int(self.chunk_size * self.scale))
        return out

    def flush(self) -> List[List[int]]:
        out = [self.buf] if self.buf else []
        self.buf = []
        return out


def crossfade(chunks: Sequence[np.ndarray], overlap_samples: int) -> np.ndarray:
    """Client-side reconstruction (client_grpc.py:390-415): linear fade over the overlap; the
    first chunk loses its tail, middle chunks lose both ends, the last chunk's tail is kept."""
    chunks = [np.asarray(c).reshape(-1) for c in chunks if np.asarray(c).size > 0]
    if not chunks:
        return np.zeros(0, dtype=np.float32)
    if len(chunks) == 1:
        return chunks[0]
    n = int(overlap_samples)
    fade_out = np.linspace(1, 0, n)
    fade_in = np.linspace(0, 1, n)
    out = [chunks[0][:-n]]
    for i in range(1, len(chunks)):
        out.append(chunks[i][:n] * fade_in + chunks[i - 1][-n:] * fade_out)
        out.append(chunks[i][n:-n])
    out.append(chunks[-1][-n:])
    return np.concatenate(out)


# ---- joined streaming (include/sparkmi.h, smi_join_*): the host arithmetic of the device-side stream joiner, no torch
JOIN_MAX_ROWS = 64     # rows of one smi_join_push_rows call


def join_history(up: int, down: int, half: int) -> int:
    """input samples of history a stream keeps for taps h[0 .. 2 half]: ceil((2H + down) / up) + 1 (0 for up = down = 1)"""
    if up == 1 and down == 1:
        return 0
    return -((-(2 * int(half) + int(down))) // int(up)) + 1


def join_piece_len(overlap: int, up: int, down: int, half: int, first: bool, n_before: int, k_before: int, length: int,
                   last: bool) -> Tuple[int, int, int]:
    """(piece length, N after, K after) of one push -- the twin of ``smi_join_piece_len``: a stream with ``n_before`` joined
    samples and ``k_before`` emitted outputs takes a chunk of ``length`` samples.  A chunk that is not the last needs
    ``length >= 2 overlap``, a last chunk that is not the first ``length >= overlap`` (ValueError).  The joined stream grows by
    ``length`` (last) or ``length - overlap`` (the tail is held back for the next fade); a stream that goes on has emitted
    ``max(0, ceil((N up - H) / down))`` outputs, a finished one ``ceil(N up / down)``; at 1/1 the piece is the joined samples."""
    overlap, up, down, half, length = int(overlap), int(up), int(down), int(half), int(length)
    if not last and length < 2 * overlap:
        raise ValueError(f"a chunk of {length} samples that is not the last is shorter than 2 * overlap = {2 * overlap}")
    if last and not first and length < overlap:
        raise ValueError(f"a last chunk of {length} samples is shorter than the overlap of {overlap}")
    n = int(n_before) + length - (0 if last else overlap)
    if up == 1 and down == 1:
        k = n
    elif last:
        k = -((-n * up) // down)
    else:
        k = max(0, -((-(n * up - half)) // down))
    return k - int(k_before), n, k


def split_calls(keys: Sequence[Hashable], max_rows: int = JOIN_MAX_ROWS) -> List[Tuple[int, int]]:
    """One poll's ready chunks, in order, as row ranges [(start, stop)] of joiner calls: a request appears at most once in a
    call (it can have two chunks ready in one poll, its last full chunk and its flush), a call has at most ``max_rows`` rows,
    and the order of a request's chunks is kept because the ranges are consecutive."""
    out, start, seen = [], 0, set()
    for i, k in enumerate(keys):
        if k in seen or i - start >= max_rows:
            out.append((start, i))
            start, seen = i, set()
        seen.add(k)
    if len(keys) > start:
        out.append((start, len(keys)))
    return out


# ---- tempo of joined streams (include/sparkmi.h, smi_tempos_*): when a frame is final, as host arithmetic
def _tempo_nominal(k: int, p: int, q: int, H: int) -> int:
    return (k * H * p) // q


def tempo_ready(k: int, p: int, q: int, N: int, D: int) -> int:
    """R_k: the input samples a stream must hold before frame ``k`` is final -- H for frame 0, else
    ``max(a_k, a_{k-1} + H) + D + N``"""
    H = int(N) // 2
    if k == 0:
        return H
    return max(_tempo_nominal(k, p, q, H), _tempo_nominal(k - 1, p, q, H) + H) + int(D) + int(N)


def tempo_history_start(frames: int, p: int, q: int, N: int, D: int) -> int:
    """the first input sample a stream that has emitted ``frames`` frames still needs: ``max(0, min(a_F, a_{F-1} + H) - D)``,
    0 before the first frame, and everything is behind a stream at p = q"""
    H = int(N) // 2
    if frames == 0:
        return 0
    return max(0, min(_tempo_nominal(frames, p, q, H), _tempo_nominal(frames - 1, p, q, H) + H) - int(D))


def tempo_history(N: int, D: int) -> int:
    """input samples of history a tempo stream keeps, enough for every p / q in 1/4 .. 4: ``max(7 H + D, 5 H + 2 D)``"""
    H = int(N) // 2
    return max(7 * H + int(D), 5 * H + 2 * int(D))


def tempo_piece_len(p: int, q: int, N: int, D: int, n_before: int, frames_before: int, length: int, last: bool) -> Tuple[int, int, int]:
    """(piece length, n after, frames after) of one push -- the twin of ``smi_tempos_piece_len``: a stream at tempo p / q that
    holds ``n_before`` input samples and has emitted ``frames_before`` frames of H = N / 2 outputs takes ``length`` more.  A
    stream that goes on emits the longest prefix of frames k with ``n >= tempo_ready(k)`` and ``(k + 1) H <= ceil(n q / p)``; a
    finished one has emitted ``ceil(n q / p)``; at p = q the piece is the chunk.  ValueError for a bad argument."""
    p, q, N, D, n_before, frames_before, length = int(p), int(q), int(N), int(D), int(n_before), int(frames_before), int(length)
    if not (1 <= p <= 32767 and 1 <= q <= 32767 and p <= 4 * q and q <= 4 * p):
        raise ValueError(f"tempo p/q = {p}/{q} outside 1/4..4 with 1 <= p, q <= 32767")
    if N < 16 or N > 2048 or N % 2 or not 0 <= D <= 1024:
        raise ValueError(f"frame N={N} must be even in 16..2048 and the radius D={D} in 0..1024")
    if n_before < 0 or frames_before < 0 or length < 0:
        raise ValueError("negative counter or length")
    H = N // 2
    n = n_before + length
    M = -((-n * q) // p)
    whole = (M - 1) // H + 1 if M else 0
    if p == q:
        return length, n, (whole if last else n // H)
    if last:
        f, piece = whole, M - frames_before * H
    else:
        f = frames_before
        while (f + 1) * H <= M and n >= tempo_ready(f, p, q, N, D):
            f += 1
        piece = (f - frames_before) * H
    if piece < 0:
        raise ValueError(f"{frames_before} frames cannot have left a stream of {n} samples")
    return piece, n, f


# ---- pitch shift of joined streams (include/sparkmi.h, smi_pitchs_*): when an output is final, as host arithmetic
def pitch_plan(tp: int, tq: int, rp: int, rq: int) -> Tuple[int, int, int, int]:
    """(P, Q, up, down): the stretch ``(tp rq) / (tq rp)`` and the resampling ``rq / rp`` of a tempo tp / tq and a pitch ratio
    rp / rq, each in lowest terms"""
    tp, tq, rp, rq = int(tp), int(tq), int(rp), int(rq)
    if min(tp, tq, rp, rq) < 1 or max(tp, tq, rp, rq) > 32767:
        raise ValueError(f"tempo {tp}/{tq} and pitch ratio {rp}/{rq} must have terms in 1..32767")
    a, b = tp * rq, tq * rp
    g, gr = math.gcd(a, b), math.gcd(rp, rq)
    return a // g, b // g, rq // gr, rp // gr


def pitch_final(E: int, up: int, down: int, half: int) -> int:
    """K: the final outputs of a stream that goes on and has emitted ``E`` stretched samples, ``max(0, ceil((E up - G) / down))``"""
    return max(0, -((-(int(E) * int(up) - int(half))) // int(down)))


def pitch_tail_start(K: int, up: int, down: int, half: int) -> int:
    """the first stretched sample that output ``K`` and those behind it reach: ``max(0, ceil((K down - G) / up))``"""
    return max(0, -((-(int(K) * int(down) - int(half))) // int(up)))


def pitch_piece_len(tp: int, tq: int, rp: int, rq: int, N: int, D: int, n_taps: int, n_before: int, frames_before: int, k_before: int,
                    length: int, last: bool) -> Tuple[int, int, int, int]:
    """(piece length, n after, frames after, outputs after) of one push -- the twin of ``smi_pitchs_piece_len``: the stretch is
    a tempo stream at P / Q (``tempo_piece_len``) that has emitted E samples; a stream that goes on has emitted
    ``pitch_final(E)`` outputs, a finished one ``ceil(n tq / tp)``.  ValueError for a bad argument."""
    P, Q, up, down = pitch_plan(tp, tq, rp, rq)
    n_taps, k_before = int(n_taps), int(k_before)
    half = n_taps // 2
    if (up, down) == (1, 1):
        if n_taps:
            raise ValueError(f"a stream at the pitch ratio 1/1 takes no taps, not {n_taps}")
    elif n_taps < 3 or n_taps % 2 == 0 or n_taps >= 1 << 15 or half < up:
        raise ValueError(f"{n_taps} taps: odd, at least 3 and G >= up = {up} at the pitch ratio {rp}/{rq}")
    if k_before < 0:
        raise ValueError("negative counter")
    if int(n_before) > 1 << 28 or int(length) > 1 << 28:
        raise ValueError("2^28 samples are the limit of a stream")
    _, n, f = tempo_piece_len(P, Q, N, D, n_before, frames_before, length, last)
    if last:
        E, K = -((-n * Q) // P), -((-n * int(tq)) // int(tp))
        if -((-E * up) // down) < K:
            raise ValueError(f"the stretched stream resamples to fewer samples than the stream's length {K}")
    else:
        E = n if P == Q else f * (int(N) // 2)
        K = pitch_final(E, up, down, half)
    if K < k_before:
        raise ValueError(f"{k_before} outputs cannot have left a stream of {n} samples")
    if E * up >= 1 << 31 or K * down >= 1 << 31:
        raise ValueError("E up or K down reaches 2^31: the limit of a stream")
    return K - k_before, n, f, K


# ---- loudness of joined streams (include/sparkmi.h, smi_louds_*): what a push emits, as host arithmetic
def loudness_knots(n: int, hop: int) -> int:
    """knots a stream of ``n`` samples that goes on has made: knot j needs blocks 0 .. j whole, ``n >= (j + 4) hop``"""
    return max(0, int(n) // int(hop) - 3)


def loudness_emitted(n: int, hop: int) -> int:
    """E(n): samples a stream that goes on has emitted: hop j needs knot j + 1, ``n >= (j + 5) hop``"""
    return int(hop) * max(0, int(n) // int(hop) - 4)


def loudness_piece_len(block: int, n_before: int, length: int, last: bool) -> Tuple[int, int, int]:
    """(piece length, n after, knots made after) of one push -- the twin of ``smi_louds_piece_len``: a stream goes on with
    ``loudness_emitted(n)`` samples out and ``loudness_knots(n)`` knots; a finished one has emitted all its L samples and has
    the knots 0 .. floor((L - 1) / hop) + 1 (none at L = 0).  ValueError for a bad argument."""
    block, n_before, length = int(block), int(n_before), int(length)
    if block < 4 or block % 4:
        raise ValueError(f"block={block} must be a positive multiple of 4")
    if n_before < 0 or length < 0:
        raise ValueError("negative counter or length")
    hop = block // 4
    n = n_before + length
    if last:
        return n - loudness_emitted(n_before, hop), n, ((n - 1) // hop + 2 if n else 0)
    return loudness_emitted(n, hop) - loudness_emitted(n_before, hop), n, loudness_knots(n, hop)


# ---- limiter of joined streams (include/sparkmi.h, smi_limits_*): what a push emits, as host arithmetic
LIMITER_HALO = 10      # samples the true-peak interpolator reaches on either side


def limiter_emitted(n: int, lookahead: int, release: int) -> int:
    """E(n): samples a stream that goes on has emitted: sample i reads its input up to ``i + A + R + 10``, in both modes"""
    return max(0, int(n) - (int(lookahead) + int(release) + LIMITER_HALO))


def limiter_piece_len(lookahead: int, release: int, n_before: int, length: int, last: bool) -> Tuple[int, int]:
    """(piece length, n after) of one push -- the twin of ``smi_limits_piece_len``: a stream goes on with ``limiter_emitted(n)``
    samples out; a finished one has emitted all its L samples.  ValueError for a bad argument."""
    A, R, n_before, length = int(lookahead), int(release), int(n_before), int(length)
    if not 0 <= A <= 256 or not 0 <= R <= 2048:
        raise ValueError(f"lookahead={A} outside 0..256 or release={R} outside 0..2048")
    if n_before < 0 or length < 0:
        raise ValueError("negative counter or length")
    n = n_before + length
    return (n if last else limiter_emitted(n, A, R)) - limiter_emitted(n_before, A, R), n


def stream_chunks(token_iter:Iterator[Sequence[int]], scheduler: ChunkScheduler) -> Iterator[List[int]]:
    """Token increments in, ready chunks out (the generator form of the reference loop)."""
    for inc in token_iter:
        if inc is None or len(inc) == 0:
            break
        for c in scheduler.push(inc):
            yield c
    for c in scheduler.flush():
        yield c


class _Stream:
    """One request of a ``StreamMux``."""

    def __init__(self, sched: ChunkScheduler, global_ids: Optional[List[int]]):
        self.sched = sched
        self.given = global_ids is not None          # clone mode: the request brought its global ids
        self.glob: List[int] = list(global_ids) if global_ids is not None else []
        self.ids: List[int] = []                     # every generated id so far (the whole-history parser needs them)
        self.tables = True                           # still on the id tables (no ordinary text id seen)
        self.n_sem = 0                               # semantic tokens handed to the scheduler
        self.held: List[List[int]] = []              # ready chunks waiting for the speaker tokens
        self.index = 0                               # chunks released so far
        self.finished = False


class StreamMux:
    """Chunked vocoding for many concurrent requests, host side only (no GPU, no torch): per request key an incremental token
    parser, the speaker-token gate and a ``ChunkScheduler``.

    ``tables``: an object with ``sem`` / ``glob`` (id -> bicodec index), ``special`` (ids to skip) and ``usable``
    (``pipeline._TokenMap``), or None; ``parse``: a callable ids -> (semantic ids, global ids) over a request's WHOLE history
    (``SparkTTS._parse``), or None.  While every id of a request is in the tables it is parsed id by id; the first id that is
    not (an ordinary text token) moves that request to ``parse`` for good, as ``_TokenMap.fast_parse`` falls back.  One of the
    two must be given.

    The gate: a clone request brings its global ids (``open(key, global_ids)``) and its chunks are released as they become
    ready; a control-mode request (no global ids) must first have GENERATED ``spk_token_num`` of them -- its ready chunks wait
    until then and are released in order, as ``inference_stream`` does.  ``global_ids(key)`` is what a released chunk is
    vocoded with."""

    def __init__(self, spk_token_num: int, tables=None, parse: Optional[Callable] = None, *, frame_rate: int = 50,
                 audio_chunk_duration: float = 1.0, max_audio_chunk_duration: float = 30.0,
                 audio_chunk_size_scale_factor: float = 8.0, audio_chunk_overlap_duration: float = 0.1):
        if tables is not None and not getattr(tables, "usable", True):
            tables = None
        if tables is None and parse is None:
            raise ValueError("StreamMux needs id tables or a parse callable")
        self.ntok = int(spk_token_num)
        self._tables, self._parse = tables, parse
        self._sched_args = (audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor,
                            audio_chunk_overlap_duration, frame_rate)
        ChunkScheduler(*self._sched_args)   # the argument checks, once, before any request
        self._streams: Dict[Hashable, _Stream] = {}

    def open(self, key: Hashable, global_ids: Optional[Sequence[int]] = None) -> None:
        """A new request; ``global_ids``: the speaker tokens a clone request brings (None: they will be generated)."""
        if key in self._streams:
            raise ValueError(f"request {key}: already open")
        g = None if global_ids is None else [int(t) for t in global_ids]
        self._streams[key] = _Stream(ChunkScheduler(*self._sched_args), g)

    def global_ids(self, key: Hashable) -> Optional[List[int]]:
        """The speaker tokens of an open request, or None while a control-mode request has not generated them all."""
        st = self._streams[key]
        if st.given:
            return st.glob
        return st.glob[: self.ntok] if len(st.glob) >= self.ntok else None

    def _feed(self, st: _Stream, new_ids: Sequence[int]) -> List[int]:
        """The semantic tokens ``new_ids`` add; generated global tokens go to the gate."""
        st.ids.extend(int(t) for t in new_ids)
        if st.tables and self._tables is not None:
            sem, glob = [], []
            for t in new_ids:
                t = int(t)
                if t in self._tables.sem:
                    sem.append(self._tables.sem[t])
                elif t in self._tables.glob:
                    glob.append(self._tables.glob[t])
                elif t not in self._tables.special:
                    if self._parse is None:
                        raise ValueError(f"id {t} is neither a bicodec token nor a special token, and no parse callable was given")
                    st.tables = False
                    break
            if st.tables:
                if not st.given:
                    st.glob.extend(glob)
                st.n_sem += len(sem)
                return sem
        st.tables = False
        sem, glob = self._parse(st.ids)
        new = [int(t) for t in sem[st.n_sem:]]
        st.n_sem = len(sem)
        if not st.given:
            st.glob = [int(t) for t in glob]
        return new

    def push(self, key: Hashable, new_ids: Sequence[int], finished: bool) -> List[Tuple[Hashable, int, List[int], bool]]:
        """The ids ``key`` has generated since its last push (``finished``: there will be no more) -> the chunks that are
        ready now, ``[(key, chunk_index, semantic ids, last)]`` in order.  Whatever the granularity of the pushes, a request's
        chunks are those of one ``ChunkScheduler`` fed its semantic ids in one go; ``last`` is on exactly one chunk, the final
        one.  (A request that ends exactly on a chunk boundary with a zero overlap, in a push after the one that released that
        chunk, has nothing left to flush: it ends with an empty chunk that carries the flag.)  A request not opened yet is
        opened here as a control-mode one."""
        if key not in self._streams:
            self.open(key)
        st = self._streams[key]
        if st.finished:
            raise ValueError(f"request {key}: push after its last one")
        ready = st.sched.push(self._feed(st, new_ids))
        if finished:
            st.finished = True
            ready += st.sched.flush()
        st.held += ready
        if self.global_ids(key) is None:
            return []                      # control mode: the speaker tokens come first; close() reports their absence
        out = []
        for chunk in st.held:
            out.append((key, st.index, chunk, False))
            st.index += 1
        st.held = []
        if finished and st.n_sem > 0:
            if not out:
                out.append((key, st.index, [], True))
                st.index += 1
            else:
                out[-1] = out[-1][:3] + (True,)
        return out

    def close(self, key: Hashable) -> None:
        """The end of a request: forgets it, and raises the ``ValueError`` that ``SparkTTS.serve`` raises for a request that
        generated no semantic token or has a wrong number of global tokens."""
        st = self._streams.pop(key)
        if len(st.glob) != self.ntok:
            raise ValueError(f"request {key}: {len(st.glob)} global tokens, the speaker encoder needs {self.ntok}")
        if st.n_sem == 0:
            raise ValueError(f"request {key}: the model generated no semantic tokens")


class Pacer:
    """Which open requests of a ``serve_stream`` loop run, host side only (no GPU, no torch).  The engine produces a request's
    audio many times faster than a listener hears it, so a request that is far enough ahead of its listener can give its decode
    row to one that is waiting: it is *parked* (its sequence leaves its KV slot as a snapshot, ``SparkLLM.park``) and *resumed*
    later (``SparkLLM.restore_slots``), and more requests can be open than there are rows.

    ``max_batch``: decode rows.  ``max_open``: requests that may be open (admitted and not finished) at once; None or a value
    <= ``max_batch``: the pacer is inert.  ``max_ahead`` (seconds; None: inert): a request may be parked once its lead exceeds
    it.  ``resume_ahead`` (seconds, default ``max_ahead / 2``): a parked request whose lead has fallen below it is resumed before
    anything else gets a row.  ``clock``: a callable returning seconds (default ``time.monotonic``).

    A request's *lead* is the audio yielded for it so far (``yielded``), in seconds, minus the clock time since its first chunk
    was yielded; before its first chunk it is minus infinity, so a request that has not spoken yet is never parked.

    Every decision is a pure function of the calls made and the clock; ties break by request key (the request index).
      ``to_park(live, parked, pending)``: the live, unfinished requests to park now.  A request qualifies only if its lead
        exceeds ``max_ahead`` and somebody is waiting -- a pending request while fewer than ``max_open`` are open, or a parked
        request.  Of those that qualify, only as many are parked as there are waiters that the free rows cannot serve (a row
        is never emptied to be handed straight back), largest lead first.
      ``to_resume(parked, free_rows, urgent)``: the parked requests that get ``free_rows`` rows, smallest lead first;
        ``urgent=True``: only those whose lead has fallen below ``resume_ahead``.  Rows go to (1) the urgent ones, (2) pending
        requests, (3) any parked request -- the caller asks with ``urgent=True``, admits, then asks with ``urgent=False``, so
        no row idles while a parked request exists.
    ``parks`` / ``resumes`` count the requests ``to_park`` / ``to_resume`` have named."""

    def __init__(self, max_batch: int, max_open: Optional[int] = None, max_ahead: Optional[float] = None,
                 resume_ahead: Optional[float] = None, frame_rate: int = 50, clock: Optional[Callable[[], float]] = None):
        import time
        self.max_batch = int(max_batch)
        self.max_open = self.max_batch if max_open is None else int(max_open)
        self.max_ahead = None if max_ahead is None else float(max_ahead)
        if self.max_batch < 1 or self.max_open < 1:
            raise ValueError("Pacer: max_batch and max_open must be >= 1")
        if self.max_ahead is not None and not self.max_ahead > 0:
            raise ValueError("Pacer: max_ahead must be > 0")
        if resume_ahead is None:
            resume_ahead = None if self.max_ahead is None else self.max_ahead / 2
        elif self.max_ahead is not None and not 0 <= float(resume_ahead) <= self.max_ahead:
            raise ValueError("Pacer: 0 <= resume_ahead <= max_ahead")
        self.resume_ahead = None if resume_ahead is None else float(resume_ahead)
        self.frame_rate = float(frame_rate)
        self.clock = clock if clock is not None else time.monotonic
        self.active = self.max_ahead is not None and self.max_open > self.max_batch
        self._first: Dict[Hashable, float] = {}    # key -> clock at its first chunk
        self._frames: Dict[Hashable, int] = {}     # key -> frames yielded
        self.parks = 0
        self.resumes = 0

    def yielded(self, key: Hashable, frames: int, seconds: Optional[float] = None) -> None:
        """A chunk of ``frames`` new audio frames of request ``key`` has just been handed to its listener.  ``seconds``: the
        audio the listener actually received, where that is not ``frames / frame_rate`` (a piece at a tempo); it is counted in
        place of the frames."""
        if key not in self._first:
            self._first[key] = self.clock()
            self._frames[key] = 0
        self._frames[key] += int(frames) if seconds is None else float(seconds) * self.frame_rate

    def close(self, key: Hashable) -> None:
        self._first.pop(key, None)
        self._frames.pop(key, None)

    def lead(self, key: Hashable, now: Optional[float] = None) -> float:
        if key not in self._first:
            return -math.inf
        now = self.clock() if now is None else now
        return self._frames[key] / self.frame_rate - (now - self._first[key])

    def to_park(self, live: Sequence[Hashable], parked: Sequence[Hashable], pending: bool) -> List[Hashable]:
        if not self.active:
            return []
        n_open = len(live) + len(parked)
        waiters = len(parked) + (1 if pending and n_open < self.max_open else 0)
        want = waiters - (self.max_batch - len(live))
        if want <= 0:
            return []
        now = self.clock()
        cands = sorted((-self.lead(k, now), k) for k in live if self.lead(k, now) > self.max_ahead)
        out = [k for _, k in cands[:want]]
        self.parks += len(out)
        return out

    def to_resume(self, parked: Sequence[Hashable], free_rows: int, urgent: bool) -> List[Hashable]:
        if free_rows <= 0 or not parked:
            return []
        now = self.clock()
        cands = sorted((self.lead(k, now), k) for k in parked)
        if urgent:
            cands = [c for c in cands if c[0] < self.resume_ahead]
        out = [k for _, k in cands[:free_rows]]
        self.resumes += len(out)
        return out
