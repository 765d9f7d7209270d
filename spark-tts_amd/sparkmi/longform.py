"""Long text, sentence by sentence (``SparkTTS.inference_long``): the text splitter and the per-sentence plan -- seeds, and the
continuation that keeps a created voice the same from sentence to sentence.  Host-side logic only: no tensors, no device.

The generator was trained on short utterances and drifts or loops on long ones, and an utterance's speech budget is bounded by
``max_positions`` and ``max_frames``.  A paragraph is therefore cut into sentences, which run as the independent rows of one
in-flight session; their waveforms are trimmed and joined on the device (include/sparkmi.h, smi_trim_rows / smi_concat_rows)."""
from __future__ import annotations

import re
import unicodedata
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from .pipeline_text import build_control_prompt

STOPS = ".!?;…"                       # end a sentence when whitespace or the end of the text follows
WIDE_STOPS = "。！？；…"   # end a sentence wherever they stand
CLOSERS = "\"'”’)]}»」』）】》"   # stay with the sentence they close
CUTS = ",;:，、；："      # where an over-wide piece is cut first
_PARAGRAPH = re.compile(r"\n[^\S\n]*\n\s*")


def char_width(c: str) -> int:
    """3 for an East-Asian wide or full-width character (roughly a syllable), 1 otherwise (a Latin letter: a third of one)"""
    return 3 if unicodedata.east_asian_width(c) in ("W", "F") else 1


def width(s: str) -> int:
    return sum(char_width(c) for c in s)


def _sentences(text: str) -> List[str]:
    """``text`` cut behind every sentence end and at every paragraph break; pieces stripped, empty ones dropped"""
    cuts, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c == "\n":
            m = _PARAGRAPH.match(text, i)
            if m:
                cuts.append(i)
                i = m.end()
                continue
        if c in STOPS or c in WIDE_STOPS:
            if c == "." and 0 < i < n - 1 and text[i - 1].isdigit() and text[i + 1].isdigit():   # "3.14"
                i += 1
                continue
            j, wide = i, False
            while j < n and (text[j] in STOPS or text[j] in WIDE_STOPS):
                wide = wide or text[j] in WIDE_STOPS
                j += 1
            while j < n and text[j] in CLOSERS:
                j += 1
            if wide or j == n or text[j].isspace():
                cuts.append(j)
            i = j
            continue
        i += 1
    out, a = [], 0
    for b in cuts + [n]:
        p = text[a:b].strip()
        if p:
            out.append(p)
        a = b
    return out


def _cut(piece: str, max_width: int) -> List[str]:
    """``piece`` (stripped) in parts no wider than ``max_width``: cut after the last of ``CUTS`` inside the limit, else at the
    last whitespace there, else hard at the limit"""
    out = []
    while width(piece) > max_width:
        j, w = 0, 0
        while w + char_width(piece[j]) <= max_width:   # piece[:j] is the longest prefix inside the limit; 1 <= j < len(piece)
            w += char_width(piece[j])
            j += 1
        at = max((piece.rfind(c, 0, j) for c in CUTS), default=-1) + 1
        if at < 1:
            at = next((q for q in range(j, 0, -1) if piece[q].isspace()), j)
        out.append(piece[:at].strip())
        piece = piece[at:].strip()
    if piece:
        out.append(piece)
    return out


def _join(a: str, b: str) -> str:
    """two pieces as one: a space between them unless a wide character stands at the seam"""
    return a + ("" if char_width(a[-1]) == 3 or char_width(b[0]) == 3 else " ") + b


def split_text(text: str, max_width: int = 300, min_width: int = 20) -> List[str]:
    """``text`` as the sentences ``inference_long`` generates one by one.

    A sentence ends after a run of ``. ! ? ; ...`` (the ellipsis character) that whitespace or the end of the text follows,
    after a run holding one of the full-width stops (or the ellipsis character), whatever follows, and at a paragraph break (a
    newline run with an empty line); closing quotes and brackets behind the run stay with the sentence, and a ``.`` between
    two digits ends nothing.  A piece wider than ``max_width`` (``width``: 3 per East-Asian wide character, 1 per other) is cut
    -- after its last ``, ; :`` (or their full-width forms) inside the limit, else at the last whitespace there, else hard at the
    limit --, then a piece narrower than ``min_width`` is merged into the following one (the last piece: into the previous
    one) where the two together stay within ``max_width``.  The pieces are non-empty, carry no whitespace at their edges, hold
    every non-whitespace character of ``text`` exactly once and in order, and none is wider than ``max_width``.
    ValueError: empty or whitespace-only text, ``max_width`` below 3 (one wide character) or below ``min_width``."""
    for name, v in (("max_width", max_width), ("min_width", min_width)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, not {v!r}")
    if max_width < 3 or min_width < 0 or max_width < min_width:
        raise ValueError(f"max_width={max_width} must be at least 3 and at least min_width={min_width} >= 0")
    if not isinstance(text, str) or not text.strip():
        raise ValueError("text is empty")
    pieces = [p for s in _sentences(text) for p in _cut(s, max_width)]
    i = 0
    while i < len(pieces):
        if width(pieces[i]) < min_width:
            if i + 1 < len(pieces):
                both = _join(pieces[i], pieces[i + 1])
                if width(both) <= max_width:
                    pieces[i: i + 2] = [both]
                    continue          # (the merged piece may still be narrow: it is looked at again)
            elif i > 0:
                both = _join(pieces[i - 1], pieces[i])
                if width(both) <= max_width:
                    pieces[i - 1: i + 1] = [both]
                    continue
        i += 1
    return pieces


def sentence_seeds(seed: Optional[int], n: int) -> List[Optional[int]]:
    """sentence k carries ``seed + k`` (the convention of ``num_return_sequences``); None: the handle's key, for every sentence"""
    if seed is None:
        return [None] * n
    if isinstance(seed, bool) or int(seed) != seed:
        raise ValueError(f"seed must be an int or None, not {seed!r}")
    return [int(seed) + k for k in range(n)]


def control_prefix(new_ids: Sequence[int], sem_ids, glob_ids: Dict[int, int], ntok: int) -> Tuple[List[int], List[int]]:
    """What sentence 0 of a created voice decided for all later ones: (the ids it generated before its first semantic id -- the
    style values and the global-token block --, that block's ``ntok`` global token values).  ``sem_ids``: the ids of the
    semantic tokens (a container); ``glob_ids``: id -> value of the global tokens.  ValueError, in ``inference_batch``'s words,
    unless the block is complete."""
    cut = next((j for j, t in enumerate(new_ids) if t in sem_ids), len(new_ids))
    prefix = [int(t) for t in new_ids[:cut]]
    glob = [glob_ids[t] for t in prefix if t in glob_ids]
    if len(glob) != ntok:
        raise ValueError(f"request 0: {len(glob)} global tokens generated, the speaker encoder needs {ntok}")
    return prefix, glob


def control_prompt_ids(tokenize: Callable[[str], List[int]], gender: str, pitch: str, speed: str, sentence: str,
                       prefix: Sequence[int] = ()) -> List[int]:
    """The prompt ids of one sentence of a created voice: its control prompt, then ``prefix`` (``control_prefix``; empty for
    sentence 0), so that the sentence continues from sentence 0's style and speaker tokens and generates semantic tokens only"""
    return list(tokenize(build_control_prompt(gender, pitch, speed, sentence))) + [int(t) for t in prefix]


def trim_params(sample_rate: int) -> Tuple[int, int, int]:
    """(window, step, margin) as ``remove_silence_on_both_ends`` passes them: int(0.1 sr), window // 10, 2 window"""
    window = int(0.1 * int(sample_rate))
    return window, window // 10, 2 * window


def ready_run(done, first: int, limit: int) -> List[int]:
    """the sentences ``first``, ``first + 1``, ... that are all in ``done``, at most ``limit`` of them"""
    run = []
    while len(run) < limit and first + len(run) in done:
        run.append(first + len(run))
    return run
