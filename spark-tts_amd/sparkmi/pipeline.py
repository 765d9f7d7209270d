"""SparkTTS -- drop-in for the reference pipeline class (``cli/SparkTTS.py``) on one MI355X.

Same constructor and ``inference()`` signature, same attributes (``device``, ``model_dir``,
``configs``, ``sample_rate``, ``tokenizer``, ``model``, ``audio_tokenizer``), same prompt
strings, same token parsing, same float32 numpy waveform.  The two heavy calls run on the HIP
kernels: ``self.model.generate`` (``SparkLLM``) and ``self.audio_tokenizer.detokenize``
(``BiCodecTokenizer``).  Keyword-only additions: ``do_sample``, ``max_new_tokens``,
``prompt_tokens`` (pre-computed prompt audio tokens), ``inference_batch``,
``inference_stream`` (chunked vocoding while the LLM generates, the reference's decoupled Triton mode), ``serve`` (in-flight
batching) and ``serve_stream`` (both at once: chunked audio for every live request of an in-flight batch); the two streaming
calls take ``joined=True`` for contiguous, playable pieces at any output rate (the chunks joined on the device);
``inference_long`` / ``inference_long_stream`` (text of any length: sentences as the rows of one in-flight session, their
waveforms trimmed and joined on the device); ``loudness`` / ``peak_ceiling`` / ``max_gain_db`` on every call that returns whole
utterances (the output at a programme loudness after BS.1770, measured and scaled on the device); ``tempo`` on the same calls
(a pitch-preserving change of the speaking rate, 0.5 .. 2.0, on the device before the loudness stage) and, with
``joined=True``, on the two streaming calls (the same arithmetic with its state carried across the chunks on the device);
``limiter`` on the calls that return whole utterances (a look-ahead true-peak limiter behind the loudness stage, on the device)
and ``stream_limiter``, with ``joined=True``, on the two streaming calls (the same limiter with its input carried across the chunks);
``pitch_shift`` on the calls that return whole utterances (semitones for any voice, in the tempo stage's place: one stretch pass
serves both, a resampler follows inside the same launch; the streaming calls refuse it) and ``stream_pitch_shift``, with
``joined=True``, on the two streaming calls (the same arithmetic with the stretch's state and the resampler's tail carried across
the chunks, in the tempo stream's place).
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .audio import LIMITER_MODES, PEAK_CEILING, check_limiter, check_loudness, pitch_ratio, tempo_len, tempo_ratio
from .bicodec import BiCodecTokenizer
from .config import LLMConfig, TopConfig
from .llm import (ALLOW_KEY, FORK_KEY, LOGPROB_KEYS, NGRAM_KEY, PENALTY_KEYS, SAMPLING_KEYS, SEQ_KEYS, SparkLLM,
                  eos_ids_from_generation_config, ngram_size, num_returns, penalty_neutral, seq_entries)
from .pipeline_text import (GENDER_MAP, LEVELS_MAP, TASK_TOKEN_MAP, build_clone_prompt,
                            build_control_prompt, parse_global, parse_semantic)
from .streaming import ChunkScheduler, Pacer, StreamMux
from .weights import load_llm_state


# request key: generate only the ids of the tokenizer's added vocabulary (the <|bicodec_*|> and control tokens) and eos
SPEECH_ONLY_KEY = "speech_tokens_only"


# request key: a bias on the end token -- sugar for one length-1 ``sequence_bias`` entry per eos id of the session (-inf: the
# request runs to its token budget; a large positive value: it ends at the first token min_new_tokens lets it)
EOS_BIAS_KEY = "eos_bias"


# request key: the programme loudness (LUFS) the request's waveform is brought to; it overrides the call's ``loudness``
LOUDNESS_KEY = "loudness"


class StreamLoudnessRefused(ValueError, TypeError):
    """``loudness`` on a chunked stream with overlapping chunks.  A ValueError like the refusals of ``tempo`` and
    ``output_sample_rate`` there; a TypeError too, because before the calls knew the keyword that is what passing it raised, and a
    caller that catches that keeps working."""


LIMITED = (None, "max_gain", "ceiling")   # what bounded a row's gain (include/sparkmi.h, smi_loud_rows: limit 0 / 1 / 2)
# request key: the request's own limiter ("true", "sample" or None); it overrides the call's ``limiter``
LIMITER_KEY = "limiter"
# the ceiling the loudness stage is given where the limiter holds ``peak_ceiling`` behind it: large and finite, it cannot bind
NO_CEILING = 1e30
# request key: the request's own streaming limiter ("true", "sample" or None) in ``serve_stream(joined=True)``; it overrides the
# call's ``stream_limiter``
STREAM_LIMITER_KEY = "stream_limiter"
# request key: the request's own tempo (0.5 .. 2.0; > 1: faster); it overrides the call's ``tempo``
TEMPO_KEY = "tempo"
# request key: the request's own pitch shift in semitones (-12.0 .. 12.0; > 0: higher); it overrides the call's ``pitch_shift``
# (``pitch`` is taken: the label argument of voice creation)
PITCH_SHIFT_KEY = "pitch_shift"
# request key of serve_stream(joined=True): the request's own pitch shift on the stream, in semitones; it overrides the call's
# ``stream_pitch_shift``
STREAM_PITCH_SHIFT_KEY = "stream_pitch_shift"


def _stream_pacing(max_batch: int, max_open=None, max_ahead=None, resume_ahead=None):
    """``serve_stream``'s pacing keywords, checked before anything reaches the device: (max_open, max_ahead, resume_ahead) with
    the defaults filled in.  ``max_open``: an int >= 1 (None: ``max_batch``); ``max_ahead`` > 0 seconds (None: no parking);
    0 <= ``resume_ahead`` <= ``max_ahead`` (None: ``max_ahead / 2``).  ``max_ahead`` without ``max_open > max_batch`` is
    accepted and inert."""
    if max_open is None:
        max_open = int(max_batch)
    elif isinstance(max_open, bool) or not isinstance(max_open, (int, np.integer)) or max_open < 1:
        raise ValueError(f"max_open must be an int >= 1, not {max_open!r}")
    for name, v in (("max_ahead", max_ahead), ("resume_ahead", resume_ahead)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number of seconds, not {v!r}")
    if max_ahead is not None and not max_ahead > 0:
        raise ValueError(f"max_ahead must be > 0, not {max_ahead!r}")
    if resume_ahead is not None:
        if resume_ahead < 0 or (max_ahead is not None and resume_ahead > max_ahead):
            raise ValueError(f"resume_ahead must lie in [0, max_ahead], not {resume_ahead!r}")
    elif max_ahead is not None:
        resume_ahead = max_ahead / 2
    return int(max_open), None if max_ahead is None else float(max_ahead), None if resume_ahead is None else float(resume_ahead)


def _request_seq(r: dict, eos: Sequence[int], vocab_size: int, what: str = "request") -> dict:
    """The ``sequence_bias`` / ``bad_words_ids`` / ``stop_sequences`` keys (``SEQ_KEYS``) a request dict carries, as lists, with
    ``eos_bias`` folded into ``sequence_bias``; checked (``seq_entries``: ValueError before anything reaches the device)."""
    d = {}
    for k in SEQ_KEYS:
        if r.get(k) is not None:
            v = r[k]
            if isinstance(v, (str, bytes, dict)) or not hasattr(v, "__iter__"):
                raise ValueError(f"{what}: {k} must be a list, not {v!r}")
            d[k] = list(v)
    if r.get(EOS_BIAS_KEY) is not None:
        b = r[EOS_BIAS_KEY]
        if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, float, np.integer, np.floating)) or np.isnan(b) or b == np.inf:
            raise ValueError(f"{what}: {EOS_BIAS_KEY} must be a finite number or -inf, not {b!r}")
        if not eos:
            raise ValueError(f"{what}: {EOS_BIAS_KEY} needs an eos id, the model has none")
        d["sequence_bias"] = list(d.get("sequence_bias", [])) + [((int(e),), float(b)) for e in dict.fromkeys(int(e) for e in eos)]
    if d:
        seq_entries(d, vocab_size, what)
    return d


def _request_sampling(r: dict, speech_ids=None, eos: Sequence[int] = (), vocab_size: Optional[int] = None) -> Optional[dict]:
    """The sampling keys (``SAMPLING_KEYS``) and penalty keys (``PENALTY_KEYS``) a request dict carries, or None: the
    call-level arguments apply unchanged.  Penalty keys that ask for no penalty are dropped, so such a request keeps the
    route (and the bits) of the same request without them.  ``return_log_probs`` (``LOGPROB_KEYS``) is kept when True.
    ``allowed_token_ids`` (``ALLOW_KEY``) and ``speech_tokens_only`` (``SPEECH_ONLY_KEY``: True -> ``speech_ids()``) become
    the request's allowed-token set (both given: their intersection); include/sparkmi.h, smi_llm_admit_constrained.
    With ``vocab_size`` given, ``sequence_bias`` / ``bad_words_ids`` / ``stop_sequences`` (``SEQ_KEYS``) and ``eos_bias``
    (``EOS_BIAS_KEY``, over the eos ids ``eos``) are checked and carried too (``_request_seq``; smi_llm_admit_biased).
    ``no_repeat_ngram_size`` (``NGRAM_KEY``) is checked (``ngram_size``: an int in 0 .. SMI_MAX_NGRAM, not a bool) and kept when
    it is > 0 (smi_llm_admit_ngram); 0 is dropped, so such a request keeps the route of the request without the key."""
    d = {k: r[k] for k in SAMPLING_KEYS if k in r}
    speech = r.get(SPEECH_ONLY_KEY, False)
    if not isinstance(speech, (bool, np.bool_)):
        raise ValueError(f"{SPEECH_ONLY_KEY} must be a bool, not {speech!r}")
    allowed = r.get(ALLOW_KEY)
    if allowed is not None or speech:
        s = None if allowed is None else tuple(allowed)
        if speech:
            sp = speech_ids()
            s = tuple(sp) if s is None else tuple(sorted(set(s) & set(sp)))
        d[ALLOW_KEY] = s
    pen = {k: r[k] for k in PENALTY_KEYS if k in r}
    if not penalty_neutral(pen):
        d.update(pen)
    for k in LOGPROB_KEYS:
        if k in r and not isinstance(r[k], (bool, np.bool_)):
            raise ValueError(f"{k} must be a bool, not {r[k]!r}")
        if r.get(k):
            d[k] = True
    if r.get(NGRAM_KEY) is not None and ngram_size(r[NGRAM_KEY]) > 0:
        d[NGRAM_KEY] = ngram_size(r[NGRAM_KEY])
    if vocab_size is not None:
        d.update(_request_seq(r, eos, vocab_size))
    return d or None


def _take_counts(requests: Sequence[dict], max_batch: int) -> Optional[List[int]]:
    """The ``num_return_sequences`` of every request (1 where a request leaves the key out), or None when no request carries
    it (today's route).  Checked before any device call: each an int >= 1 (a bool is refused), all takes together at most
    ``max_batch``."""
    if not any(FORK_KEY in r for r in requests):
        return None
    n = [num_returns(r[FORK_KEY], f"request {i}: {FORK_KEY}") if FORK_KEY in r else 1 for i, r in enumerate(requests)]
    if sum(n) > max_batch:
        raise ValueError(f"{sum(n)} takes (num_return_sequences) > max_batch={max_batch}")
    return n


def _lp_info(toks: Sequence[int], lps: np.ndarray) -> dict:
    """The info dict that comes with a waveform when log-probabilities are asked for."""
    lps = np.asarray(lps, dtype=np.float32)
    return {"token_ids": list(toks), "output_log_probs": lps, "cum_log_prob": float(np.sum(lps, dtype=np.float64))}


class _TokenMap:
    """id -> bicodec index tables read from the tokenizer's own vocabulary, used to skip the
    decode + regex round trip of ``cli/SparkTTS.py:213-228`` when it provably gives the same
    answer (every generated id is either a bicodec token or a special token)."""

    def __init__(self, tokenizer):
        import re
        self.sem: Dict[int, int] = {}
        self.glob: Dict[int, int] = {}
        rs, rg = re.compile(r"^<\|bicodec_semantic_(\d+)\|>$"), re.compile(r"^<\|bicodec_global_(\d+)\|>$")
        for tok, idx in tokenizer.get_vocab().items():
            m = rs.match(tok)
            if m:
                self.sem[idx] = int(m.group(1))
                continue
            m = rg.match(tok)
            if m:
                self.glob[idx] = int(m.group(1))
        self.special = set(int(i) for i in getattr(tokenizer, "all_special_ids", []) or [])
        # The reference decodes with skip_special_tokens=True (cli/SparkTTS.py:213): a bicodec token that a tokenizer lists
        # as SPECIAL would be dropped there before the regex sees it.  The id tables cannot reproduce that, so such a
        # tokenizer always takes the reference's decode + regex route.
        self.usable = not (self.special & (set(self.sem) | set(self.glob)))

    def fast_parse(self, ids: Sequence[int]) -> Optional[Tuple[List[int], List[int]]]:
        if not self.usable:
            return None
        sem, glob = [], []
        for i in ids:
            if i in self.sem:
                sem.append(self.sem[i])
            elif i in self.glob:
                glob.append(self.glob[i])
            elif i not in self.special:
                return None   # ordinary text token: fall back to the reference's decode + regex
        return sem, glob


class SparkTTS:
    """Spark-TTS for text-to-speech generation (MI355X-native hot path)."""

    def __init__(self, model_dir: Path, device: torch.device = torch.device("cuda:0"), *,
                 max_batch: int = 1, max_positions: int = 4096, kv_dtype: str = "bf16",
                 max_frames: int = 3000):
        self.device = torch.device(device)
        self.model_dir = model_dir
        top = TopConfig.from_yaml(Path(model_dir) / "config.yaml")
        self.configs = {"sample_rate": top.sample_rate, "ref_segment_duration": top.ref_segment_duration,
                        "latent_hop_length": top.latent_hop_length, "volume_normalize": top.volume_normalize}
        self.sample_rate = self.configs["sample_rate"]
        self._max_batch, self._max_positions, self._kv_dtype, self._max_frames = max_batch, max_positions, kv_dtype, max_frames
        self._initialize_inference()

    def _initialize_inference(self):
        """Tokenizer (HF, host side), LLM and audio tokenizer (both on the HIP kernels)."""
        from transformers import AutoTokenizer
        llm_dir = Path(self.model_dir) / "LLM"
        self.tokenizer = AutoTokenizer.from_pretrained(str(llm_dir))
        cfg = LLMConfig.from_json(llm_dir / "config.json")
        # HF generate() as the reference calls it (no eos argument, cli/SparkTTS.py:197-204) stops on EVERY id of
        # generation_config.json's eos_token_id; all of them go down to the step kernel
        self._eos = eos_ids_from_generation_config(llm_dir, cfg)
        if not self._eos and self.tokenizer.eos_token_id is not None:
            self._eos = [int(self.tokenizer.eos_token_id)]
        self.model = SparkLLM(cfg, load_llm_state(llm_dir), self.device, max_slots=self._max_batch,
                              max_positions=self._max_positions, kv_dtype=self._kv_dtype, eos_token_ids=self._eos)
        self.audio_tokenizer = BiCodecTokenizer(self.model_dir, device=self.device, max_batch=self._max_batch,
                                                max_frames=self._max_frames)
        self._map = _TokenMap(self.tokenizer)

    # ------------------------------------------------------------------ prompts
    def process_prompt(self, text: str, prompt_speech_path: Path, prompt_text: str = None,
                       prompt_tokens: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[str, torch.Tensor]:
        """Voice-cloning prompt.  Returns (prompt string, global token ids (1, 1, Ntok))."""
        if prompt_tokens is not None:
            global_token_ids, semantic_token_ids = prompt_tokens
        else:
            global_token_ids, semantic_token_ids = self.audio_tokenizer.tokenize(prompt_speech_path)
        global_token_ids = torch.as_tensor(global_token_ids)
        semantic_token_ids = torch.as_tensor(semantic_token_ids)
        inputs = build_clone_prompt(text, global_token_ids.reshape(-1).tolist(),
                                    semantic_token_ids.reshape(-1).tolist(), prompt_text)
        return inputs, global_token_ids

    def process_prompt_control(self, gender: str, pitch: str, speed: str, text: str):
        """Voice-creation prompt (gender: female | male; pitch/speed: very_low .. very_high)."""
        return build_control_prompt(gender, pitch, speed, text)

    # ------------------------------------------------------------------ inference
    def _parse(self, new_ids: Sequence[int]) -> Tuple[List[int], List[int]]:
        fast = self._map.fast_parse(new_ids)
        if fast is not None:
            return fast
        predicts = self.tokenizer.batch_decode([list(new_ids)], skip_special_tokens=True)[0]
        return parse_semantic(predicts), parse_global(predicts)

    def speech_token_ids(self) -> List[int]:
        """The ids a ``speech_tokens_only`` request may generate: the tokenizer's added vocabulary (the ``<|bicodec_*|>``
        and control tokens) and every eos id of the session; the ordinary BPE text ids are left out."""
        if getattr(self, "_speech_ids", None) is None:
            self._speech_ids = sorted(set(int(i) for i in self.tokenizer.get_added_vocab().values()) | set(self._eos))
        return self._speech_ids

    @torch.no_grad()
    def inference(self, text: str, prompt_speech_path: Path = None, prompt_text: str = None,
                  gender: str = None, pitch: str = None, speed: str = None,
                  temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *,
                  do_sample: bool = True, max_new_tokens: int = 3000, seed: Optional[int] = None,
                  prompt_tokens: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                  min_new_tokens: int = 0, penalize_prompt: bool = True, return_log_probs: bool = False,
                  num_return_sequences: int = 1, allowed_token_ids: Optional[Sequence[int]] = None,
                  speech_tokens_only: bool = False, no_repeat_ngram_size: int = 0, output_sample_rate: Optional[int] = None,
                  loudness: Optional[float] = None, peak_ceiling: float = PEAK_CEILING, max_gain_db: float = 20.0,
                  tempo: Optional[float] = None, limiter: Optional[str] = None, limiter_lookahead_ms: float = 2.5,
                  limiter_release_ms: float = 25.0, pitch_shift: Optional[float] = None):
        """Text (+ optional prompt audio / style labels) -> float32 waveform at ``sample_rate`` (or at ``output_sample_rate``,
        as in ``inference_batch``; ``loudness`` / ``peak_ceiling`` / ``max_gain_db``: the output's programme loudness, as
        there; ``tempo``: the speaking rate, as there; ``limiter`` / ``limiter_lookahead_ms`` / ``limiter_release_ms``: the
        look-ahead limiter, as there; ``pitch_shift``: semitones on the output, as there -- not ``pitch``, the label of voice
        creation).  The penalties
        (include/sparkmi.h, smi_llm_admit_penalized) apply before token selection; their defaults leave it unpenalised.
        For voice cloning ``penalize_prompt=False`` keeps the reference clip's semantic tokens out of the repetition
        penalty.  ``return_log_probs=True``: (waveform, info) with info = {``token_ids``: the generated ids,
        ``output_log_probs``: float32, one per id (include/sparkmi.h, smi_llm_admit_logprobs), ``cum_log_prob``: their
        float64 sum}; the waveform is the one the call gives without it.  ``num_return_sequences=n > 1``: a list of n takes
        (waveforms, or (waveform, info) pairs), the prompt prefilled once (include/sparkmi.h, smi_llm_admit_forked) and the
        takes vocoded together -- the same as ``inference_batch`` of the request n times; with its own ``seed``, take j is
        the call alone with ``seed + j``.  ``allowed_token_ids`` (an iterable of ids) / ``speech_tokens_only=True`` (the
        tokenizer's added vocabulary and the eos ids: every ordinary BPE text id is banned): every generated id lies in that
        set (include/sparkmi.h, smi_llm_admit_constrained; eos ids are not added to an ``allowed_token_ids`` set).
        ``no_repeat_ngram_size=n > 0`` (transformers' argument of that name; include/sparkmi.h, smi_llm_admit_ngram): no run of n
        ids occurs twice in prompt + generated ids, which rules out the looping failure of the speech-token generator."""
        n_takes = num_returns(num_return_sequences)
        if n_takes > self._max_batch:
            raise ValueError(f"num_return_sequences={n_takes} > max_batch={self._max_batch}")
        n_gram = ngram_size(no_repeat_ngram_size)   # (a bool is refused here as it is in the request key)
        pen = dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                   frequency_penalty=frequency_penalty, min_new_tokens=min_new_tokens, penalize_prompt=penalize_prompt)
        return self.inference_batch([dict(text=text, prompt_speech_path=prompt_speech_path, prompt_text=prompt_text,
                                          gender=gender, pitch=pitch, speed=speed, prompt_tokens=prompt_tokens, **pen,
                                          **({FORK_KEY: n_takes} if n_takes > 1 else {}),
                                          **({ALLOW_KEY: allowed_token_ids} if allowed_token_ids is not None else {}),
                                          **({SPEECH_ONLY_KEY: speech_tokens_only} if speech_tokens_only else {}),
                                          **({NGRAM_KEY: n_gram} if n_gram > 0 else {}))],
                                    temperature=temperature, top_k=top_k, top_p=top_p, do_sample=do_sample,
                                    max_new_tokens=max_new_tokens, seed=seed, return_log_probs=return_log_probs,
                                    output_sample_rate=output_sample_rate, loudness=loudness, peak_ceiling=peak_ceiling,
                                    max_gain_db=max_gain_db, tempo=tempo, limiter=limiter,
                                    limiter_lookahead_ms=limiter_lookahead_ms, limiter_release_ms=limiter_release_ms,
                                    pitch_shift=pitch_shift)[0]

    def _output_ratio(self, output_sample_rate: Optional[int]) -> Optional[Tuple[int, int]]:
        """(up, down) from the model's rate to ``output_sample_rate``; None when the vocoder's rows go out as they are"""
        if output_sample_rate is None:
            return None
        if isinstance(output_sample_rate, bool) or int(output_sample_rate) != output_sample_rate or int(output_sample_rate) < 1:
            raise ValueError(f"output_sample_rate must be a positive integer or None, not {output_sample_rate!r}")
        if int(output_sample_rate) == int(self.sample_rate):
            return None
        from .audio import ratio
        return ratio(self.sample_rate, int(output_sample_rate))

    @staticmethod
    def _no_stream_tempo(tempo, who: str) -> None:
        if tempo is not None:
            raise ValueError(f"{who}: tempo is not supported for overlapping chunks (a time-scale change across chunk edges needs "
                             "carried state); pass joined=True for contiguous pieces at that tempo, or use inference / "
                             "inference_batch / serve / inference_long / inference_long_stream")

    @staticmethod
    def _no_stream_loudness(loudness, who: str) -> None:
        if loudness is not None:
            raise StreamLoudnessRefused(f"{who}: loudness is not supported for overlapping chunks (the running gain is defined on "
                                        "one contiguous stream and carries state across chunk edges); pass joined=True for "
                                        "contiguous pieces at that loudness, or use inference / inference_batch / serve / "
                                        "inference_long / inference_long_stream")

    @staticmethod
    def _check_slew(max_slew_db) -> None:
        v = max_slew_db
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0 <= v <= 200:
            raise ValueError(f"max_slew_db must be a number in 0..200 (dB a hop of 100 ms), not {v!r}")

    @staticmethod
    def _stream_loudness_info(row: Sequence[float]) -> dict:
        """a finished stream's entry: ``loudness`` (LUFS of the whole utterance before the gain, the batch measure), ``peak``,
        ``gain`` (of the last knot) and ``flags`` (the OR over all knots: 1 max_gain, 2 ceiling, 4 slew, 8 hold)"""
        return dict(loudness=float(row[0]), peak=float(row[1]), gain=float(row[2]), flags=int(row[3]))

    def _stream_stages(self, who: str, output_sample_rate: Optional[int], max_streams: int, audio_chunk_duration: float,
                       max_audio_chunk_duration: float, audio_chunk_size_scale_factor: float, audio_chunk_overlap_duration: float,
                       loudness: bool = False, limiter: Optional[Tuple[float, float]] = None, pitch: bool = False):
        """The stages of a ``joined=True`` call with a tempo, a pitch shift, a loudness or a streaming limiter, in the batch path's
        order, their slots all free: (the crossfade -- a ``StreamJoiner`` at 1/1 --, the ``StreamTempo`` or, with ``pitch``, the
        ``StreamPitch`` that takes its place (one stretch pass serves both), with ``loudness`` the
        ``StreamLoudness``, else None, with ``limiter`` = (lookahead_ms, release_ms) the ``StreamLimiter``, else None, and with
        ``output_sample_rate`` the resampler with state -- a second ``StreamJoiner`` with overlap 0 at that ratio, which is
        plain concatenation plus the filter --, else None).  Every stage's ``max_chunk`` is the longest piece the stage before it
        can emit.  Everything is checked before any device call."""
        from .audio import StreamJoiner, StreamLimiter, StreamLoudness, StreamPitch, StreamTempo, tempo_frame
        out_ratio = self._output_ratio(output_sample_rate)
        fade = self._stream_joiner(who, None, max_streams, audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor,
                                   audio_chunk_overlap_duration)
        frame = tempo_frame(self.sample_rate)
        key = (int(max_streams), fade.max_chunk, frame)
        if pitch:
            if getattr(self, "_pitchs", None) is None:
                self._pitchs = {}
            if key not in self._pitchs:
                self._pitchs[key] = StreamPitch(*key, device=self.device)
            scale = self._pitchs[key]
            scale.reset()
            longest = scale.longest()   # what a push of the pitch stage emits at most: the stretch's piece at up to two outputs a sample
        else:
            if getattr(self, "_tempos", None) is None:
                self._tempos = {}
            if key not in self._tempos:
                self._tempos[key] = StreamTempo(*key, device=self.device)
            scale = self._tempos[key]
            scale.reset()
            longest = 4 * (scale.history + scale.max_chunk) + scale.N   # what a push of the tempo stage emits at most (include/sparkmi.h)
        loud = None
        if loudness:
            key = (int(max_streams), longest)
            if getattr(self, "_louds", None) is None:
                self._louds = {}
            if key not in self._louds:
                self._louds[key] = StreamLoudness(*key, sr=self.sample_rate, max_seconds=3600.0, device=self.device)
            loud = self._louds[key]
            loud.reset()
            longest += 5 * loud.hop   # a stream's last push brings what the stage held back
        lim = None
        if limiter is not None:
            key = (int(max_streams), longest, float(limiter[0]), float(limiter[1]))
            if getattr(self, "_limits", None) is None:
                self._limits = {}
            if key not in self._limits:
                self._limits[key] = StreamLimiter(key[0], key[1], sr=self.sample_rate, lookahead_ms=key[2], release_ms=key[3],
                                                  device=self.device)
            lim = self._limits[key]
            lim.reset()
            longest += lim.delay      # A + R + 10: likewise
        rate = None
        if out_ratio is not None:
            key = (int(max_streams), longest, 0) + tuple(out_ratio)
            if key not in self._joiners:
                self._joiners[key] = StreamJoiner(*key, device=self.device)
            rate = self._joiners[key]
            rate.reset()
        return fade, scale, loud, lim, rate

    @staticmethod
    def _open_scale(stage, key, rate: Optional[Tuple[int, int]], shift: Optional[Tuple[int, int]]) -> None:
        """opens request ``key`` in stage 1: a ``StreamTempo`` at its tempo, or a ``StreamPitch`` at its tempo and pitch ratio
        (the taps' copy is enqueued on the current stream: the one the pushes go to)"""
        from .audio import StreamPitch
        if isinstance(stage, StreamPitch):
            stage.open(key, rate or (1, 1), shift or (1, 1))
        else:
            stage.open(key, *(rate or (1, 1)))

    def _staged_push(self, stages, x, rows: Sequence[Tuple]):
        """One poll's ready chunks ``rows[b] = (key, length, last)`` (``x`` [B][stride] on the device) through the stages of
        ``_stream_stages``, all enqueued on the current stream: (rows on the device, {b: its row there}, the final pieces'
        lengths, the pieces' lengths behind the tempo stage -- what a listener hears, at the model's rate --, and {b: the
        loudness stage's stats row, on the device} and {b: the limiter stage's} for the rows that are their stream's last).  A
        stage is skipped for a push whose piece from the stage before is empty, unless it is the stream's last: its later
        pieces are empty."""
        cur, lens = stages[0].push(x, rows)
        lens = list(lens)
        at = {b: b for b in range(len(rows))}
        heard, final, final_lim = lens, {}, {}
        for stage in stages[1:]:
            if stage is None:
                continue
            go = [b for b in sorted(at) if lens[b] > 0 or rows[b][2]]
            for b in at:
                if b not in go:
                    lens[b] = 0
            if not go:
                at = {}
            else:
                src = [at[b] for b in go]
                if src != list(range(cur.shape[0])):
                    cur = cur[torch.tensor(src, device=self.device)].contiguous()
                cur, got = stage.push(cur, [(rows[b][0], lens[b], rows[b][2]) for b in go])
                at = {b: i for i, b in enumerate(go)}
                for b, v in zip(go, got):
                    lens[b] = v
            if stage is stages[1]:
                heard = list(lens)
            elif stage is stages[2] and go:
                final = {b: stage.last_stats[i] for i, b in enumerate(go) if rows[b][2]}
            elif stage is stages[3] and go:
                final_lim = {b: stage.last_stats[i] for i, b in enumerate(go) if rows[b][2]}
        return cur, at, lens, heard, final, final_lim

    @staticmethod
    def _stream_limiter_info(row: Sequence[float]) -> dict:
        """a finished stream's entry, as ``inference_batch``'s ``last_limiter``: ``true_peak`` (going in; the sample peak in the
        "sample" mode), ``reduction_db`` (-20 log10 of the smallest factor) and ``limited_samples``"""
        peak, _, smin, count = row
        return dict(true_peak=peak, reduction_db=0.0 if smin >= 1.0 else (math.inf if smin <= 0.0 else -20.0 * math.log10(smin)),
                    limited_samples=int(count))

    @staticmethod
    def _no_stream_rate(output_sample_rate: Optional[int], who: str) -> None:
        if output_sample_rate is not None:
            raise ValueError(f"{who}: output_sample_rate is not supported for overlapping chunks (a chunk alone has no filter "
                             "state across its edges); pass joined=True for contiguous pieces at that rate, or use inference / "
                             "inference_batch")

    def _stream_joiner(self, who: str, output_sample_rate: Optional[int], max_streams: int, audio_chunk_duration: float,
                       max_audio_chunk_duration: float, audio_chunk_size_scale_factor: float, audio_chunk_overlap_duration: float):
        """The ``StreamJoiner`` of a ``joined=True`` call, its slots all free.  Everything is checked before any device call:
        the rate, the scheduler's arguments, and that the first chunk holds two overlaps (every later chunk that is not a
        request's last is at least as long, and a last chunk may be as short as one overlap)."""
        from .audio import StreamJoiner
        up, down = self._output_ratio(output_sample_rate) or (1, 1)
        hop = self.audio_tokenizer.model.hop
        sched = ChunkScheduler(audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor,
                               audio_chunk_overlap_duration, self.sample_rate // hop)
        if 2 * sched.overlap > sched.chunk_size:
            raise ValueError(f"{who}: joined=True needs a first chunk of at least two overlaps: audio_chunk_duration gives "
                             f"{sched.chunk_size} frames, audio_chunk_overlap_duration {sched.overlap}")
        key = (int(max_streams), max(sched.chunk_size, sched.max_chunk_size) * hop, sched.overlap * hop, up, down)
        if getattr(self, "_joiners", None) is None:
            self._joiners = {}
        if key not in self._joiners:
            self._joiners[key] = StreamJoiner(*key, device=self.device)
        self._joiners[key].reset()
        return self._joiners[key]

    def _device_audio(self):
        if getattr(self, "_audio", None) is None:
            from .audio import DeviceAudio
            self._audio = DeviceAudio(self.device)
        return self._audio

    @staticmethod
    def _loudness_targets(requests: Sequence[dict], loudness, peak_ceiling, max_gain_db) -> List[Optional[float]]:
        """every request's loudness target (its own ``loudness`` key, else the call's; None: left as vocoded), all checked"""
        check_loudness(loudness, peak_ceiling, max_gain_db)
        out = []
        for i, r in enumerate(requests):
            t = r.get(LOUDNESS_KEY, loudness)
            try:
                check_loudness(t, peak_ceiling, max_gain_db)
            except ValueError as e:
                raise ValueError(f"request {i}: {e}") from None
            out.append(None if t is None else float(t))
        return out

    def _normalize_rows(self, wav, n: Sequence[int], targets: Sequence[Optional[float]], peak_ceiling: float, max_gain_db: float,
                        spans=None):
        """Vocoded rows to their loudness targets, in place and on the device (``audio.DeviceAudio.loudness_rows`` /
        ``gain_rows``: five launches for all rows, nothing waits).  Returns the rows' stats [B][4] on the device, or None where
        no row has a target -- then nothing is launched."""
        if all(t is None for t in targets):
            return None
        audio = self._device_audio()
        stats = audio.loudness_rows(wav, n, spans=spans, targets=targets, max_gain_db=max_gain_db, ceiling=peak_ceiling, sr=self.sample_rate)
        audio.gain_rows(wav, n, stats, spans=spans, out=wav)
        return stats

    @staticmethod
    def _loudness_info(stats, targets: Sequence[Optional[float]]) -> List[Optional[dict]]:
        """one small copy: per row with a target {``loudness`` (LUFS before the gain), ``gain``, ``limited`` (None, "max_gain" or
        "ceiling")}, None for a row without one"""
        if stats is None:
            return [None] * len(targets)
        host = stats.cpu().tolist()
        return [None if t is None else dict(loudness=row[0], gain=row[2], limited=LIMITED[int(row[3])]) for t, row in zip(targets, host)]

    def _limiter_modes(self, requests: Sequence[dict], limiter, peak_ceiling, lookahead_ms, release_ms, first: int = 0):
        """(every request's limiter mode -- its own ``limiter`` key, else the call's; None: no limiter --, (A, R): the look-ahead
        and the release in samples at the model's rate), all checked"""
        reach = check_limiter(limiter, peak_ceiling, lookahead_ms, release_ms, self.sample_rate)
        out = []
        for i, r in enumerate(requests):
            m = r.get(LIMITER_KEY, limiter)
            try:
                check_limiter(m, peak_ceiling, lookahead_ms, release_ms, self.sample_rate)
            except ValueError as e:
                raise ValueError(f"request {first + i}: {e}") from None
            out.append(m)
        return out, reach

    @staticmethod
    def _no_stream_limiter(limiter, who: str) -> None:
        if limiter is not None:
            raise ValueError(f"{who}: limiter is not supported on chunked streams (the look-ahead and the release reach across "
                             "chunk edges): pass joined=True with stream_limiter= for the streaming form, whose pieces leave "
                             "A + R + 10 samples late, or use inference / inference_batch / serve / inference_long / "
                             "inference_long_stream")

    @staticmethod
    def _no_stream_limiter_form(stream_limiter, who: str) -> None:
        if stream_limiter is not None:
            raise ValueError(f"{who}: stream_limiter is not supported for overlapping chunks (the limiter works on one contiguous "
                             "stream and carries its input across chunk edges); pass joined=True")

    def _stream_limiter_mode(self, r: dict, stream_limiter, peak_ceiling, lookahead_ms, release_ms, who: str = ""):
        """the streaming limiter's mode of one request -- its own ``stream_limiter`` key, else the call's; None: none --, checked"""
        m = r.get(STREAM_LIMITER_KEY, stream_limiter)
        try:
            check_limiter(m, peak_ceiling, lookahead_ms, release_ms, self.sample_rate)
        except ValueError as e:
            raise ValueError(who + str(e).replace("limiter must", "stream_limiter must", 1)) from None
        return m

    def _level_rows(self, wav, n: Sequence[int], targets: Sequence[Optional[float]], modes: Sequence[Optional[str]], peak_ceiling: float,
                    max_gain_db: float, reach: Tuple[int, int], spans=None):
        """The loudness stage and the limiter for rows, in place and on the device: (the loudness stats [B][4] or None, the
        limiter's stats [B][4] or None).  Without a limiter this is ``_normalize_rows``, launch for launch.  Rows with a
        limiter are measured with a ceiling that cannot bind and go through ``audio.DeviceAudio.limit_rows``, which applies the
        loudness gain itself and holds ``peak_ceiling``; ``gain_rows`` is not launched for them.  Rows of different modes in one
        call go mode by mode, the other rows as empty spans, which every stage copies."""
        if all(m is None for m in modes):
            return self._normalize_rows(wav, n, targets, peak_ceiling, max_gain_db, spans=spans), None
        audio = self._device_audio()
        B = len(n)
        full = [(0, int(v)) for v in n] if spans is None else [(int(a), int(b)) for a, b in spans]
        stats = lstats = None
        for mode in (None,) + LIMITER_MODES:
            rows = [b for b in range(B) if modes[b] == mode]
            if not rows:
                continue
            sp = spans if len(rows) == B else [full[b] if modes[b] == mode else (0, 0) for b in range(B)]
            tg = [targets[b] if modes[b] == mode else None for b in range(B)]
            st = None
            if any(t is not None for t in tg):
                st = audio.loudness_rows(wav, n, spans=sp, targets=tg, max_gain_db=max_gain_db,
                                         ceiling=peak_ceiling if mode is None else NO_CEILING, sr=self.sample_rate)
            if mode is None:
                if st is not None:
                    audio.gain_rows(wav, n, st, spans=sp, out=wav)
                ls = None
            else:
                _, ls = audio.limit_rows(wav, n, gains=st, spans=sp, ceiling=peak_ceiling, mode=mode, lookahead=reach[0],
                                         release=reach[1], out=wav)
            if len(rows) == B:
                stats, lstats = st, ls
            else:   # (a few words per row, merged on the device so that one copy brings them all)
                idx = torch.tensor(rows, dtype=torch.long, device=wav.device)
                if st is not None:
                    stats = torch.full((B, 4), math.nan, dtype=torch.float64, device=wav.device) if stats is None else stats
                    stats[idx] = st[idx]
                if ls is not None:
                    lstats = torch.full((B, 4), math.nan, dtype=torch.float64, device=wav.device) if lstats is None else lstats
                    lstats[idx] = ls[idx]
        return stats, lstats

    @staticmethod
    def _level_info(stats, lstats, targets: Sequence[Optional[float]], modes: Sequence[Optional[str]]):
        """one small copy behind everything enqueued: (``_loudness_info``'s entries, per row with a limiter {``true_peak``: of
        the row times its gain, going in (the sample peak in "sample" mode), ``reduction_db``: -20 log10 of the smallest
        factor, ``limited_samples``}, None for a row without one)"""
        if lstats is None:
            return SparkTTS._loudness_info(stats, targets), [None] * len(targets)
        host = (lstats if stats is None else torch.cat([stats, lstats], dim=1)).cpu().tolist()
        loud = [None if t is None or stats is None else dict(loudness=row[0], gain=row[2], limited=LIMITED[int(row[3])])
                for t, row in zip(targets, host)]
        lim = []
        for m, row in zip(modes, host):
            peak, _, smin, count = row[-4:]
            lim.append(None if m is None else dict(true_peak=peak, reduction_db=0.0 if smin >= 1.0 else (
                math.inf if smin <= 0.0 else -20.0 * math.log10(smin)), limited_samples=int(count)))
        return loud, lim

    @staticmethod
    def _tempo_ratios(requests: Sequence[dict], tempo, first: int = 0) -> List[Optional[Tuple[int, int]]]:
        """every request's tempo as (p, q) (its own ``tempo`` key, else the call's), all checked; None for a request without
        one or at 1.0, which is left as vocoded.  ``first``: the index of ``requests[0]`` in the caller's list, for the message."""
        if tempo is not None:
            tempo_ratio(tempo)
        out = []
        for i, r in enumerate(requests):
            t = r.get(TEMPO_KEY, tempo)
            try:
                pq = None if t is None else tempo_ratio(t)
            except ValueError as e:
                raise ValueError(f"request {first + i}: {e}") from None
            out.append(None if pq == (1, 1) else pq)
        return out

    @staticmethod
    def _pitch_ratios(requests: Sequence[dict], pitch_shift, first: int = 0) -> List[Optional[Tuple[int, int]]]:
        """every request's pitch shift as the frequency ratio (p, q) (its own ``pitch_shift`` key, else the call's), all checked;
        None for a request without one or whose ratio comes out 1/1, which is left as it is.  ``first``: as in ``_tempo_ratios``."""
        if pitch_shift is not None:
            pitch_ratio(pitch_shift)
        out = []
        for i, r in enumerate(requests):
            t = r.get(PITCH_SHIFT_KEY, pitch_shift)
            try:
                pq = None if t is None else pitch_ratio(t)
            except ValueError as e:
                raise ValueError(f"request {first + i}: {e}") from None
            out.append(None if pq == (1, 1) else pq)
        return out

    @staticmethod
    def _no_stream_pitch(pitch_shift, who: str) -> None:
        if pitch_shift is not None:
            raise ValueError(f"{who}: pitch_shift is not supported on chunked streams, joined or not (the stretch and the resampler "
                             "behind it would need their state carried across chunk edges); the batch calls take it: inference / "
                             "inference_batch / serve / inference_long / inference_long_stream")

    @staticmethod
    def _stream_pitch_ratios(requests: Sequence[dict], stream_pitch_shift, first: int = 0) -> List[Optional[Tuple[int, int]]]:
        """``_pitch_ratios`` for the streaming calls: a request's own ``stream_pitch_shift`` key, else the call's; values and
        rounding are ``audio.pitch_ratio``'s, and the message names the streaming keyword"""
        def one(v):
            try:
                return pitch_ratio(v)
            except ValueError as e:
                raise ValueError(str(e).replace("pitch_shift", "stream_pitch_shift", 1)) from None
        if stream_pitch_shift is not None:
            one(stream_pitch_shift)
        out = []
        for i, r in enumerate(requests):
            t = r.get(STREAM_PITCH_SHIFT_KEY, stream_pitch_shift)
            try:
                pq = None if t is None else one(t)
            except ValueError as e:
                raise ValueError(f"request {first + i}: {e}") from None
            out.append(None if pq == (1, 1) else pq)
        return out

    @staticmethod
    def _no_stream_pitch_form(stream_pitch_shift, who: str) -> None:
        if stream_pitch_shift is not None:
            raise ValueError(f"{who}: stream_pitch_shift is not supported for overlapping chunks (the stretch and the resampler "
                             "behind it carry state across chunk edges); pass joined=True for contiguous pieces at that pitch, or "
                             "use pitch_shift on inference / inference_batch / serve / inference_long / inference_long_stream")

    def _tempo_rows(self, wav, n: Sequence[int], ratios: Sequence[Optional[Tuple[int, int]]], spans=None,
                    pitches: Optional[Sequence[Optional[Tuple[int, int]]]] = None):
        """Rows (or their ``spans``) at their tempos, on the device (``audio.DeviceAudio.tempo_rows``: two launches for all rows,
        nothing waits): (new rows, their lengths).  A row without a ratio goes through at 1/1, which copies it bit for bit.
        Where no row has a ratio nothing is launched: (wav, n) as they came -- only without ``spans``.  Where any row has a
        pitch ratio (``pitches``) the pitch stage replaces the tempo stage for all rows of the call
        (``audio.DeviceAudio.pitch_rows``: two launches as well, the tempo and the pitch in one stretch pass; a row without a
        pitch ratio comes out as ``tempo_rows`` gives it, bit for bit)."""
        if pitches is not None and any(r is not None for r in pitches):
            y, m, _ = self._device_audio().pitch_rows(wav.contiguous(), n, [r or (1, 1) for r in ratios], [r or (1, 1) for r in pitches],
                                                      spans=spans, sr=self.sample_rate)
            return y, m
        if spans is None and all(r is None for r in ratios):
            return wav, list(n)
        y, m, _ = self._device_audio().tempo_rows(wav.contiguous(), n, [r or (1, 1) for r in ratios], spans=spans, sr=self.sample_rate)
        return y, m

    @torch.no_grad()
    def inference_batch(self, requests: Sequence[dict], temperature: float = 0.8, top_k: float = 50,
                        top_p: float = 0.95, *, do_sample: bool = True, max_new_tokens: int = 3000,
                        seed: Optional[int] = None, return_log_probs: bool = False, prompt_encode: str = "streams",
                        prompt_audio: str = "host", output_sample_rate: Optional[int] = None,
                        loudness: Optional[float] = None, peak_ceiling: float = PEAK_CEILING, max_gain_db: float = 20.0,
                        tempo: Optional[float] = None, limiter: Optional[str] = None, limiter_lookahead_ms: float = 2.5,
                        limiter_release_ms: float = 25.0, pitch_shift: Optional[float] = None) -> List:
        """Several independent utterances in one ragged batch (<= max_batch).  Greedy: each result equals the
        single-utterance call for that request -- exactly with an f32 KV cache; with the default bf16 cache up to near-tie
        arg-max flips between the prefill kernels the two call shapes select (include/sparkmi.h, smi_llm_session_begin).
        A request may carry its own ``do_sample`` / ``temperature`` / ``top_k`` / ``top_p`` / ``seed`` (the call's arguments
        are the defaults of the keys it leaves out; TensorRT-LLM's per-request inputs): such a batch, even of one request,
        runs through the admission path, so a request with its own ``seed`` gets the same tokens alone and in any batch.
        Likewise ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` / ``min_new_tokens`` /
        ``penalize_prompt`` (TensorRT-LLM's per-request penalty inputs); neutral values leave the request's route unchanged.
        ``return_log_probs=True`` (every request) or a request's ``return_log_probs`` key: that request's waveform comes as
        (waveform, info), info as in ``inference``; such a batch runs through the admission path.
        A request's ``num_return_sequences`` key (an int >= 1): that many takes of it, its prompt prefilled once; its result
        is a list of one result per take.  All takes together are at most ``max_batch``.  A request's ``allowed_token_ids``
        / ``speech_tokens_only`` keys (as in ``inference``) restrict its generated ids, and its ``no_repeat_ngram_size`` key
        (as in ``inference``) bans repeated n-grams; such a batch runs through the admission path.
        ``prompt_encode``: how the batch's prompt files are encoded -- "streams" (default): side by side on parallel HIP streams
        (``tokenize_many``); "rows": as one ragged call on one handle (``tokenize_rows``).  The ids are equal bit for bit, so
        the waveforms are the same.
        ``prompt_audio``: where the prompt files are resampled, volume-normalised and clipped -- "host" (default): numpy / scipy,
        file by file, as ever; "device" (needs ``prompt_encode="rows"``): in one device call for all of them
        (``BiCodecTokenizer.tokenize_rows``).  Both follow ``resample_poly``, not the reference's soxr VHQ; the device path works in
        fp32, so its prompt ids may differ from the host path's at near-ties.
        ``output_sample_rate``: None or the model's rate: the vocoder's rows as they are.  Another rate (24000, 44100, 48000,
        8000, ...): every row is resampled on the device (``sparkmi/audio.py``, ``resample_poly``'s arithmetic in fp32) before
        the copy to the host; row b then has ``audio.out_len`` of its own length.
        ``loudness`` (LUFS, e.g. -23 or -16; None: the rows as vocoded, no extra launch) or a request's own ``loudness`` key,
        which overrides it: the whole vocoded row is brought to that programme loudness (ITU-R BS.1770; include/sparkmi.h,
        smi_loud_rows) on the device, after vocoding and before the resampling -- by a gain of at most ``max_gain_db`` that
        keeps the sample peak at or below ``peak_ceiling`` (a sample peak, not a true peak); a silent row is left as it is.
        All rows go through the same two device calls.  ``self.last_loudness`` then holds, per request (per take where it
        has takes), None or {``loudness``: measured before the gain, ``gain``, ``limited``: None / "max_gain" / "ceiling"}.
        ``tempo`` (0.5 .. 2.0, to a hundredth; > 1: faster; None or 1.0: the rows as vocoded, no extra launch) or a request's own
        ``tempo`` key, which overrides it: the speaking rate of the vocoded row is changed at unchanged pitch (WSOLA;
        include/sparkmi.h, smi_tempo_rows) on the device, after vocoding and before the loudness stage, which measures the
        final signal; a row of n samples then has ``audio.tempo_len(n, p, q)``.  It works for cloned voices, which the
        ``speed`` label of voice creation does not reach, and it is exact where the label is a hint.
        ``limiter`` (None: nothing is launched and no bit changes; "true"; "sample") or a request's own ``limiter`` key, which
        overrides it: a look-ahead limiter (include/sparkmi.h, smi_limit_rows) on the device, behind the
        loudness stage and before the resampling, keeps every sample of the row at or under ``peak_ceiling`` by reducing the
        gain around the overs only -- from ``limiter_lookahead_ms`` (2.5) before them to ``limiter_release_ms`` (25) behind --;
        "true" finds the overs on the 4x oversampled signal, "sample" on the samples.  With ``loudness`` the row then reaches
        its target (or ``max_gain_db``): the loudness stage measures with a ceiling that cannot bind, the limiter applies its
        gain, and ``limited`` is None or "max_gain".  Without ``loudness`` the limiter alone bounds the vocoder's output.
        ``self.last_limiter`` holds, per request (per take where it has takes), None or {``true_peak``: going in,
        ``reduction_db``: the deepest reduction, ``limited_samples``}, from the one small copy that brings ``last_loudness``.
        ``pitch_shift`` (semitones, -12.0 .. 12.0; > 0: higher; None or a value whose ratio comes out 1/1: nothing new is
        launched and no bit changes) or a request's own ``pitch_shift`` key, which overrides it: the vocoded row's pitch is moved
        by the frequency ratio ``audio.pitch_ratio`` gives (2 ** (s / 12) to a hundredth: about 9 to 17 cents) at unchanged
        length, on the device (include/sparkmi.h, smi_pitch_rows).  It works for cloned voices, which the
        ``pitch`` label of voice creation does not reach.  Where a call has a pitched row the stage replaces the tempo stage:
        one WSOLA stretch serves ``tempo`` and ``pitch_shift`` together, a polyphase resampler follows inside the same launch,
        and the row has ``audio.tempo_len(n, p, q)`` samples as with ``tempo`` alone.  The formants move with the pitch."""
        targets = self._loudness_targets(requests, loudness, peak_ceiling, max_gain_db)
        ratios = self._tempo_ratios(requests, tempo)
        shifts = self._pitch_ratios(requests, pitch_shift)
        if prompt_encode not in ("streams", "rows"):
            raise ValueError(f"prompt_encode must be 'streams' or 'rows', not {prompt_encode!r}")
        if prompt_audio not in ("host", "device"):
            raise ValueError(f"prompt_audio must be 'host' or 'device', not {prompt_audio!r}")
        if prompt_audio == "device" and prompt_encode != "rows":
            raise ValueError("prompt_audio='device' prepares the prompts for the rows encode: pass prompt_encode='rows'")
        out_ratio = self._output_ratio(output_sample_rate)
        if len(requests) > self._max_batch:
            raise ValueError(f"{len(requests)} requests > max_batch={self._max_batch}")
        n_takes = _take_counts(requests, self._max_batch)
        modes, reach = self._limiter_modes(requests, limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        prompts, globals_ = [], []
        # voice-clone requests that come with prompt FILES: all their prompt encodes run together (parallel HIP streams, or one ragged call)
        need = [i for i, r in enumerate(requests)
                if r.get("gender") is None and r.get("prompt_tokens") is None and r.get("prompt_speech_path") is not None]
        if len(need) > 1 or (need and prompt_audio == "device"):
            paths = [requests[i]["prompt_speech_path"] for i in need]
            if prompt_audio == "device":
                toks = self.audio_tokenizer.tokenize_rows(paths, prompt_audio="device")
            else:
                toks = self.audio_tokenizer.tokenize_rows(paths) if prompt_encode == "rows" else self.audio_tokenizer.tokenize_many(paths)
            requests = [dict(r) for r in requests]
            for i, t in zip(need, toks):
                requests[i]["prompt_tokens"] = t
        for r in requests:
            if r.get("gender") is not None:
                prompts.append(self.process_prompt_control(r["gender"], r.get("pitch"), r.get("speed"), r["text"]))
                globals_.append(None)
            else:
                p, g = self.process_prompt(r["text"], r.get("prompt_speech_path"), r.get("prompt_text"),
                                           r.get("prompt_tokens"))
                prompts.append(p)
                globals_.append(g)
        ids = [self.tokenizer([p], return_tensors="pt").input_ids[0].tolist() for p in prompts]
        # the reference's budget (3000) against a 32k-position model never binds; here the KV arena holds max_positions
        # tokens per sequence, so the budget shrinks with the prompt (as inference_stream and serve do) -- only a
        # prompt that itself does not fit is an error
        room = self._max_positions - max(len(i) for i in ids)
        if room < 1:
            raise ValueError(f"a prompt of {max(len(i) for i in ids)} tokens does not fit max_positions={self._max_positions}")
        max_new_tokens = min(int(max_new_tokens), room)
        sampling = [_request_sampling(r, self.speech_token_ids, self._eos, self.model.cfg.vocab_size) for r in requests]
        if return_log_probs:
            sampling = [dict(d or {}, return_log_probs=True) for d in sampling]
        owner = list(range(len(ids)))   # request of every generated row
        if n_takes is not None:          # takes of one prompt: one forked admission (SparkLLM.admit(n_return=...))
            self.model.set_sampling(bool(do_sample), temperature, int(top_k), float(top_p), seed)
            grouped = self.model.generate_ragged(ids, [max_new_tokens] * len(ids), self._eos, sampling=sampling, n_return=n_takes)
            owner = [b for b, k in enumerate(n_takes) for _ in range(k)]
            new = [r for takes in grouped for r in takes]
            globals_ = [globals_[b] for b in owner]
        elif any(sampling):   # (max_batch = the LLM's slots)
            self.model.set_sampling(bool(do_sample), temperature, int(top_k), float(top_p), seed)
            new = self.model.generate_ragged(ids, [max_new_tokens] * len(ids), self._eos, sampling=sampling)
        elif len(ids) > 1 and self._eos and len(ids) <= self.model.max_slots:
            # a batch: rows are retired at their own eos (SparkLLM.generate_ragged), so the step runs on the rows still
            # speaking instead of padding the finished ones to the longest utterance; same tokens per row
            self.model.set_sampling(bool(do_sample), temperature, int(top_k), float(top_p), seed)
            new = self.model.generate_ragged(ids, [max_new_tokens] * len(ids), self._eos)
        elif do_sample:
            new = self.model.generate_ids(ids, max_new_tokens, self._eos, do_sample=True, temperature=temperature,
                                          top_k=int(top_k), top_p=float(top_p), seed=seed)
        else:
            new = self.model.generate_ids(ids, max_new_tokens, self._eos)
        infos: List[Optional[dict]] = [None] * len(new)
        for b, r in enumerate(new):
            if isinstance(r, tuple):   # a flagged row: (tokens, log-probabilities)
                new[b] = r[0]
                infos[b] = _lp_info(*r)
        sems, globs, lens = [], [], []
        ntok = self.audio_tokenizer.model.cfg.spk_token_num
        for b, toks in enumerate(new):
            sem, glob = self._parse(toks)
            if globals_[b] is None:
                g = torch.tensor(glob, dtype=torch.long)
            else:
                g = torch.as_tensor(globals_[b]).reshape(-1).long()
            if g.numel() != ntok:
                raise ValueError(f"request {b}: {g.numel()} global tokens generated, the speaker encoder needs {ntok}")
            if not sem:
                raise ValueError(f"request {b}: the model generated no semantic tokens")
            sems.append(sem)
            globs.append(g)
            lens.append(len(sem))
        T = max(lens)
        sem_t = torch.zeros((len(sems), T), dtype=torch.long)
        for b, s in enumerate(sems):
            sem_t[b, : len(s)] = torch.tensor(s)
        wav = self.audio_tokenizer.model.detokenize(sem_t, torch.stack(globs).unsqueeze(1), lengths=lens)
        hop = self.audio_tokenizer.model.hop
        n_wav = [n * hop for n in lens]
        wav = wav.squeeze(1)
        row_targets = [targets[b] for b in owner]
        wav, n_wav = self._tempo_rows(wav, n_wav, [ratios[b] for b in owner], pitches=[shifts[b] for b in owner])
        row_modes = [modes[b] for b in owner]
        stats = lstats = None
        if any(t is not None for t in row_targets) or any(m is not None for m in row_modes):
            wav = wav.contiguous()
            stats, lstats = self._level_rows(wav, n_wav, row_targets, row_modes, peak_ceiling, max_gain_db, reach)
        if out_ratio is not None:   # rows at the caller's rate, still on the device
            wav, n_wav = self._device_audio().resample_rows(wav, n_wav, [out_ratio[0]] * len(lens), [out_ratio[1]] * len(lens))
        wav = wav.cpu().numpy()
        loud, lim = self._level_info(stats, lstats, row_targets, row_modes)
        out = [wav[b, : n_wav[b]].copy() for b in range(len(sems))]
        out = [(w, infos[b]) if infos[b] is not None else w for b, w in enumerate(out)]
        if n_takes is None:
            self.last_loudness, self.last_limiter = loud, lim
            return out
        res: List = [[] for _ in requests]
        per: List = [[] for _ in requests]
        perl: List = [[] for _ in requests]
        for i, b in enumerate(owner):
            res[b].append(out[i])
            per[b].append(loud[i])
            perl[b].append(lim[i])
        self.last_loudness = [per[b] if FORK_KEY in r else per[b][0] for b, r in enumerate(requests)]
        self.last_limiter = [perl[b] if FORK_KEY in r else perl[b][0] for b, r in enumerate(requests)]
        return [res[b] if FORK_KEY in r else res[b][0] for b, r in enumerate(requests)]

    @torch.no_grad()
    def inference_stream(self, text: str, prompt_speech_path: Path = None, prompt_text: str = None,
                         gender: str = None, pitch: str = None, speed: str = None,
                         temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *,
                         do_sample: bool = True, max_new_tokens: int = 3000, seed: Optional[int] = None,
                         prompt_tokens: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                         audio_chunk_duration: float = 1.0, max_audio_chunk_duration: float = 30.0,
                         audio_chunk_size_scale_factor: float = 8.0, audio_chunk_overlap_duration: float = 0.1,
                         decode_stride: int = 10, output_sample_rate: Optional[int] = None,
                         joined: bool = False, tempo: Optional[float] = None, loudness: Optional[float] = None,
                         peak_ceiling: float = PEAK_CEILING, max_gain_db: float = 20.0,
                         max_slew_db: float = 1.0, limiter: Optional[str] = None, stream_limiter: Optional[str] = None,
                         limiter_lookahead_ms: float = 2.5, limiter_release_ms: float = 25.0,
                         pitch_shift: Optional[float] = None, stream_pitch_shift: Optional[float] = None) -> Iterator[np.ndarray]:
        """Yields float32 waveform chunks while the LLM is still generating, cut and overlapped as
        the reference's decoupled Triton model does (model.py:347-385; run.sh:53-56 defaults); join
        them with ``sparkmi.streaming.crossfade(chunks, int(overlap_duration * sample_rate))``
        (client_grpc.py:390-415).  Every chunk is the vocoder's output for that chunk's tokens alone.
        ``decode_stride`` = decode steps enqueued between host checks for new tokens.  The chunks are at ``sample_rate``:
        with ``joined=False`` a given ``output_sample_rate`` is refused (ValueError) -- a resampled chunk would need the
        filter's state across the chunk edges.

        ``joined=True``: yields contiguous, playable float32 pieces instead -- a listener plays them one after the other.
        The chunks are cross-faded on the device (include/sparkmi.h, smi_join_*; ``audio.StreamJoiner``): the pieces'
        concatenation is ``crossfade`` of the chunks cast to float32, bit for bit, ``semantic tokens * hop`` samples in
        all.  ``output_sample_rate`` is then accepted (None or ``sample_rate``: the model's rate): the pieces'
        concatenation is, bit for bit, what ``inference_batch(output_sample_rate=...)``'s resampler gives for that joined
        waveform, the filter's state being kept across the chunk edges; a piece that would be empty is not yielded.
        Refused (ValueError, before any device call) if the first chunk is shorter than two overlaps.

        ``loudness`` (LUFS; None: nothing new is built or launched) needs ``joined=True``.  The integrated loudness of BS.1770
        is a property of the whole utterance, which a piece that must leave before the utterance ends cannot know, so this is
        not the batch stage: the gain follows the running integrated loudness of what has arrived, knot by knot on the
        stream's absolute hops of 100 ms, moves at most ``max_slew_db`` a hop, is at most ``max_gain_db`` and keeps every
        sample under ``peak_ceiling`` (include/sparkmi.h, smi_louds_*; ``audio.StreamLoudness``).  The stage sits
        behind the tempo stage and before the resampler with state, holds back up to five hops (500 ms) and keeps the total
        length; the pieces do not depend, by a bit, on the chunking.  After the last piece ``self.last_loudness`` holds
        {``loudness`` (of the whole utterance before the gain, equal to the batch measure), ``peak``, ``gain`` (the last
        knot's), ``flags``}: one 32-byte copy.  With ``joined=False`` a given ``loudness`` is refused (ValueError).

        ``tempo`` (0.5 .. 2.0, to a hundredth; > 1: faster; None or 1.0: nothing new is built or launched) needs
        ``joined=True``: the joined stream's speaking rate is changed at unchanged pitch while it is still arriving (WSOLA with
        the frame places and an input history carried on the device; include/sparkmi.h, smi_tempos_*; ``audio.StreamTempo``).
        The stages run in the batch path's order on the device -- crossfade, tempo, then with ``output_sample_rate`` the
        resampler with state -- and only the final pieces are copied.  The pieces' concatenation is, bit for bit,
        ``DeviceAudio.tempo_rows`` of the concatenated ``joined=True`` pieces without tempo (and ``resample_rows`` of that), so
        it does not depend on the chunking; a piece holds back up to N + D + H samples of its input (63 ms at 16 kHz) for the
        frames that are not final yet, and the last piece brings them.  With
        ``joined=False`` a given ``tempo`` is refused (ValueError): overlapping chunks have no edges to carry state across.

        ``stream_limiter`` (None: nothing new is built or launched; "true": peaks of the 4x oversampled signal; "sample": of the
        samples alone) needs ``joined=True``: the look-ahead limiter of ``inference_batch`` on the stream while it is still
        arriving (include/sparkmi.h, smi_limits_*; ``audio.StreamLimiter``), behind the loudness stage and before
        the resampler with state.  ``peak_ceiling``, ``limiter_lookahead_ms`` and ``limiter_release_ms`` mean what they mean
        there.  The limiter is feed-forward, so the pieces' concatenation is, bit for bit, ``DeviceAudio.limit_rows`` of the
        concatenated pieces of the same call without it, whatever the chunking; a piece leaves A + R + 10 samples (28 ms at
        16 kHz) behind its input and the last piece brings them.  Its contract is its own: with ``loudness`` it works behind the
        running gain of that stage, not behind one gain a row, and the loudness stage is then given no ceiling -- its gain
        follows the target and the limiter holds ``peak_ceiling``.  After the last piece ``self.last_limiter`` holds
        {``true_peak``, ``reduction_db``, ``limited_samples``} of the whole stream: one 32-byte copy.  With ``joined=False`` a
        given ``stream_limiter`` is refused (ValueError).

        ``limiter`` is refused (ValueError), joined or not: that keyword names the limiter of whole utterances, which
        ``inference_batch`` has; the streaming form is asked for by ``stream_limiter``.  ``pitch_shift`` is refused (ValueError),
        joined or not: the batch calls take it; the streaming form is asked for by ``stream_pitch_shift``.

        ``stream_pitch_shift`` (semitones, -12.0 .. 12.0; > 0: higher; values and rounding are ``audio.pitch_ratio``'s; None, 0 or
        a value whose ratio comes out 1/1: nothing new is built or launched) needs ``joined=True``: the joined stream's pitch is
        moved at unchanged length while it is still arriving (include/sparkmi.h, smi_pitchs_*; ``audio.StreamPitch``; DESIGN.md
        4.1.10).  The stage takes the tempo stage's place: one stretch pass serves ``tempo`` and the pitch, and the loudness
        stage, ``stream_limiter`` and ``output_sample_rate`` see the shifted stream.  The pieces' concatenation is, bit for bit,
        ``DeviceAudio.pitch_rows`` of the concatenated pieces of the same call without it, whatever the chunking, and as long
        as ``tempo`` alone makes it; a piece is the tempo stream's hold-back plus the filter's reach late and the last piece
        brings the rest.  The formants move with the pitch.  With ``joined=False`` it is refused (ValueError)."""
        self._no_stream_limiter(limiter, "inference_stream")
        self._no_stream_pitch(pitch_shift, "inference_stream")
        if not joined:
            self._no_stream_pitch_form(stream_pitch_shift, "inference_stream")
            self._no_stream_tempo(tempo, "inference_stream")
            self._no_stream_loudness(loudness, "inference_stream")
            self._no_stream_limiter_form(stream_limiter, "inference_stream")
            self._no_stream_rate(output_sample_rate, "inference_stream")
        rate = self._tempo_ratios([{}], tempo)[0]
        shift = self._stream_pitch_ratios([{}], stream_pitch_shift)[0]
        target = self._loudness_targets([{}], loudness, peak_ceiling, max_gain_db)[0]
        self._check_slew(max_slew_db)
        mode = self._stream_limiter_mode({}, stream_limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        sched_args = (audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor, audio_chunk_overlap_duration)
        stages = None
        if joined and (rate is not None or shift is not None or target is not None or mode is not None):
            stages = self._stream_stages("inference_stream", output_sample_rate, 1, *sched_args, loudness=target is not None,
                                         limiter=None if mode is None else (limiter_lookahead_ms, limiter_release_ms),
                                         pitch=shift is not None)
            joiner = stages[0]
            self._open_scale(stages[1], 0, rate, shift)
            if stages[2] is not None:   # (with a limiter behind it the gain follows the target: the limiter holds the ceiling)
                stages[2].open(0, target, max_gain_db, peak_ceiling if mode is None else NO_CEILING, max_slew_db)
                self.last_loudness = None
            if stages[3] is not None:
                stages[3].open(0, mode, peak_ceiling)
                self.last_limiter = None
        else:
            joiner = self._stream_joiner("inference_stream", output_sample_rate, 1, *sched_args) if joined else None
        if gender is not None:
            prompt, glob = self.process_prompt_control(gender, pitch, speed, text), None
        else:
            prompt, g = self.process_prompt(text, prompt_speech_path, prompt_text, prompt_tokens)
            glob = torch.as_tensor(g).reshape(-1).long()
        ids = self.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
        if len(ids) + max_new_tokens > self._max_positions:
            max_new_tokens = self._max_positions - len(ids)
        voc = self.audio_tokenizer.model
        ntok, hop = voc.cfg.spk_token_num, voc.hop
        frame_rate = self.sample_rate // hop
        sched = ChunkScheduler(audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor,
                               audio_chunk_overlap_duration, frame_rate)
        self.model.set_sampling(do_sample, temperature, int(top_k), float(top_p), seed)
        self.model.prefill([ids], self._eos)
        produced, n_sem, pending = 1, 0, []

        def vocode(chunk: List[int]) -> np.ndarray:
            wav = voc.detokenize(torch.tensor([chunk], dtype=torch.long), glob.reshape(1, 1, -1), lengths=[len(chunk)])
            return wav.reshape(-1)[: len(chunk) * hop].cpu().numpy().copy()

        def piece(chunk: List[int], last: bool) -> np.ndarray:   # the chunk's share of the joined stream; only that crosses to the host
            if chunk:
                wav = voc.detokenize(torch.tensor([chunk], dtype=torch.long), glob.reshape(1, 1, -1), lengths=[len(chunk)]).reshape(1, -1)
            else:
                wav = torch.zeros((1, 1), dtype=torch.float32, device=self.device)
            if stages is not None:
                out, at, lens, _, final, final_lim = self._staged_push(stages, wav, [(0, len(chunk) * hop, last)])
                w = out[at[0], : lens[0]].cpu().numpy().copy() if 0 in at else np.zeros(0, dtype=np.float32)
                if 0 in final:   # behind the last piece
                    self.last_loudness = self._stream_loudness_info(final[0].cpu().tolist())
                if 0 in final_lim:
                    self.last_limiter = self._stream_limiter_info(final_lim[0].cpu().tolist())
                return w
            out, lens = joiner.push(wav, [(0, len(chunk) * hop, last)])
            return out[0, : lens[0]].cpu().numpy().copy()

        pushed = 0
        while True:
            toks = self.model.tokens(max_new_tokens)[0]
            sem, gl = self._parse(toks)
            if glob is None and len(gl) >= ntok:        # voice creation: the speaker tokens are generated first
                glob = torch.tensor(gl[:ntok], dtype=torch.long)
            pending += sched.push(sem[n_sem:])
            n_sem = len(sem)
            done = produced >= max_new_tokens or self.model.all_done()
            if done:
                pending += sched.flush()
            if glob is not None and joiner is None:
                for chunk in pending:
                    yield vocode(chunk)
                pending = []
            elif glob is not None:
                if done and pushed + len(pending) > 0 and not pending:
                    pending = [[]]                      # nothing left to flush: an empty last chunk empties the resampler
                for ci, chunk in enumerate(pending):
                    w = piece(chunk, done and ci == len(pending) - 1)
                    pushed += 1
                    if w.size:
                        yield w
                pending = []
            if done:
                break
            n = min(decode_stride, max_new_tokens - produced)
            self.model.decode(n)
            produced += n
        if glob is None:
            raise ValueError(f"{ntok} global tokens were not generated; the speaker encoder needs them")

    # ------------------------------------------------------------------ finished requests: tokens -> rows -> waveforms on the device
    def _cut_eos(self, toks: List[int]) -> List[int]:
        """``toks`` up to and including its first eos id"""
        stops = [toks.index(e) for e in self._eos if e in toks]
        return toks[: min(stops) + 1] if stops else toks

    def _speech_row(self, i, toks: Sequence[int], glob) -> Tuple[List[int], torch.Tensor]:
        """(semantic token values, global token ids) of request ``i``'s generated ids; ``glob``: the prompt's global token ids,
        or None when the ids carry them (voice creation)"""
        sem, gl = self._parse(toks)
        g = torch.tensor(gl, dtype=torch.long) if glob is None else torch.as_tensor(glob).reshape(-1).long()
        ntok = self.audio_tokenizer.model.cfg.spk_token_num
        if g.numel() != ntok:
            raise ValueError(f"request {i}: {g.numel()} global tokens, the speaker encoder needs {ntok}")
        if not sem:
            raise ValueError(f"request {i}: the model generated no semantic tokens")
        return sem, g

    def _vocode_rows(self, rows: Sequence[Tuple[List[int], torch.Tensor]]):
        """One ragged vocoder call for ``rows`` of (semantic values, global ids): (waveforms [B][stride] float32 on the device,
        row b valid for ``lens[b] * hop`` samples; lens, in frames)"""
        lens = [len(sem) for sem, _ in rows]
        sem_t = torch.zeros((len(rows), max(lens)), dtype=torch.long)
        for b, (sem, _) in enumerate(rows):
            sem_t[b, : len(sem)] = torch.tensor(sem)
        wav = self.audio_tokenizer.model.detokenize(sem_t, torch.stack([g for _, g in rows]).unsqueeze(1), lengths=lens)
        return wav.squeeze(1), lens

    @torch.no_grad()
    def serve(self, requests, temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *, do_sample: bool = True,
              max_new_tokens: int = 3000, seed: Optional[int] = None, decode_stride: int = 8, return_log_probs: bool = False,
              loudness: Optional[float] = None, peak_ceiling: float = PEAK_CEILING, max_gain_db: float = 20.0,
              tempo: Optional[float] = None, limiter: Optional[str] = None, limiter_lookahead_ms: float = 2.5,
              limiter_release_ms: float = 25.0, pitch_shift: Optional[float] = None):
        """In-flight batching front end (the functional analogue of the reference's Triton deployment,
        runtime/triton_trtllm/run.sh:50-65): ``requests`` is an iterable of the dicts ``inference_batch`` takes;
        yields ``(index, waveform)`` as each utterance finishes.  Up to ``max_batch`` utterances are live; a new
        request is admitted into the LLM's free KV slot as soon as one retires, so short utterances do not wait for
        long ones.  Greedy results equal ``inference()`` of the same request.  Per-request ``do_sample`` / ``temperature`` /
        ``top_k`` / ``top_p`` / ``seed`` and penalty keys as in ``inference_batch``.  ``return_log_probs=True`` (every
        request) or a request's ``return_log_probs`` key: that request yields ``(index, waveform, info)``, info as in
        ``inference`` (up to and including the first eos id, like the waveform's tokens).  A request's
        ``num_return_sequences`` key (an int >= 1, at most ``max_batch``): that many takes of it, admitted together once
        that many slots are free, its prompt prefilled once; it yields ``(index, [one result per take])`` when all of its
        takes have finished, each take a waveform or a (waveform, info) pair, vocoded together.
        ``loudness`` / ``peak_ceiling`` / ``max_gain_db`` and a request's own ``loudness`` key as in ``inference_batch``: each
        waveform is brought to its target on the device before its copy; ``self.last_loudness[index]`` holds what was measured
        (a list for a request with takes) once the request has been yielded.  ``tempo`` and a request's own ``tempo`` key as in
        ``inference_batch``: the waveform's speaking rate is changed on the device, before the loudness stage.  ``limiter`` /
        ``limiter_lookahead_ms`` / ``limiter_release_ms`` and a request's own ``limiter`` key as in ``inference_batch``: the
        look-ahead limiter behind the loudness stage; ``self.last_limiter[index]`` holds its entry (a list for a request with
        takes) once the request has been yielded.  ``pitch_shift`` and a request's own ``pitch_shift`` key as in
        ``inference_batch``: the waveform's pitch is moved on the device, in the tempo stage's place and pass."""
        forks: Dict[int, int] = {}   # request index -> takes, for the requests that carry num_return_sequences
        lims: Dict[int, Optional[str]] = {}   # request index -> limiter mode
        self.last_limiter = {}
        goals: Dict[int, Optional[float]] = {}   # request index -> loudness target
        rates: Dict[int, Optional[Tuple[int, int]]] = {}   # request index -> tempo as (p, q)
        check_loudness(loudness, peak_ceiling, max_gain_db)
        self._tempo_ratios([], tempo)
        self._pitch_ratios([], pitch_shift)
        shifts: Dict[int, Optional[Tuple[int, int]]] = {}   # request index -> pitch shift as a frequency ratio (p, q)
        self.last_loudness = {}

        def checked(reqs):   # each request's takes, checked before the request reaches the device
            for i, r in enumerate(reqs):
                if FORK_KEY in r:
                    forks[i] = _take_counts([r], self._max_batch)[0]
                _request_seq(r, self._eos, self.model.cfg.vocab_size, f"request {i}")
                goals[i] = self._loudness_targets([r], loudness, peak_ceiling, max_gain_db)[0]
                rates[i] = self._tempo_ratios([r], tempo, i)[0]
                shifts[i] = self._pitch_ratios([r], pitch_shift, i)[0]
                lims[i] = self._limiter_modes([r], limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms, i)[0][0]
                yield r

        if isinstance(requests, (list, tuple)):   # a whole list is checked before anything runs
            for _ in checked(requests):
                pass
        reach = self._limiter_modes([], limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)[1]
        hop = self.audio_tokenizer.model.hop
        globals_: Dict[int, Optional[torch.Tensor]] = {}
        self.model.set_sampling(do_sample, temperature, int(top_k), float(top_p), seed)

        def llm_requests():
            for i, r in enumerate(checked(requests)):
                if r.get("gender") is not None:
                    prompt, g = self.process_prompt_control(r["gender"], r.get("pitch"), r.get("speed"), r["text"]), None
                else:
                    prompt, g = self.process_prompt(r["text"], r.get("prompt_speech_path"), r.get("prompt_text"), r.get("prompt_tokens"))
                globals_[i] = g
                ids = self.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
                d = _request_sampling(r, self.speech_token_ids, self._eos, self.model.cfg.vocab_size)
                if FORK_KEY in r:
                    d = dict(d or {}, **{FORK_KEY: forks[i]})
                yield i, ids, min(max_new_tokens, self._max_positions - len(ids) - decode_stride), self._eos, d

        def vocode_takes(i, takes):   # one ragged vocoder call for all takes of request i
            rows, infos = [], []
            for toks in takes:
                lps = None
                if isinstance(toks, tuple):
                    toks, lps = toks
                toks = self._cut_eos(toks)
                rows.append(self._speech_row(i, toks, globals_[i]))
                infos.append(None if lps is None else _lp_info(toks, lps[: len(toks)]))
            wav, lens = self._vocode_rows(rows)
            wav, n = finished(i, wav, lens, True)
            wav = wav.cpu().numpy()
            return [(wav[b, : n[b]].copy(), infos[b]) if infos[b] is not None else wav[b, : n[b]].copy() for b in range(len(rows))]

        def finished(i, wav, lens, takes):   # the vocoded rows of request i at its tempo and loudness target, still on the device
            wav, n = self._tempo_rows(wav, [f * hop for f in lens], [rates[i]] * len(lens), pitches=[shifts[i]] * len(lens))
            if goals[i] is None and lims[i] is None:
                return wav, n
            wav = wav.contiguous()
            stats, lstats = self._level_rows(wav, n, [goals[i]] * len(lens), [lims[i]] * len(lens), peak_ceiling, max_gain_db, reach)
            got, lim = self._level_info(stats, lstats, [goals[i]] * len(lens), [lims[i]] * len(lens))
            if goals[i] is not None:
                self.last_loudness[i] = got if takes else got[0]
            if lims[i] is not None:
                self.last_limiter[i] = lim if takes else lim[0]
            return wav, n

        for i, toks in self.model.serve(llm_requests(), max_live=self._max_batch, decode_stride=decode_stride,
                                        return_log_probs=return_log_probs):
            if i in forks:
                yield i, vocode_takes(i, toks)
                continue
            lps = None
            if isinstance(toks, tuple):   # a flagged request: (tokens, log-probabilities)
                toks, lps = toks
            toks = self._cut_eos(toks)
            wav, lens = self._vocode_rows([self._speech_row(i, toks, globals_[i])])
            wav, n = finished(i, wav, lens, False)
            w = wav[0, : n[0]].cpu().numpy().copy()
            if lps is None:
                yield i, w
            else:
                yield i, w, _lp_info(toks, lps[: len(toks)])

    @torch.no_grad()
    def serve_stream(self, requests, temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *, do_sample: bool = True,
                     max_new_tokens: int = 3000, seed: Optional[int] = None, decode_stride: int = 8,
                     audio_chunk_duration: float = 1.0, max_audio_chunk_duration: float = 30.0,
                     audio_chunk_size_scale_factor: float = 8.0, audio_chunk_overlap_duration: float = 0.1,
                     max_open: Optional[int] = None, max_ahead: Optional[float] = None, resume_ahead: Optional[float] = None,
                     clock=None, pacer: Optional[Pacer] = None, output_sample_rate: Optional[int] = None, joined: bool = False,
                     tempo: Optional[float] = None, loudness: Optional[float] = None, peak_ceiling: float = PEAK_CEILING,
                     max_gain_db: float = 20.0, max_slew_db: float = 1.0, limiter: Optional[str] = None,
                     stream_limiter: Optional[str] = None, limiter_lookahead_ms: float = 2.5, limiter_release_ms: float = 25.0,
                     pitch_shift: Optional[float] = None, stream_pitch_shift: Optional[float] = None):
        """``serve`` and ``inference_stream`` at once (the reference's deployment: in-flight batching with the decoupled chunk loop
        answering every live request, run.sh:49-65, model.py:347-385): ``requests`` is an iterable of the dicts ``serve`` takes;
        yields ``(index, chunk_waveform, last)``, a request's chunks in order, cut and overlapped as ``inference_stream`` cuts
        them (join with ``streaming.crossfade``), while up to ``max_batch`` requests are live.  Requests enter free slots as in
        ``serve`` (one admission fills all free slots; budget ``max_positions - len(ids) - decode_stride``), so the sampling,
        penalty, ``allowed_token_ids`` and ``speech_tokens_only`` keys work per request, and a request's tokens -- cut at the
        first eos -- are those of the admission path for that request alone.  Every chunk is the vocoder's output for that
        chunk's tokens alone, bit for bit, whoever else is live: the ready chunks of all requests go through ONE
        ``detokenize_rows`` call per poll.  Between polls (every ``decode_stride`` steps) only the new ids cross to the host
        (``SparkLLM.poll``).  The vocoder call runs on a HIP stream of its own -- its inputs come from the host, so it waits
        for nothing of the LLM, and the LLM's stream never waits for it -- and the next ``decode_stride`` steps are enqueued
        before the host waits for the waveforms.  ``num_return_sequences`` and ``return_log_probs`` are refused (ValueError,
        before anything reaches the device).

        Parking (``streaming.Pacer``): with ``max_open`` > ``max_batch`` and ``max_ahead`` (seconds) given, up to ``max_open``
        requests are open at once.  After a poll, a live request whose lead -- audio yielded minus the ``clock`` time since its
        first chunk -- exceeds ``max_ahead`` gives its row to a waiting one: its sequence is parked (one ``SparkLLM.park`` per
        poll) while its chunks keep coming out; it is resumed (``restore_slots``, one call per poll, before the admission of
        new requests) once its lead has fallen below ``resume_ahead`` (default ``max_ahead / 2``), or as soon as a row would
        otherwise idle.  ``clock``: a callable returning seconds (default ``time.monotonic``).  The defaults (``max_open``
        None) are the loop without any of this: no save, no restore, no extra kernel or round trip; ``max_ahead`` without
        ``max_open > max_batch`` is accepted and inert.  Guarantee: a request's chunks -- samples, boundaries and ``last``
        flags -- are bit for bit those of the same call without parking, which are those of the request alone: a parked
        sequence comes back with every bit of its state, whatever the schedule did to it, greedy and sampled with any seed
        alike.  ``pacer``: a ``Pacer`` of the caller's, built for this ``max_batch``, in place of the four keywords (ValueError if
        both are given); its ``parks`` / ``resumes`` then tell the caller what the schedule did.  Nothing of a call is kept on
        ``self``.  The chunks are at ``sample_rate``: with ``joined=False`` a given ``output_sample_rate`` is refused (ValueError),
        as in ``inference_stream``.

        ``joined=True``: yields ``(index, piece, last)`` with contiguous, playable float32 pieces -- a listener plays a request's
        pieces one after the other; a piece may be empty, and ``last`` is on exactly one piece of a request.  The vocoder's rows
        stay on the device: the join (include/sparkmi.h, smi_join_*; ``audio.StreamJoiner``) runs on the vocoder's own stream
        right behind ``detokenize_rows``, one launch per poll (two in a poll in which a request has both its last full chunk
        and its flush ready), and only the pieces cross to the host -- the overlaps no longer travel.  Per request the pieces'
        concatenation is ``crossfade`` of its ``joined=False`` chunks cast to float32, bit for bit (``semantic tokens * hop``
        samples); with ``output_sample_rate`` (accepted here; None or ``sample_rate``: the model's rate) it is, bit for bit,
        what ``inference_batch``'s resampler gives for that joined waveform, whoever else is live, with or without parking.
        The joiner's state is keyed by request, not by KV slot, so park and resume do not touch it; it has
        max(``max_open``, ``max_batch``) stream slots -- the requests that can be admitted and not yet through their last
        chunk at once, since a request's last chunk is pushed in the poll that retires it -- so the slots cannot run out.  The
        ``Pacer`` counts frames yielded as without it.  (The joiner's handle stays on ``self`` for the next call with the same
        sizes and rate; its slots are all freed when a call begins, so nothing of a request outlives its call.)  Refused
        (ValueError, before any device call) if the first chunk is shorter than two overlaps.

        ``loudness`` and a request's own ``loudness`` key, which overrides it (LUFS; None everywhere: nothing new is built or
        launched and every piece keeps its bits), need ``joined=True``; with ``joined=False`` either is refused (ValueError).
        Every request's stream then goes through a loudness stream of its own (``inference_stream`` describes the running
        gain; include/sparkmi.h, smi_louds_*; ``audio.StreamLoudness``) behind the tempo stage and before the resampler with
        state, five launches more per poll; a request without a target is measured and copied.  The stage holds back up to
        500 ms of a request and keeps its total; the ``Pacer`` goes on counting the lengths behind the tempo stage.  After a
        request's last piece ``self.last_loudness[index]`` holds its entry as in ``inference_stream`` (one 32-byte copy).
        Whether a call has the stage is settled when it begins, as for ``tempo``.

        ``tempo`` and a request's own ``tempo`` key, which overrides it (0.5 .. 2.0; None or 1.0 everywhere: nothing new is
        built or launched and every piece keeps its bits), need ``joined=True``; with ``joined=False`` either is refused
        (ValueError).  Every request's joined stream then goes through a tempo stream of its own (include/sparkmi.h,
        smi_tempos_*; ``audio.StreamTempo``) behind the crossfade and, with ``output_sample_rate``, through the resampler with
        state behind that -- all on the vocoder's stream, two launches more per poll (four with a rate), the rows never
        leaving the device.  A request without a tempo in such a call goes through a stream at 1/1, which copies with no
        latency.  Per request the pieces' concatenation is, bit for bit, ``DeviceAudio.tempo_rows`` of its pieces without
        tempo (then ``resample_rows`` of that), whoever else is live, with or without parking: the stages' state is keyed by
        request like the joiner's, and a parked request's tempo stream stays open.  The ``Pacer`` then counts the seconds a
        listener receives: the scaled piece's length at the model's rate.  Whether a call has the stages is settled when it
        begins, from ``tempo`` and, where ``requests`` is a list, its requests; a request that brings a tempo of its own from
        an iterator into a call without them is refused (ValueError): pass a list, or a ``tempo`` for the call.

        ``stream_limiter`` and a request's own ``stream_limiter`` key, which overrides it (None everywhere: nothing new is built
        or launched and every piece keeps its bits), need ``joined=True``; with ``joined=False`` either is refused (ValueError).
        Every request's stream then goes through a limiter stream of its own (``inference_stream`` describes it;
        include/sparkmi.h, smi_limits_*; ``audio.StreamLimiter``) behind the loudness stage and before the resampler with state,
        three launches more per poll, with max(``max_open``, ``max_batch``) slots, so a parked request keeps its slot.  A
        request with a limiter has its loudness stream opened without a ceiling, as in ``inference_batch``.  A request without
        one in a call that has the stage is copied through it: its stream is opened in the "sample" mode under a ceiling that
        cannot bind, which gives every sample back bit for bit, A + R + 10 samples later.  The ``Pacer`` goes on counting the
        lengths behind the tempo stage.  After a request's last piece ``self.last_limiter[index]`` holds its entry as in
        ``inference_stream`` (one 32-byte copy; None for a request without a limiter).  Whether a call has the stage is settled
        when it begins, as for ``tempo``; a request that brings a ``stream_limiter`` of its own from an iterator into a call
        without it is refused (ValueError).

        ``limiter`` and a request's own ``limiter`` key are refused (ValueError), joined or not: they name the limiter of whole
        utterances; the streaming form is asked for by ``stream_limiter``.  ``pitch_shift`` and a request's own ``pitch_shift``
        key are refused (ValueError), joined or not: the batch calls take it; the streaming form is asked for by
        ``stream_pitch_shift``.

        ``stream_pitch_shift`` and a request's own ``stream_pitch_shift`` key, which overrides it (semitones, -12.0 .. 12.0, as
        ``audio.pitch_ratio`` rounds them; None, 0 or a ratio of 1/1 everywhere: nothing new is built or launched), need
        ``joined=True``; without it they are refused (ValueError).  In a call that has a pitched request the pitch stage
        (include/sparkmi.h, smi_pitchs_*; ``audio.StreamPitch``) takes the tempo stage's place for every
        request: one stretch pass serves a request's tempo and pitch, and a request without a pitch goes through at the ratio
        1/1, which is the tempo stream's bits (a copy with no latency where it has no tempo either).  Per request the pieces'
        concatenation is, bit for bit, ``DeviceAudio.pitch_rows`` of its pieces without the shift, whoever else is live, with or
        without parking: the state is keyed by request.  Loudness, ``stream_limiter`` and ``output_sample_rate`` see the shifted
        stream; the ``Pacer`` goes on counting the lengths behind this stage.  Whether a call has the stage is settled when it
        begins, as for ``tempo``; a request that brings a shift of its own from an iterator into a call without the stage is
        refused (ValueError).  The formants move with the pitch."""
        self._no_stream_limiter(limiter, "serve_stream")
        self._no_stream_pitch(pitch_shift, "serve_stream")
        if not joined:
            self._no_stream_pitch_form(stream_pitch_shift, "serve_stream")
            self._no_stream_tempo(tempo, "serve_stream")
            self._no_stream_loudness(loudness, "serve_stream")
            self._no_stream_limiter_form(stream_limiter, "serve_stream")
            self._no_stream_rate(output_sample_rate, "serve_stream")
        call_mode = self._stream_limiter_mode({}, stream_limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        modes: Dict[int, Optional[str]] = {}   # request index -> its streaming limiter's mode, None without one
        call_rate = self._tempo_ratios([{}], tempo)[0]
        call_shift = self._stream_pitch_ratios([{}], stream_pitch_shift)[0]
        shifts: Dict[int, Optional[Tuple[int, int]]] = {}   # request index -> its pitch shift as a frequency ratio (p, q), None without one
        call_target = self._loudness_targets([{}], loudness, peak_ceiling, max_gain_db)[0]
        self._check_slew(max_slew_db)
        rates: Dict[int, Tuple[int, int]] = {}   # request index -> its tempo as (p, q), (1, 1) without one
        targets: Dict[int, Optional[float]] = {}   # request index -> its loudness target, None without one

        def checked(reqs):   # a request's keys, checked before it reaches the device
            for i, r in enumerate(reqs):
                staged_keys = (TEMPO_KEY, LOUDNESS_KEY, STREAM_LIMITER_KEY, STREAM_PITCH_SHIFT_KEY)
                for k in (FORK_KEY,) + (() if joined else staged_keys) + tuple(LOGPROB_KEYS):
                    if k in r:
                        raise ValueError(f"request {i}: {k} is not supported by serve_stream" + (
                            " with overlapping chunks; pass joined=True" if k in staged_keys else ""))
                if r.get(LIMITER_KEY) is not None:
                    self._no_stream_limiter(r[LIMITER_KEY], f"request {i}: serve_stream")
                if r.get(PITCH_SHIFT_KEY) is not None:
                    self._no_stream_pitch(r[PITCH_SHIFT_KEY], f"request {i}: serve_stream")
                _request_seq(r, self._eos, self.model.cfg.vocab_size, f"request {i}")
                rates[i] = self._tempo_ratios([r], tempo, i)[0] or (1, 1)
                shifts[i] = self._stream_pitch_ratios([r], stream_pitch_shift, i)[0]
                try:
                    targets[i] = self._loudness_targets([r], loudness, peak_ceiling, max_gain_db)[0]
                except ValueError as e:
                    raise ValueError(str(e).replace("request 0:", f"request {i}:", 1)) from None
                modes[i] = self._stream_limiter_mode(r, stream_limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms,
                                                     f"request {i}: ")
                yield r

        staged, leveled, limited = call_rate is not None, call_target is not None, call_mode is not None
        pitched = call_shift is not None
        if isinstance(requests, (list, tuple)):   # a whole list is checked before anything runs
            for _ in checked(requests):
                pass
            staged = staged or any(v != (1, 1) for v in rates.values())
            leveled = leveled or any(v is not None for v in targets.values())
            limited = limited or any(v is not None for v in modes.values())
            pitched = pitched or any(v is not None for v in shifts.values())
        decode_stride = int(decode_stride)
        if decode_stride < 1:
            raise ValueError("decode_stride must be >= 1")
        voc = self.audio_tokenizer.model
        ntok, hop = voc.cfg.spk_token_num, voc.hop
        if pacer is None:
            max_open, max_ahead, resume_ahead = _stream_pacing(self._max_batch, max_open, max_ahead, resume_ahead)
            pacer = Pacer(self._max_batch, max_open, max_ahead, resume_ahead, self.sample_rate // hop, clock)
        else:
            if any(v is not None for v in (max_open, max_ahead, resume_ahead, clock)):
                raise ValueError("pacer= takes the place of max_open, max_ahead, resume_ahead and clock: give one or the other")
            if not isinstance(pacer, Pacer) or pacer.max_batch != self._max_batch:
                raise ValueError(f"pacer must be a streaming.Pacer for max_batch={self._max_batch}")
            max_open = pacer.max_open
        overlap = math.ceil(audio_chunk_overlap_duration * (self.sample_rate // hop))   # frames a chunk shares with its predecessor
        mux = StreamMux(ntok, self._map, self._parse, frame_rate=self.sample_rate // hop,
                        audio_chunk_duration=audio_chunk_duration, max_audio_chunk_duration=max_audio_chunk_duration,
                        audio_chunk_size_scale_factor=audio_chunk_size_scale_factor,
                        audio_chunk_overlap_duration=audio_chunk_overlap_duration)
        sched_args = (audio_chunk_duration, max_audio_chunk_duration, audio_chunk_size_scale_factor, audio_chunk_overlap_duration)
        stages = None
        if joined and (staged or pitched or leveled or limited):
            stages = self._stream_stages("serve_stream", output_sample_rate, max(int(max_open), self._max_batch), *sched_args,
                                         loudness=leveled, limiter=(limiter_lookahead_ms, limiter_release_ms) if limited else None,
                                         pitch=pitched)
            joiner = stages[0]
            if leveled:
                self.last_loudness = {}
            if limited:
                self.last_limiter = {}
        else:
            joiner = self._stream_joiner("serve_stream", output_sample_rate, max(int(max_open), self._max_batch), *sched_args) if joined else None
        if getattr(self, "_voc_stream", None) is None:
            self._voc_stream = torch.cuda.Stream(device=self.device)
        vs = self._voc_stream

        def llm_requests():
            for i, r in enumerate(checked(requests)):
                if stages is None and rates[i] != (1, 1):
                    raise ValueError(f"request {i}: a tempo of its own from an iterator of requests, in a serve_stream call that began "
                                     "without the tempo stages; pass the requests as a list, or a tempo for the call")
                if not pitched and shifts[i] is not None:
                    raise ValueError(f"request {i}: a stream_pitch_shift of its own from an iterator of requests, in a serve_stream "
                                     "call that began without the pitch stage; pass the requests as a list, or a stream_pitch_shift "
                                     "for the call")
                if (stages is None or stages[2] is None) and targets[i] is not None:
                    raise ValueError(f"request {i}: a loudness of its own from an iterator of requests, in a serve_stream call that "
                                     "began without the loudness stage; pass the requests as a list, or a loudness for the call")
                if (stages is None or stages[3] is None) and modes[i] is not None:
                    raise ValueError(f"request {i}: a stream_limiter of its own from an iterator of requests, in a serve_stream call "
                                     "that began without the limiter stage; pass the requests as a list, or a stream_limiter for "
                                     "the call")
                if r.get("gender") is not None:
                    prompt, g = self.process_prompt_control(r["gender"], r.get("pitch"), r.get("speed"), r["text"]), None
                else:
                    prompt, g = self.process_prompt(r["text"], r.get("prompt_speech_path"), r.get("prompt_text"), r.get("prompt_tokens"))
                    g = torch.as_tensor(g).reshape(-1).tolist()
                    if len(g) != ntok:
                        raise ValueError(f"request {i}: {len(g)} global tokens, the speaker encoder needs {ntok}")
                ids = self.tokenizer([prompt], return_tensors="pt").input_ids[0].tolist()
                budget = min(max_new_tokens, self._max_positions - len(ids) - decode_stride)
                if budget < 1:
                    raise ValueError(f"request {i}: a prompt of {len(ids)} tokens leaves no room in max_positions={self._max_positions}")
                yield i, ids, budget, g, _request_sampling(r, self.speech_token_ids, self._eos, self.model.cfg.vocab_size)

        def vocode(chunks):   # every ready chunk of every request in one ragged call, enqueued on the vocoder's own stream
            rows = [c for c in chunks if c[2]]
            wav = None
            if rows:
                lens = [len(c[2]) for c in rows]
                sem_t = torch.zeros((len(rows), max(lens)), dtype=torch.long)
                for b, c in enumerate(rows):
                    sem_t[b, : lens[b]] = torch.tensor(c[2])
                glob_t = torch.tensor([mux.global_ids(c[0]) for c in rows], dtype=torch.long).unsqueeze(1)
                with torch.cuda.stream(vs):
                    wav = voc.detokenize_rows(sem_t, glob_t, lengths=lens)
            if joiner is not None:   # the join, right behind the vocoder on its stream: the rows never leave the device
                with torch.cuda.stream(vs):
                    x = wav.squeeze(1) if wav is not None else torch.zeros((len(chunks), 1), dtype=torch.float32, device=self.device)
                    if wav is not None and len(rows) != len(chunks):   # an empty last chunk gets a row of its own (zero overlap only)
                        at = iter(range(len(rows)))
                        idx = torch.tensor([next(at) if c[2] else len(rows) for c in chunks], device=self.device)
                        x = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=torch.float32, device=self.device)])[idx].contiguous()
                    if stages is not None:   # crossfade, tempo and the resampler, each with its state, one behind the other
                        return chunks, (x,) + self._staged_push(stages, x, [(c[0], len(c[2]) * hop, c[3]) for c in chunks])
                    out, n_out = joiner.push(x, [(c[0], len(c[2]) * hop, c[3]) for c in chunks])
                return chunks, (x, out, n_out)
            return chunks, wav

        def collect_joined(job):
            chunks, (_, out, *rest) = job
            at, n_out, heard, final, final_lim = rest if stages is not None else ({b: b for b in range(len(chunks))}, rest[0], None, {}, {})
            with torch.cuda.stream(vs):
                out = out.cpu().numpy()
                for b, row in final.items():   # behind a request's last piece
                    self.last_loudness[chunks[b][0]] = self._stream_loudness_info(row.cpu().tolist())
                for b, row in final_lim.items():
                    key = chunks[b][0]
                    self.last_limiter[key] = None if modes[key] is None else self._stream_limiter_info(row.cpu().tolist())
            for b, (key, index, sem, last) in enumerate(chunks):
                if pacer.active:
                    frames = max(0, len(sem) - (overlap if index else 0))
                    if heard is None:
                        pacer.yielded(key, frames)
                    else:                 # what the listener receives: the scaled piece at the model's rate
                        pacer.yielded(key, frames, heard[b] / self.sample_rate)
                    if last:
                        pacer.close(key)
                yield key, (out[at[b], : n_out[b]].copy() if b in at else np.zeros(0, dtype=np.float32)), last

        def collect(job):     # the host waits for the vocoder's stream only
            if joiner is not None:
                yield from collect_joined(job)
                return
            chunks, wav = job
            if wav is not None:
                with torch.cuda.stream(vs):
                    wav = wav.squeeze(1).cpu().numpy()
            b = 0
            for key, index, sem, last in chunks:
                if pacer.active:
                    pacer.yielded(key, max(0, len(sem) - (overlap if index else 0)))
                    if last:          # nothing more is yielded for it: the pacer forgets the request here, not at its retirement
                        pacer.close(key)
                if sem:
                    yield key, wav[b, : len(sem) * hop].copy(), last
                    b += 1
                else:
                    yield key, np.zeros(0, dtype=np.float32), last

        self.model.set_sampling(do_sample, temperature, int(top_k), float(top_p), seed)
        it = llm_requests()
        pending = next(it, None)
        live: Dict[int, list] = {}    # slot -> [index, budget, tokens read so far]
        parked: Dict[int, tuple] = {}  # index -> (snapshot, its live entry): open requests that hold no row (Pacer)
        started, job = False, None
        try:
            while pending is not None or live or parked:
                # free rows go to the parked requests that are running out of lead, then to new requests, then to any parked one
                back = pacer.to_resume(list(parked), self._max_batch - len(live), True) if parked else []
                batch = []
                while (pending is not None and len(live) + len(back) + len(batch) < self._max_batch
                       and len(live) + len(parked) + len(batch) < max_open):
                    batch.append(pending)
                    pending = next(it, None)
                if parked:
                    rest = [k for k in parked if k not in back]
                    back += pacer.to_resume(rest, self._max_batch - len(live) - len(back) - len(batch), False)
                if back:              # ONE restore, ahead of the admission; a snapshot is dropped once its request is back
                    entries = [parked.pop(k) for k in back]
                    for slot, (_, entry) in zip(self.model.restore_slots([e[0] for e in entries]), entries):
                        live[slot] = entry
                    del entries
                if batch:             # all free slots are filled by ONE admission, as SparkLLM.serve does
                    if not started:
                        self.model.session_begin(self._eos)
                        started = True
                    slots = self.model.admit([r[1] for r in batch], [r[4] for r in batch])
                    for slot, r in zip(slots, batch):
                        live[slot] = [r[0], int(r[2]), 0]
                        mux.open(r[0], r[3])
                        if stages is not None:   # (host only; a request without a tempo copies through at 1/1)
                            with torch.cuda.stream(vs):   # (a pitched request's taps travel on the stream its pushes go to)
                                self._open_scale(stages[1], r[0], rates[r[0]], shifts[r[0]])
                            if stages[2] is not None:   # (host only; a request without a target is measured and copied)
                                stages[2].open(r[0], targets[r[0]], max_gain_db, peak_ceiling if modes[r[0]] is None else NO_CEILING,
                                               max_slew_db)
                            if stages[3] is not None:   # (host only; a request without a limiter is copied through, A + R + 10 late)
                                if modes[r[0]] is None:
                                    stages[3].open(r[0], "sample", NO_CEILING)
                                else:
                                    stages[3].open(r[0], modes[r[0]], peak_ceiling)
                self.model.decode(decode_stride)   # enqueued: it runs while the host collects the previous poll's chunks
                if job is not None:
                    yield from collect(job)
                    job = None
                order = list(live)
                cap = decode_stride + (1 if any(live[s][2] == 0 for s in order) else 0)   # (+ the token the admission emitted)
                got = self.model.poll(order, [live[s][2] for s in order], cap)
                ready, leave = [], []
                for slot, (new, count, fin) in zip(order, got):
                    key, budget, off = live[slot]
                    new = new[: budget - off]
                    live[slot][2] = off + len(new)
                    done = (bool(fin) or count >= budget) and live[slot][2] >= min(count, budget)   # (and every id of it is read)
                    ready += mux.push(key, new, done)
                    if done:
                        leave.append(slot)
                if ready:
                    job = vocode(ready)
                if leave:             # their last chunks are flushed (mux.push above); their rows are dropped on the device
                    self.model.retire_many(leave)
                    for slot in leave:
                        mux.close(live.pop(slot)[0])
                if pacer.active and live:   # the requests far enough ahead of their listeners make room for the waiting ones
                    by_key = {live[s][0]: s for s in live}
                    out = [by_key[k] for k in pacer.to_park(list(by_key), list(parked), pending is not None)]
                    if out:           # ONE save + retire_many; their mux entries stay open, their ready chunks are vocoded as usual
                        for slot, blob in zip(out, self.model.park(out)):
                            entry = live.pop(slot)
                            parked[entry[0]] = (blob, entry)
            if job is not None:
                yield from collect(job)
                job = None
        finally:
            parked.clear()     # the snapshots of requests that never resumed go with the generator
            vs.synchronize()   # an abandoned stream leaves no vocoder work behind (the handle's scratch is shared with detokenize)

    # ------------------------------------------------------------------ long text: sentences as rows, trimmed and joined on the device
    def _long_pieces(self, text, prompt_speech_path, prompt_text, gender, pitch, speed, temperature, top_k, top_p, do_sample,
                     max_new_tokens, seed, prompt_tokens, keys: dict, max_width, min_width, pause, trim, trim_threshold, fade, eager: bool,
                     info: dict, loudness=None, peak_ceiling=PEAK_CEILING, max_gain_db=20.0, tempo=None, limiter=None,
                     limiter_lookahead_ms=2.5, limiter_release_ms=25.0, pitch_shift=None):
        """The engine of ``inference_long`` and ``inference_long_stream``: yields (first sentence, joined [total] float32 on the
        device, [(offset in it, gap, length) per sentence]) for runs of consecutive sentences in text order -- with ``eager``
        as soon as the next sentence due and those behind it are done, else in runs of ``max_batch`` once all are done.  Fills
        ``info``.  With ``tempo``, every sentence's trimmed piece is time-scaled on its own into a row of its own; with
        ``loudness``, every piece (scaled or not) is brought to that programme loudness in place before the assembly; with
        ``limiter``, every piece goes through the look-ahead limiter on its own span there as well (``_level_rows``).
        With ``pitch_shift`` the pitch stage takes the tempo stage's place: every trimmed piece on its own, in one pass.
        Everything is checked before anything reaches the device."""
        check_loudness(loudness, peak_ceiling, max_gain_db)
        mode, reach = self._limiter_modes([{}], limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        mode = mode[0]
        rate = self._tempo_ratios([{}], tempo)[0]
        shift = self._pitch_ratios([{}], pitch_shift)[0]
        from .longform import control_prefix, control_prompt_ids, ready_run, sentence_seeds, split_text, trim_params
        sentences = split_text(text, max_width, min_width)
        for name, v in (("pause", pause), ("fade", fade), ("trim_threshold", trim_threshold)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
                raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
        n_sent, sr, decode_stride = len(sentences), int(self.sample_rate), 8
        gap, fade_n = int(round(pause * sr)), int(round(fade * sr))
        window, step, margin = trim_params(sr)
        seeds = sentence_seeds(seed, n_sent)
        reqs = [dict(keys, text=s, **({} if seeds[k] is None else {"seed": seeds[k]})) for k, s in enumerate(sentences)]
        sampling = [_request_sampling(r, self.speech_token_ids, self._eos, self.model.cfg.vocab_size) for r in reqs]
        tokenize = lambda p: self.tokenizer([p], return_tensors="pt").input_ids[0].tolist()   # noqa: E731
        voc = self.audio_tokenizer.model
        hop = voc.hop
        if gender is None:    # voice cloning: the prompt is encoded once, every sentence's prompt carries its tokens
            if prompt_tokens is None:
                prompt_tokens = self.audio_tokenizer.tokenize(prompt_speech_path)
            glob = torch.as_tensor(prompt_tokens[0]).reshape(-1).long()
            sessions = [list(range(n_sent))]
        else:                 # voice creation: sentence 0 alone decides the style values and the speaker tokens of all
            build_control_prompt(gender, pitch, speed, sentences[0])
            glob = None
            sessions = [[0]] + ([list(range(1, n_sent))] if n_sent > 1 else [])
        prefix: List[int] = []
        budgets: Dict[int, int] = {}
        info.update(sentences=sentences, token_ids=[None] * n_sent, bounds=[None] * n_sent, offsets=[None] * n_sent, truncated=[], silent=[])
        if loudness is not None:
            info.update(loudness=[None] * n_sent, gain=[None] * n_sent, limited=[None] * n_sent)
        if mode is not None:
            info.update(limiter=[None] * n_sent)
        if rate is not None:
            info.update(tempo_lengths=[None] * n_sent)
        audio = self._device_audio()
        tokens: Dict[int, List[int]] = {}
        state = {"due": 0, "total": 0, "spoken": False}

        def llm_requests(ks):
            for k in ks:
                if gender is None:
                    ids = tokenize(self.process_prompt(sentences[k], None, prompt_text, prompt_tokens)[0])
                else:
                    ids = control_prompt_ids(tokenize, gender, pitch, speed, sentences[k], prefix)
                budgets[k] = min(int(max_new_tokens), self._max_positions - len(ids) - decode_stride, self._max_frames)
                if budgets[k] < 1:
                    raise ValueError(f"sentence {k}: a prompt of {len(ids)} tokens leaves no room in max_positions={self._max_positions}")
                yield k, ids, budgets[k], self._eos, sampling[k]

        def flush(ks):   # consecutive sentences: one ragged vocoder call, their bounds, one assembly launch
            rows = [self._speech_row(k, tokens[k], glob) for k in ks]
            wav, lens = self._vocode_rows(rows)
            wav = wav.contiguous()
            n = [f * hop for f in lens]
            bounds = audio.trim_rows(wav, n, window, step, float(trim_threshold), margin) if trim else [(0, v) for v in n]
            gaps = []
            for a, b in bounds:
                gaps.append(gap if b > a and state["spoken"] else 0)
                state["spoken"] = state["spoken"] or b > a
            cut = bounds              # of the untrimmed rows: what info["bounds"] reports
            if rate is not None or shift is not None:   # each trimmed piece on its own: row k of the new rows is the whole piece
                wav, n = self._tempo_rows(wav, n, [rate] * len(ks), spans=bounds, pitches=[shift] * len(ks))
                bounds = [(0, v) for v in n]
                for k, v in zip(ks, n):
                    if rate is not None:
                        info["tempo_lengths"][k] = v
            offs, total = audio.concat_layout(bounds, gaps)
            stats = lstats = None
            goal = None if loudness is None else float(loudness)
            if goal is not None or mode is not None:   # each piece on its own trimmed span, in place, before the assembly
                stats, lstats = self._level_rows(wav, n, [goal] * len(ks), [mode] * len(ks), peak_ceiling, max_gain_db, reach, spans=bounds)
            out = None
            if total:
                out, _ = audio.concat_rows(wav, bounds, gaps, fade_n, n=n)
            if stats is not None or lstats is not None:      # (one small copy, like the bounds', behind everything that was enqueued)
                loud, lim = self._level_info(stats, lstats, [loudness] * len(ks), [mode] * len(ks))
                for k, d, e in zip(ks, loud, lim):
                    if d is not None:
                        info["loudness"][k], info["gain"][k], info["limited"][k] = d["loudness"], d["gain"], d["limited"]
                    if e is not None:
                        info["limiter"][k] = e
            for k, (a, b), o, g in zip(ks, cut, offs, gaps):
                info["bounds"][k], info["offsets"][k] = (a, b), state["total"] + o
                if b == a:
                    info["silent"].append(k)
            res = ks[0], out, [(o - g, g, b - a) for (a, b), o, g in zip(bounds, offs, gaps)]
            state["total"] += total
            state["due"] = ks[-1] + 1
            for k in ks:
                del tokens[k]
            return res

        for ks in sessions:
            self.model.set_sampling(do_sample, temperature, int(top_k), float(top_p), seed)
            for k, toks in self.model.serve(llm_requests(ks), max_live=self._max_batch, decode_stride=decode_stride):
                full = len(toks) >= budgets[k]
                toks = self._cut_eos(toks)
                if full and not any(e in toks for e in self._eos):
                    info["truncated"].append(k)
                info["token_ids"][k] = tokens[k] = list(toks)
                if gender is not None and k == 0:
                    prefix, gl = control_prefix(toks, self._map.sem, self._map.glob, voc.cfg.spk_token_num)
                    glob = torch.tensor(gl, dtype=torch.long)
                while eager:
                    run = ready_run(tokens, state["due"], self._max_batch)
                    if not run:
                        break
                    yield flush(run)
            while state["due"] < ks[-1] + 1:
                yield flush(ready_run(tokens, state["due"], self._max_batch))
        info["truncated"].sort()
        info["silent"].sort()

    def _long_keys(self, prompt_speech_path, gender, prompt_tokens, repetition_penalty, presence_penalty, frequency_penalty,
                   min_new_tokens, penalize_prompt, allowed_token_ids, speech_tokens_only, no_repeat_ngram_size) -> dict:
        """the request keys every sentence of a long text shares, as ``inference`` builds them for one utterance"""
        if gender is None and prompt_tokens is None and prompt_speech_path is None:
            raise ValueError("inference_long needs a voice: prompt_speech_path or prompt_tokens (cloning), or gender / pitch / speed (creation)")
        n_gram = ngram_size(no_repeat_ngram_size)
        return dict(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty, frequency_penalty=frequency_penalty,
                    min_new_tokens=min_new_tokens, penalize_prompt=penalize_prompt,
                    **({ALLOW_KEY: allowed_token_ids} if allowed_token_ids is not None else {}),
                    **({SPEECH_ONLY_KEY: speech_tokens_only} if speech_tokens_only else {}),
                    **({NGRAM_KEY: n_gram} if n_gram > 0 else {}))

    @torch.no_grad()
    def inference_long(self, text: str, prompt_speech_path: Path = None, prompt_text: str = None,
                       gender: str = None, pitch: str = None, speed: str = None,
                       temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *,
                       do_sample: bool = True, max_new_tokens: int = 3000, seed: Optional[int] = None,
                       prompt_tokens: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                       repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                       min_new_tokens: int = 0, penalize_prompt: bool = True, allowed_token_ids: Optional[Sequence[int]] = None,
                       speech_tokens_only: bool = False, no_repeat_ngram_size: int = 0,
                       max_width: int = 300, min_width: int = 20, pause: float = 0.25, trim: bool = True,
                       trim_threshold: float = 0.01, fade: float = 0.005, output_sample_rate: Optional[int] = None,
                       return_info: bool = False, loudness: Optional[float] = None, peak_ceiling: float = PEAK_CEILING,
                       max_gain_db: float = 20.0, tempo: Optional[float] = None, limiter: Optional[str] = None,
                       limiter_lookahead_ms: float = 2.5, limiter_release_ms: float = 25.0, pitch_shift: Optional[float] = None):
        """A text of any length -> one float32 waveform: the text is cut into sentences (``longform.split_text``: ``max_width``,
        ``min_width``), the sentences are generated with the same voice as the requests of one in-flight session (up to
        ``max_batch`` live; ``max_new_tokens`` is per sentence), vocoded in ragged calls, cut at their speech bounds
        (``trim``, ``trim_threshold``: ``remove_silence_on_both_ends``' arithmetic; include/sparkmi.h, smi_trim_rows) and joined
        in text order with ``pause`` seconds of silence between them and ``fade`` seconds of fade at every piece's edges
        (smi_concat_rows).  The waveforms stay on the device up to the one copy of the result; only the bounds (8 bytes a
        sentence) cross before it.

        Voice cloning: the prompt audio is encoded once (or ``prompt_tokens`` is taken as given); sentence k has the tokens of
        ``inference(sentence_k, ..., prompt_tokens=...)`` through the admission path.  Voice creation (``gender`` given):
        sentence 0 runs alone; the ids it generated before its first semantic token -- the style values and the global-token
        block -- are appended to the control prompt of every later sentence, which therefore continues from the same style and
        speaker tokens and generates semantic tokens only; all are vocoded with sentence 0's global tokens.  ValueError if
        sentence 0 gives no complete global block.  ``seed=s``: sentence k carries ``s + k``; None: the handle's key.

        ``output_sample_rate``: the joined waveform is resampled on the device (``audio.DeviceAudio.resample_rows``) before the
        copy.  ``return_info=True``: (waveform, info) with ``sentences``, ``token_ids`` (per sentence, up to and including its
        eos), ``bounds`` (per sentence, in samples of its untrimmed row), ``offsets`` (of the pieces in the joined waveform at the
        model's rate), ``truncated`` (the sentences that used their whole budget -- the room left in ``max_positions`` and
        ``max_frames`` bound it -- without an eos) and ``silent`` (those with an empty piece, which also get no pause).

        ``loudness`` (LUFS; None: the pieces as vocoded, no extra launch): every sentence is an independent generation and
        comes out at its own level, so each trimmed piece is brought to that programme loudness on its own (ITU-R BS.1770;
        include/sparkmi.h, smi_loud_rows / smi_gain_rows: trim, measure over the piece, scale in place, assemble) by a gain of at
        most ``max_gain_db`` that keeps its sample peak at or below ``peak_ceiling``; a silent sentence is untouched.  ``info``
        then also holds ``loudness`` (measured before the gain), ``gain`` and ``limited`` (None, "max_gain" or "ceiling") per
        sentence.

        ``tempo`` (0.5 .. 2.0; None or 1.0: no extra launch): every trimmed piece is time-scaled on its own at unchanged pitch
        (include/sparkmi.h, smi_tempo_rows) after the trim and before the loudness stage and the assembly.  ``pause`` and
        ``fade`` stay seconds of the joined waveform -- the silences are not scaled --, ``info["bounds"]`` stays in samples of
        the untrimmed row, ``info["tempo_lengths"]`` holds every scaled piece's length and ``info["offsets"]`` places the scaled
        pieces in the joined waveform.

        ``limiter`` (None: no extra launch, no bit changes; "true"; "sample"), ``limiter_lookahead_ms``, ``limiter_release_ms``
        as in ``inference_batch``: every piece goes through the look-ahead limiter (include/sparkmi.h, smi_limit_rows) on its
        own trimmed span, behind the loudness stage and before the assembly, so one click no longer holds a whole sentence
        under its target: with ``loudness`` a piece reaches the target (or ``max_gain_db``) and ``limited`` is None or
        "max_gain".  Every sample of every piece is at or under ``peak_ceiling``; ``info["limiter"]`` holds {``true_peak``,
        ``reduction_db``, ``limited_samples``} per sentence.

        ``pitch_shift`` (semitones, -12.0 .. 12.0; None or a ratio of 1/1: no extra launch) as in ``inference_batch``: every
        trimmed piece's pitch is moved on its own (include/sparkmi.h, smi_pitch_rows), in the tempo stage's place and pass; a
        piece keeps the length ``tempo`` alone gives it -- its own without one."""
        check_loudness(loudness, peak_ceiling, max_gain_db)
        self._tempo_ratios([], tempo)
        self._pitch_ratios([], pitch_shift)
        self._limiter_modes([], limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        out_ratio = self._output_ratio(output_sample_rate)
        keys = self._long_keys(prompt_speech_path, gender, prompt_tokens, repetition_penalty, presence_penalty, frequency_penalty,
                               min_new_tokens, penalize_prompt, allowed_token_ids, speech_tokens_only, no_repeat_ngram_size)
        info: dict = {}
        parts = [out for _, out, _ in self._long_pieces(text, prompt_speech_path, prompt_text, gender, pitch, speed, temperature, top_k, top_p,
                                                        do_sample, max_new_tokens, seed, prompt_tokens, keys, max_width, min_width, pause, trim,
                                                        trim_threshold, fade, False, info, loudness, peak_ceiling, max_gain_db, tempo,
                                                        limiter, limiter_lookahead_ms, limiter_release_ms, pitch_shift)
                 if out is not None]
        if not parts:
            wav = np.zeros(0, dtype=np.float32)
        else:
            joined = parts[0] if len(parts) == 1 else torch.cat(parts)   # (more sentences than max_batch: one run each)
            if out_ratio is not None:
                y, n_out = self._device_audio().resample_rows(joined.reshape(1, -1), [joined.numel()], [out_ratio[0]], [out_ratio[1]])
                joined = y[0, : n_out[0]]
            wav = joined.cpu().numpy().copy()
        return (wav, info) if return_info else wav

    @torch.no_grad()
    def inference_long_stream(self, text: str, prompt_speech_path: Path = None, prompt_text: str = None,
                              gender: str = None, pitch: str = None, speed: str = None,
                              temperature: float = 0.8, top_k: float = 50, top_p: float = 0.95, *,
                              do_sample: bool = True, max_new_tokens: int = 3000, seed: Optional[int] = None,
                              prompt_tokens: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                              repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                              min_new_tokens: int = 0, penalize_prompt: bool = True, allowed_token_ids: Optional[Sequence[int]] = None,
                              speech_tokens_only: bool = False, no_repeat_ngram_size: int = 0,
                              max_width: int = 300, min_width: int = 20, pause: float = 0.25, trim: bool = True,
                              trim_threshold: float = 0.01, fade: float = 0.005,
                              output_sample_rate: Optional[int] = None, loudness: Optional[float] = None,
                              peak_ceiling: float = PEAK_CEILING, max_gain_db: float = 20.0,
                              tempo: Optional[float] = None, limiter: Optional[str] = None, limiter_lookahead_ms: float = 2.5,
                              limiter_release_ms: float = 25.0, pitch_shift: Optional[float] = None) -> Iterator[np.ndarray]:
        """``inference_long`` piece by piece: yields contiguous float32 pieces in text order, sentence k's pause + trimmed and faded
        piece as soon as k and every sentence before it are done (an empty piece is not yielded).  At the model's rate the
        pieces' concatenation is ``inference_long``'s waveform bit for bit: a piece's bits are its own (include/sparkmi.h,
        smi_concat_rows).  With ``output_sample_rate`` the pieces go through a ``StreamJoiner`` with ``overlap = 0`` -- plain
        concatenation with the resampler's state kept across the pieces -- and the concatenation of what is yielded (the last
        piece is the resampler's flush) is bit for bit ``inference_long(..., output_sample_rate=...)``.  ``loudness`` /
        ``peak_ceiling`` / ``max_gain_db`` as in ``inference_long``: a sentence's loudness is measured over its own piece, so
        the pieces stay bit for bit those of ``inference_long``.  ``tempo`` as in ``inference_long``: a sentence's piece is
        scaled whole and on its own before it leaves, so no state crosses the pieces and the same holds.  ``limiter`` /
        ``limiter_lookahead_ms`` / ``limiter_release_ms`` as in ``inference_long``: a piece is limited whole and on its own
        span -- this is the batch limiter, not a streaming one --, so the same holds again.  ``pitch_shift`` as in
        ``inference_long``: a piece is shifted whole and on its own, so the same holds once more."""
        check_loudness(loudness, peak_ceiling, max_gain_db)
        self._pitch_ratios([], pitch_shift)
        self._limiter_modes([], limiter, peak_ceiling, limiter_lookahead_ms, limiter_release_ms)
        rate = self._tempo_ratios([{}], tempo)[0] or (1, 1)
        out_ratio = self._output_ratio(output_sample_rate)
        keys = self._long_keys(prompt_speech_path, gender, prompt_tokens, repetition_penalty, presence_penalty, frequency_penalty,
                               min_new_tokens, penalize_prompt, allowed_token_ids, speech_tokens_only, no_repeat_ngram_size)
        pieces = self._long_pieces(text, prompt_speech_path, prompt_text, gender, pitch, speed, temperature, top_k, top_p, do_sample,
                                   max_new_tokens, seed, prompt_tokens, keys, max_width, min_width, pause, trim, trim_threshold, fade, True, {},
                                   loudness, peak_ceiling, max_gain_db, tempo, limiter, limiter_lookahead_ms, limiter_release_ms,
                                   pitch_shift)
        joiner = None
        for _, out, spans in pieces:
            if out is None:
                continue
            if out_ratio is None:
                host = out.cpu().numpy()
                for start, g, length in spans:
                    if length:
                        yield host[start: start + g + length].copy()
                continue
            if joiner is None:   # (pieces of up to a pause and a whole vocoder row)
                from .audio import StreamJoiner
                key = (1, int(round(pause * self.sample_rate)) + tempo_len(self._max_frames * self.audio_tokenizer.model.hop, *rate), 0) + tuple(out_ratio)
                if getattr(self, "_joiners", None) is None:
                    self._joiners = {}
                if key not in self._joiners:
                    self._joiners[key] = StreamJoiner(*key, device=self.device)
                joiner = self._joiners[key]
                joiner.reset()
            for start, g, length in spans:
                if length:
                    y, n_out = joiner.push(out[start: start + g + length].reshape(1, -1), [(0, g + length, False)])
                    if n_out[0]:
                        yield y[0, : n_out[0]].cpu().numpy().copy()
        if joiner is not None:   # an empty last chunk empties the resampler
            y, n_out = joiner.push(torch.zeros((1, 1), dtype=torch.float32, device=self.device), [(0, 0, True)])
            if n_out[0]:
                yield y[0, : n_out[0]].cpu().numpy().copy()
