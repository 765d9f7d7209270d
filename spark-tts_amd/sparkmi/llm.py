"""SparkLLM -- the speech-token generator behind ``AutoModelForCausalLM.generate`` as the
reference calls it (``cli/SparkTTS.py:197-204``), running on the HIP kernels of ``smi_llm.hip``.

``generate`` keeps the HF call shape (``input_ids`` (B, P), ``attention_mask``,
``max_new_tokens``, ``do_sample``, ``eos_token_id``, ``pad_token_id``) and returns (B, P + N)
ids, prompt included, exactly like the reference expects when it slices the prompt off at
``cli/SparkTTS.py:207-210``.  Greedy by default; ``do_sample=True`` runs the reference's temperature → top-k →
top-p → multinomial chain on the device (``k_sample``).
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import warnings
from pathlib import Path
from typing import Iterable, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from . import _lib
from .arena import llm_cfg_struct, pack_llm_arena
from .config import LLMConfig


EosLike = Union[None, int, Iterable[int]]
# keys of a per-request sampling dict (SparkLLM.admit, generate_ragged, serve; SparkTTS.inference_batch / serve requests)
SAMPLING_KEYS = ("do_sample", "temperature", "top_k", "top_p", "seed")
# keys of its logits penalties, in the same dicts (smi_llm_admit_penalized; include/sparkmi.h states the semantics), and the
# values that leave a request unpenalised
PENALTY_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "min_new_tokens", "penalize_prompt")
PENALTY_NEUTRAL = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0)
# key of the per-token log-probabilities, in the same dicts (smi_llm_admit_logprobs; include/sparkmi.h states the semantics)
LOGPROB_KEYS = ("return_log_probs",)
# key of the allowed-token set, in the same dicts (smi_llm_admit_constrained; include/sparkmi.h states the semantics): an
# iterable of token ids, merged into sorted runs of consecutive ids (at most SMI_MAX_ALLOW_RANGES of them)
ALLOW_KEY = "allowed_token_ids"


def allow_ranges(ids, vocab_size: int, what: str = ALLOW_KEY) -> List[tuple]:
    """The sorted, disjoint half-open runs [lo, hi) of consecutive ids that make up the set ``ids``.  ValueError, before any
    device call, when the set is empty, holds a non-integer or an id outside [0, vocab_size), or needs more than
    ``SMI_MAX_ALLOW_RANGES`` runs."""
    if isinstance(ids, (str, bytes)) or not isinstance(ids, Iterable):
        raise ValueError(f"{what} must be an iterable of token ids, not {ids!r}")
    vals = []
    for v in ids:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {v!r} is not an integer token id")
        if not 0 <= int(v) < vocab_size:
            raise ValueError(f"{what}: id {int(v)} outside [0, {vocab_size})")
        vals.append(int(v))
    if not vals:
        raise ValueError(f"{what} is empty: nothing could be generated")
    runs: List[list] = []
    for v in sorted(set(vals)):
        if runs and runs[-1][1] == v:
            runs[-1][1] = v + 1
        else:
            runs.append([v, v + 1])
    if len(runs) > _lib.SMI_MAX_ALLOW_RANGES:
        raise ValueError(f"{what}: {len(runs)} runs of consecutive ids, at most {_lib.SMI_MAX_ALLOW_RANGES} are supported")
    return [tuple(r) for r in runs]


def allow_records(requests: Optional[Sequence[Optional[Mapping]]], n: int, vocab_size: int):
    """One ``smi_allow_params`` per prompt from the ``allowed_token_ids`` keys of the request dicts, or None when no request
    carries the key (the admission then keeps the route and bits it has without it).  A request without the key gets a record
    with no ranges (not constrained)."""
    if requests is None:
        return None
    requests = list(requests)
    if len(requests) != n:
        raise ValueError(f"sampling: {len(requests)} entries for {n} prompts")
    if not any(d is not None and d.get(ALLOW_KEY) is not None for d in requests):
        return None
    recs = (_lib.AllowParams * n)()
    for i, d in enumerate(requests):
        if d is None or d.get(ALLOW_KEY) is None:
            continue
        runs = allow_ranges(d[ALLOW_KEY], vocab_size, f"sampling[{i}].{ALLOW_KEY}")
        recs[i].n_ranges = len(runs)
        for r, (lo, hi) in enumerate(runs):
            recs[i].lo[r], recs[i].hi[r] = lo, hi
    return recs


# keys of the per-request sequence bias, banned and stop token sequences, in the same dicts (smi_llm_admit_biased;
# include/sparkmi.h states the semantics): sequence_bias = [(ids, bias), ...] (transformers' SequenceBiasLogitsProcessor; a
# bias is finite or -inf), bad_words_ids = [ids, ...] (= bias -inf: NoBadWordsLogitsProcessor), stop_sequences = [ids, ...]
SEQ_KEYS = ("sequence_bias", "bad_words_ids", "stop_sequences")


def _id_seq(ids, vocab_size: int, what: str) -> tuple:
    if isinstance(ids, (str, bytes)) or not isinstance(ids, Iterable):
        raise ValueError(f"{what} must be a sequence of token ids, not {ids!r}")
    out = []
    for v in ids:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {v!r} is not an integer token id")
        if not 0 <= int(v) < vocab_size:
            raise ValueError(f"{what}: id {int(v)} outside [0, {vocab_size})")
        out.append(int(v))
    if not 1 <= len(out) <= _lib.SMI_MAX_SEQ_LEN:
        raise ValueError(f"{what}: {len(out)} ids, a sequence holds 1..{_lib.SMI_MAX_SEQ_LEN}")
    return tuple(out)


def _seq_list(v, what: str) -> list:
    if isinstance(v, (str, bytes, Mapping)) or not isinstance(v, Iterable):
        raise ValueError(f"{what} must be a list, not {v!r}")
    return list(v)


def seq_entries(d: Optional[Mapping], vocab_size: int, what: str = "sampling"):
    """(bias entries [(ids, float32 bias)], stop sequences [ids]) of one request dict, checked: ``sequence_bias`` entries first,
    then ``bad_words_ids`` as bias -inf.  ValueError, before any device call, for a malformed list, a sequence of 0 or more
    than ``SMI_MAX_SEQ_LEN`` ids, an id outside the vocabulary, a bias that is NaN or +inf, a sequence listed twice, or more
    than ``SMI_MAX_BIAS_SEQS`` / ``SMI_MAX_STOP_SEQS`` entries."""
    bias, stops = [], []
    if d is None:
        return bias, stops
    if d.get("sequence_bias") is not None:
        for k, e in enumerate(_seq_list(d["sequence_bias"], f"{what}.sequence_bias")):
            if isinstance(e, (str, bytes)) or not isinstance(e, Sequence) or len(e) != 2:
                raise ValueError(f"{what}.sequence_bias[{k}] must be (ids, bias), not {e!r}")
            ids, b = e
            if isinstance(b, (bool, np.bool_)) or not isinstance(b, (int, float, np.integer, np.floating)):
                raise ValueError(f"{what}.sequence_bias[{k}]: bias {b!r} is not a number")
            b = np.float32(b)
            if np.isnan(b) or b == np.inf:
                raise ValueError(f"{what}.sequence_bias[{k}]: bias must be finite or -inf, not {e[1]!r}")
            bias.append((_id_seq(ids, vocab_size, f"{what}.sequence_bias[{k}]"), b))
    if d.get("bad_words_ids") is not None:
        for k, ids in enumerate(_seq_list(d["bad_words_ids"], f"{what}.bad_words_ids")):
            bias.append((_id_seq(ids, vocab_size, f"{what}.bad_words_ids[{k}]"), np.float32(-np.inf)))
    if d.get("stop_sequences") is not None:
        for k, ids in enumerate(_seq_list(d["stop_sequences"], f"{what}.stop_sequences")):
            stops.append(_id_seq(ids, vocab_size, f"{what}.stop_sequences[{k}]"))
    if len(bias) > _lib.SMI_MAX_BIAS_SEQS:
        raise ValueError(f"{what}: {len(bias)} bias / banned sequences, at most {_lib.SMI_MAX_BIAS_SEQS} are supported")
    if len(stops) > _lib.SMI_MAX_STOP_SEQS:
        raise ValueError(f"{what}: {len(stops)} stop sequences, at most {_lib.SMI_MAX_STOP_SEQS} are supported")
    if len({ids for ids, _ in bias}) != len(bias):
        raise ValueError(f"{what}: a sequence is listed twice among sequence_bias / bad_words_ids")
    if len(set(stops)) != len(stops):
        raise ValueError(f"{what}: a sequence is listed twice among stop_sequences")
    return bias, stops


def seq_records(requests: Optional[Sequence[Optional[Mapping]]], n: int, vocab_size: int, eos_ids: Sequence[int] = ()):
    """One ``smi_seq_params`` per prompt from the ``SEQ_KEYS`` of the request dicts, or None when no request carries one (the
    admission then keeps the route and bits it has without them).  A request without a key gets a neutral record.  Every rule
    of ``smi_llm_admit_biased`` is checked here first (``seq_entries``), the survivor rule included: the request's
    ``allowed_token_ids`` (the vocabulary without the key) minus the last ids of its -inf entries must hold an id, and with
    ``min_new_tokens`` > 0 an id that is not one of ``eos_ids``."""
    if requests is None:
        return None
    requests = list(requests)
    if len(requests) != n:
        raise ValueError(f"sampling: {len(requests)} entries for {n} prompts")
    if not any(d is not None and any(d.get(k) is not None for k in SEQ_KEYS) for d in requests):
        return None
    recs = (_lib.SeqParams * n)()
    L = _lib.SMI_MAX_SEQ_LEN
    for i, d in enumerate(requests):
        bias, stops = seq_entries(d, vocab_size, f"sampling[{i}]")
        gone = {ids[-1] for ids, b in bias if b == -np.inf}
        if gone:
            allowed = None if d.get(ALLOW_KEY) is None else set(int(v) for v in d[ALLOW_KEY])
            size = vocab_size if allowed is None else len(allowed)
            if allowed is not None:
                gone &= allowed
            if size <= len(gone):
                raise ValueError(f"sampling[{i}]: the banned ids leave nothing the request could emit")
            if int(d.get("min_new_tokens", 0) or 0) > 0:
                gone |= {int(e) for e in eos_ids if 0 <= int(e) < vocab_size and (allowed is None or int(e) in allowed)}
                if size <= len(gone):
                    raise ValueError(f"sampling[{i}]: the banned ids leave only eos ids, which min_new_tokens bans")
        r = recs[i]
        r.n_bias, r.n_stop = len(bias), len(stops)
        for k, (ids, b) in enumerate(bias):
            r.bias_len[k], r.bias[k] = len(ids), float(b)
            for t, v in enumerate(ids):
                r.bias_ids[k * L + t] = v
        for k, ids in enumerate(stops):
            r.stop_len[k] = len(ids)
            for t, v in enumerate(ids):
                r.stop_ids[k * L + t] = v
    return recs


# key of a request's n-gram ban, in the same dicts (transformers' / TensorRT-LLM's no_repeat_ngram_size; smi_llm_admit_ngram;
# include/sparkmi.h states the semantics): an int 0 .. SMI_MAX_NGRAM, 0 = none
NGRAM_KEY = "no_repeat_ngram_size"


def ngram_size(v, what: str = NGRAM_KEY) -> int:
    """A ``no_repeat_ngram_size``: an int (a bool is refused) in 0 .. ``SMI_MAX_NGRAM``; ValueError otherwise, before any device
    call."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{what} must be an int, not {v!r}")
    if not 0 <= int(v) <= _lib.SMI_MAX_NGRAM:
        raise ValueError(f"{what}={int(v)} outside 0..{_lib.SMI_MAX_NGRAM}")
    return int(v)


def ngram_records(requests: Optional[Sequence[Optional[Mapping]]], n: int):
    """One int32 ``no_repeat_ngram_size`` per prompt from the ``NGRAM_KEY`` of the request dicts, or None when no request asks
    for a ban (no key, or 0 everywhere: the admission then keeps the route and bits it has without it).  Every value is checked
    here first (``ngram_size``); the survivor rule is the library's."""
    if requests is None:
        return None
    requests = list(requests)
    if len(requests) != n:
        raise ValueError(f"sampling: {len(requests)} entries for {n} prompts")
    sizes = np.zeros(n, dtype=np.int32)
    for i, d in enumerate(requests):
        if d is not None and d.get(NGRAM_KEY) is not None:
            sizes[i] = ngram_size(d[NGRAM_KEY], f"sampling[{i}].{NGRAM_KEY}")
    return sizes if sizes.any() else None


# key of a request's number of takes (TensorRT-LLM's num_return_sequences; smi_llm_admit_forked): SparkLLM.serve and SparkTTS
# requests take it out of the dict before its records are built
FORK_KEY = "num_return_sequences"


def num_returns(v, what: str = FORK_KEY) -> int:
    """A number of takes: an int >= 1 (a bool is refused); ValueError otherwise, before any device call."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or int(v) < 1:
        raise ValueError(f"{what} must be an int >= 1, not {v!r}")
    return int(v)


def expand_takes(sampling: Optional[Sequence[Optional[Mapping]]], n_return: Sequence[int]):
    """The per-take request dicts of a forked admission, prompt-major (prompt 0's takes, then prompt 1's, ...), or None when
    ``sampling`` is None.  A dict with its own ``seed`` gives take j the seed ``seed + j`` (mod 2^64) -- otherwise every take
    would draw the same tokens; every other key is copied as is."""
    if sampling is None:
        return None
    sampling = list(sampling)
    if len(sampling) != len(n_return):
        raise ValueError(f"sampling: {len(sampling)} entries for {len(n_return)} prompts")
    out: List[Optional[dict]] = []
    for d, k in zip(sampling, n_return):
        if d is not None and d.get(ALLOW_KEY) is not None and not isinstance(d[ALLOW_KEY], (list, tuple)):
            d = dict(d, **{ALLOW_KEY: tuple(d[ALLOW_KEY])})   # a one-shot iterable serves every take
        for key in SEQ_KEYS:                                  # the bias / banned / stop lists likewise: every take carries them
            if d is not None and d.get(key) is not None and not isinstance(d[key], (list, tuple)):
                d = dict(d, **{key: tuple(_seq_list(d[key], key))})
        for j in range(k):
            if d is None:
                out.append(None)
            elif d.get("seed") is not None:
                out.append(dict(d, seed=(int(d["seed"]) + j) % 2 ** 64))
            else:
                out.append(dict(d))
    return out


def logprob_flags(requests: Optional[Sequence[Optional[Mapping]]], n: int):
    """One int32 0/1 flag per prompt from the ``return_log_probs`` keys of the request dicts, or None when no request carries
    the key (the admission then keeps the route and bits it has without it).  The value must be a bool: anything else is
    refused here, before any device call."""
    if requests is None:
        return None
    requests = list(requests)
    if len(requests) != n:
        raise ValueError(f"sampling: {len(requests)} entries for {n} prompts")
    if not any(d is not None and "return_log_probs" in d for d in requests):
        return None
    flags = np.zeros(n, dtype=np.int32)
    for i, d in enumerate(requests):
        v = (d or {}).get("return_log_probs", False)
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"sampling[{i}]: return_log_probs must be a bool, not {v!r}")
        flags[i] = int(bool(v))
    return flags


def logprob_requested(d: Optional[Mapping]) -> bool:
    """The request dict asks for per-token log-probabilities."""
    return d is not None and bool(d.get("return_log_probs", False))


def penalty_neutral(d: Optional[Mapping]) -> bool:
    """True when a request dict asks for no penalty (every penalty key it carries has its neutral value)."""
    return d is None or all(float(d.get(k, v)) == v for k, v in PENALTY_NEUTRAL.items())


def penalty_records(requests: Optional[Sequence[Optional[Mapping]]], n: int):
    """One ``smi_penalty_params`` per prompt from the penalty keys of the request dicts, or None when no request is penalised
    (neutral values and missing keys alike: the admission is then exactly the unpenalised one).  ``penalize_prompt``
    defaults to True (transformers' default; False: only the generated tokens count for ``repetition_penalty``).  Ranges are
    checked by the library."""
    if requests is None:
        return None
    requests = list(requests)
    if len(requests) != n:
        raise ValueError(f"sampling: {len(requests)} entries for {n} prompts")
    if all(penalty_neutral(d) for d in requests):
        return None
    recs = (_lib.PenaltyParams * n)()
    for i, d in enumerate(requests):
        r = recs[i]
        r.repetition_penalty, r.penalize_prompt = 1.0, 1
        if penalty_neutral(d):
            continue
        r.repetition_penalty = float(d.get("repetition_penalty", 1.0))
        r.presence_penalty = float(d.get("presence_penalty", 0.0))
        r.frequency_penalty = float(d.get("frequency_penalty", 0.0))
        r.min_new_tokens = int(d.get("min_new_tokens", 0))
        r.penalize_prompt = int(bool(d.get("penalize_prompt", True)))
    return recs


def sampling_records(sampling: Optional[Sequence[Optional[Mapping]]], n: int, defaults: Mapping):
    """One ``smi_sample_params`` per prompt, or None when every prompt inherits the handle's settings (``smi_llm_admit``).
    ``sampling[i]`` None, or a dict of penalty keys (``PENALTY_KEYS``) alone: inherit.  A dict: ``do_sample`` False -> greedy, else this record's own temperature / top_k / top_p
    (keys it leaves out take ``defaults``, the handle's ``set_sampling`` values, ``do_sample`` included) and, with ``seed``
    given, its own stream keyed by that seed and the sequence's token index alone.  Ranges are checked by the library."""
    if sampling is None:
        return None
    sampling = list(sampling)
    if len(sampling) != n:
        raise ValueError(f"sampling: {len(sampling)} entries for {n} prompts")
    if all(d is None for d in sampling):
        return None
    known = SAMPLING_KEYS + PENALTY_KEYS + LOGPROB_KEYS + (ALLOW_KEY,) + SEQ_KEYS + (NGRAM_KEY,)
    for i, d in enumerate(sampling):
        bad = set(d or ()) - set(known)
        if bad:
            raise ValueError(f"sampling[{i}]: unknown keys {sorted(bad)} (known: {', '.join(known)})")
    # a dict that carries penalty / log-probability keys alone leaves the token selection to the handle (inherit)
    sampling = [None if d is not None and d and not set(d) & set(SAMPLING_KEYS) else d for d in sampling]
    if all(d is None for d in sampling):
        return None
    recs = (_lib.SampleParams * n)()
    for i, d in enumerate(sampling):
        if d is None:
            continue
        r = recs[i]
        if not bool(d.get("do_sample", defaults["do_sample"])):
            r.mode = _lib.SAMPLING_GREEDY
            continue
        r.mode = _lib.SAMPLING_SAMPLE
        r.temperature = float(d.get("temperature", defaults["temperature"]))
        r.top_k = int(d.get("top_k", defaults["top_k"]))
        r.top_p = float(d.get("top_p", defaults["top_p"]))
        if d.get("seed") is not None:
            r.seed, r.has_seed = int(d["seed"]) & (2 ** 64 - 1), 1
    return recs


def eos_ids_from_generation_config(model_dir: Union[str, Path], cfg: Optional[LLMConfig] = None) -> List[int]:
    """The ids HF ``generate()`` stops on when the caller passes no ``eos_token_id`` -- which is how the reference
    calls it (``cli/SparkTTS.py:197-204``): every id of ``generation_config.json``'s ``eos_token_id`` (an int or a
    list), else ``config.json``'s."""
    ids: List[int] = []
    g = Path(model_dir) / "generation_config.json"
    if g.exists():
        e = json.loads(g.read_text()).get("eos_token_id")
        if e is not None:
            ids = [int(x) for x in (e if isinstance(e, (list, tuple)) else [e])]
    if not ids and cfg is not None and cfg.eos_token_id is not None:
        e = cfg.eos_token_id
        ids = [int(x) for x in (e if isinstance(e, (list, tuple)) else [e])]
    return ids


class SparkLLM:
    def __init__(self, cfg: LLMConfig, weights: Mapping[str, np.ndarray],
                 device: Union[str, torch.device] = "cuda:0", max_slots: int = 1,
                 max_positions: int = 4096, kv_dtype: str = "bf16", use_graph: bool = True,
                 arena: Optional[torch.Tensor] = None, eos_token_ids: EosLike = None,
                 kv_page_tokens: int = 0, kv_pages: int = 0, diag: bool = False, weights_exact: bool = False):
        """``eos_token_ids``: the model's default stop ids (``generation_config.json``; see
        ``eos_ids_from_generation_config``).  ``generate()`` falls back to them when the caller passes none, like HF.
        ``kv_page_tokens`` / ``kv_pages``: paged KV cache -- a pool of ``kv_pages`` pages of ``kv_page_tokens`` tokens
        shared by the ``max_slots`` sequences instead of ``max_positions`` reserved tokens per slot (sparkmi.h).
        ``weights_exact``: the verification mode of ``smi_llm_cfg.weights_exact`` -- the arena keeps the matrices in fp32 and every
        GEMM is an exact fp32 chain, so a checkpoint SAVED in fp32 (the published Spark-TTS-0.5B LLM is) gives the fp32 PyTorch
        CPU path's tokens instead of those of its bf16 rounding; opt-in, ~4x slower, 2x the weight bytes.
        ``diag``: put the handle on ``libsparkmi_diag.so`` (timing probes, scratch dumps, SPARKMI_* switches, the one-row engine:
        ``include/sparkmi_debug.h``) instead of the product library -- tools, bench probes and tests only."""
        cfg.validate()
        self.cfg = cfg
        if eos_token_ids is None and cfg.eos_token_id is not None:
            eos_token_ids = cfg.eos_token_id
        self.default_eos = self._eos_list(eos_token_ids)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SparkMIError("SparkLLM runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self._lib = _lib.pick(diag)
        torch.cuda.set_device(self.device)
        _lib.require_gfx950()
        self.max_slots, self.max_positions = max_slots, max_positions
        self._cs = llm_cfg_struct(cfg, max_slots, max_positions, kv_dtype, use_graph, kv_page_tokens, kv_pages, weights_exact)
        if arena is None:
            host = pack_llm_arena(cfg, weights, self._cs)
            arena = torch.from_numpy(host).to(self.device)
        else:
            # a packed arena says how it was packed (section LLM_TAG): its W_down tile order wins over what the environment
            # would choose now; any other disagreement with the config is refused by smi_llm_create
            off, nb = C.c_size_t(), C.c_size_t()
            self._lib.check(self._lib.smi_llm_arena_section(C.byref(self._cs), _lib.LLM_TAG, 0, C.byref(off), C.byref(nb)),
                            "smi_llm_arena_section")
            if arena.numel() >= off.value + nb.value:
                tag = _lib.LLMArenaTag.from_buffer_copy(arena[off.value: off.value + nb.value].cpu().numpy().tobytes())
                if tag.magic == b"SMIARENA":
                    self._cs.wd_plain = tag.wd_plain
        self.arena = arena  # uint8 device tensor; must outlive the handle
        self._sampling = dict(do_sample=False, temperature=0.8, top_k=50, top_p=0.95)   # the handle's (smi_llm_create's)
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_llm_create(C.byref(self._cs), C.c_void_p(arena.data_ptr()),
                                            arena.numel(), C.byref(self._h)), "smi_llm_create")

    # ------------------------------------------------------------------ plumbing
    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_llm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @classmethod
    def from_pretrained(cls, llm_dir: Union[str, Path], device: Union[str, torch.device] = "cuda:0", **kw) -> "SparkLLM":
        """Stands where ``AutoModelForCausalLM.from_pretrained(f"{model_dir}/LLM")`` stands (``cli/SparkTTS.py:49``):
        config.json, safetensors and generation_config.json (stop ids) of a checkpoint directory."""
        from .weights import load_llm_state
        llm_dir = Path(llm_dir)
        cfg = LLMConfig.from_json(llm_dir / "config.json")
        return cls(cfg, load_llm_state(llm_dir), device, eos_token_ids=eos_ids_from_generation_config(llm_dir, cfg), **kw)

    @staticmethod
    def _eos_list(eos: EosLike) -> List[int]:
        if eos is None:
            return []
        ids = [int(eos)] if isinstance(eos, (int, np.integer)) else [int(e) for e in eos]
        if len(ids) > _lib.SMI_MAX_EOS:
            raise ValueError(f"{len(ids)} eos ids; the step kernel checks at most {_lib.SMI_MAX_EOS}")
        return ids

    def _eos_args(self, eos: EosLike):
        ids = self._eos_list(eos)
        arr = (C.c_int64 * max(len(ids), 1))(*ids)
        return arr, len(ids)

    # ------------------------------------------------------------------ generation
    def prefill(self, prompts: Sequence[Sequence[int]], eos_token_id: EosLike = None) -> None:
        """``eos_token_id``: an id, a list of ids (any of them stops the sequence) or None (never stop)."""
        B = len(prompts)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        pmax = int(lens.max())
        ids = np.zeros((B, pmax), dtype=np.int64)
        for b, p in enumerate(prompts):
            ids[b, : len(p)] = np.asarray(p, dtype=np.int64)
        eos_arr, n_eos = self._eos_args(eos_token_id)
        self._lib.check(self._lib.smi_llm_prefill(
            self._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(C.POINTER(C.c_int32)),
            B, pmax, eos_arr, n_eos, self._stream()), "smi_llm_prefill")
        self._B, self._lens = B, lens

    def decode(self, n_steps: int) -> None:
        self._lib.check(self._lib.smi_llm_decode(self._h, int(n_steps), self._stream()), "smi_llm_decode")

    def all_done(self) -> bool:
        d = C.c_int(0)
        self._lib.check(self._lib.smi_llm_all_done(self._h, C.byref(d), self._stream()), "smi_llm_all_done")
        return bool(d.value)

    def tokens(self, cap: int) -> List[List[int]]:
        out = np.zeros((self._B, cap), dtype=np.int64)
        lens = np.zeros(self._B, dtype=np.int32)
        self._lib.check(self._lib.smi_llm_get_tokens(
            self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(C.POINTER(C.c_int32)),
            cap, self._stream()), "smi_llm_get_tokens")
        return [out[b, : lens[b]].tolist() for b in range(self._B)]

    def set_sampling(self, do_sample: bool, temperature: float = 0.8, top_k: int = 50, top_p: float = 0.95,
                     seed: Optional[int] = None) -> None:
        if seed is None:
            seed = int(np.random.SeedSequence().generate_state(1, dtype=np.uint64)[0]) if do_sample else 0
        self._lib.check(self._lib.smi_llm_set_sampling(self._h, int(bool(do_sample)), float(temperature), int(top_k),
                                                  float(top_p), int(seed) & (2 ** 64 - 1)), "smi_llm_set_sampling")
        self._sampling = dict(do_sample=bool(do_sample), temperature=float(temperature), top_k=int(top_k), top_p=float(top_p))

    def generate_ids(self, prompts: Sequence[Sequence[int]], max_new_tokens: int,
                     eos_token_id: EosLike = None, check_every: int = 32, do_sample: bool = False,
                     temperature: float = 0.8, top_k: int = 50, top_p: float = 0.95,
                     seed: Optional[int] = None) -> List[List[int]]:
        """Generation for B ragged prompts; returns only the new ids per sequence (eos included
        when emitted).  Greedy by default; ``do_sample`` selects the reference's temperature /
        top-k / top-p sampler.  With no eos the whole run is enqueued without a host sync."""
        self.set_sampling(do_sample, temperature, top_k, top_p, seed)
        if max_new_tokens < 1:
            raise ValueError("max_new_tokens must be >= 1")
        longest = max(len(p) for p in prompts)
        if longest + max_new_tokens > self.max_positions:
            raise ValueError(f"prompt ({longest}) + max_new_tokens ({max_new_tokens}) exceeds "
                             f"max_positions ({self.max_positions})")
        self.prefill(prompts, eos_token_id)
        remaining = max_new_tokens - 1
        if not self._eos_list(eos_token_id):
            self.decode(remaining)
        else:
            while remaining > 0 and not self.all_done():
                n = min(check_every, remaining)
                self.decode(n)
                remaining -= n
        return self.tokens(max_new_tokens)

    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                 max_new_tokens: int = 3000, do_sample: bool = False, eos_token_id: EosLike = None,
                 pad_token_id: Optional[int] = None, temperature: float = 1.0, top_k: int = 50,
                 top_p: float = 1.0, seed: Optional[int] = None, **unused) -> torch.Tensor:
        """HF-shaped entry.  ``attention_mask`` marks real tokens of right- or left-padded rows.  Like HF's
        ``generate``: with no ``eos_token_id`` the model's own stop ids apply (``generation_config.json``, given at
        construction) -- the reference's call at ``cli/SparkTTS.py:197-204`` relies on exactly that -- and generation
        ends at the context limit when ``max_new_tokens`` would pass it (HF's limit is the model's 32k positions; here it
        is ``max_positions``, so a long clone prompt shortens the budget instead of failing)."""
        ids = input_ids.detach().cpu().numpy().astype(np.int64)
        if ids.ndim == 1:
            ids = ids[None]
        if attention_mask is not None:
            msk = attention_mask.detach().cpu().numpy().astype(bool)
            prompts = [ids[b][msk[b]].tolist() for b in range(ids.shape[0])]
        else:
            prompts = [ids[b].tolist() for b in range(ids.shape[0])]
        eos = self._eos_list(eos_token_id) or self.default_eos
        room = self.max_positions - max(len(p) for p in prompts)
        if room < 1:
            raise ValueError(f"prompt of {max(len(p) for p in prompts)} tokens leaves no room in max_positions={self.max_positions}")
        new = self.generate_ids(prompts, min(int(max_new_tokens), room), eos, do_sample=do_sample, temperature=temperature,
                                top_k=top_k, top_p=top_p, seed=seed)
        pad = pad_token_id if pad_token_id is not None else (eos[0] if eos else 0)
        n = max(len(t) for t in new)
        out = np.full((ids.shape[0], ids.shape[1] + n), pad, dtype=np.int64)
        out[:, : ids.shape[1]] = ids
        for b, t in enumerate(new):
            out[b, ids.shape[1]: ids.shape[1] + len(t)] = t
        return torch.from_numpy(out).to(input_ids.device)

    # ------------------------------------------------------------------ continuous batching
    def session_begin(self, eos_token_id: EosLike = None) -> None:
        """Empty in-flight-batching session: sequences are admitted and retired between decode steps."""
        eos_arr, n_eos = self._eos_args(eos_token_id)
        self._session_eos = self._eos_list(eos_token_id)
        self._lib.check(self._lib.smi_llm_session_begin(self._h, eos_arr, n_eos, self._stream()), "smi_llm_session_begin")

    def admit(self, prompts: Sequence[Sequence[int]], sampling: Optional[Sequence[Optional[Mapping]]] = None,
              n_return: Optional[Sequence[int]] = None) -> List[int]:
        """Prefill new prompts into free KV slots (first token emitted); returns their slot ids.  ``sampling``: one dict or
        None per prompt; None everywhere (the default): every sequence follows ``set_sampling`` and carries no record.  The
        keys of a dict make up to six records for its sequence: its own token selection (``SAMPLING_KEYS``;
        ``sampling_records``), logits penalties (``PENALTY_KEYS``; ``penalty_records``), ``return_log_probs`` (``LOGPROB_KEYS``,
        a bool; ``logprob_flags`` -- the flagged sequences' log-probabilities are read with ``slots_logprobs``),
        ``allowed_token_ids`` (``ALLOW_KEY``: an iterable of ids; ``allow_records`` -- the sequence emits only ids of its set,
        eos ids are not added to it) and ``sequence_bias`` / ``bad_words_ids`` / ``stop_sequences`` (``SEQ_KEYS``;
        ``seq_records``), and ``no_repeat_ngram_size`` (``NGRAM_KEY``; ``ngram_records``).  ``n_return``: one int >= 1 per prompt -- that many takes of the prompt, its prompt prefilled once;
        ``sampling`` stays one dict per prompt and is expanded per take (``expand_takes``), and the result is the flat,
        prompt-major slot list.
        Every admission is one ``smi_llm_admit_ngram`` call.  A kind of record that no request asks for is passed as NULL, and
        so is ``n_return`` None: by the contract of include/sparkmi.h that is exactly the narrower entry point
        (``smi_llm_admit`` when all are NULL), with its route and bits."""
        n = N = len(prompts)
        takes, nret = sampling, None
        if n_return is not None:
            n_return = [num_returns(k, f"n_return[{b}]") for b, k in enumerate(n_return)]
            if len(n_return) != n or n == 0:
                raise ValueError(f"n_return: {len(n_return)} entries for {n} prompts")
            N = sum(n_return)
            if N > self.max_slots:
                raise ValueError(f"{N} takes > max_slots={self.max_slots}")
            takes = expand_takes(sampling, n_return)
            nret = np.asarray(n_return, dtype=np.int32)
        lens = np.array([len(p) for p in prompts], dtype=np.int32)
        pmax = int(lens.max())
        ids = np.zeros((n, pmax), dtype=np.int64)
        for b, p in enumerate(prompts):
            ids[b, : len(p)] = np.asarray(p, dtype=np.int64)
        recs = sampling_records(takes, N, self._sampling)
        pens = penalty_records(takes, N)
        flags = logprob_flags(takes, N)
        allow = allow_records(takes, N, self.cfg.vocab_size)
        seqs = seq_records(takes, N, self.cfg.vocab_size, getattr(self, "_session_eos", ()))
        ngr = ngram_records(takes, N)
        slots = np.zeros(N, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_admit_ngram(self._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), lens.ctypes.data_as(i32), n, pmax,
                                                      None if nret is None else nret.ctypes.data_as(i32), recs, pens,
                                                      None if flags is None else flags.ctypes.data_as(i32), allow, seqs,
                                                      None if ngr is None else ngr.ctypes.data_as(i32),
                                                      slots.ctypes.data_as(i32), self._stream()), "smi_llm_admit")
        return slots.tolist()

    def retire(self, slot: int) -> None:
        self._lib.check(self._lib.smi_llm_retire(self._h, int(slot), self._stream()), "smi_llm_retire")

    def retire_many(self, slots: Sequence[int]) -> None:
        """Several sequences leave at once; no host round trip (the device row list is compacted in place)."""
        arr = np.asarray(list(slots), dtype=np.int32)
        self._lib.check(self._lib.smi_llm_retire_many(self._h, arr.ctypes.data_as(C.POINTER(C.c_int32)), len(arr), self._stream()),
                   "smi_llm_retire_many")

    def slot_blob_bytes(self, slot: int) -> int:
        """Bytes of the snapshot ``save_slots`` would write for the sequence now in ``slot`` (host arithmetic only)."""
        nb = C.c_size_t(0)
        self._lib.check(self._lib.smi_llm_slot_blob_bytes(self._h, int(slot), C.byref(nb)), "smi_llm_slot_blob_bytes")
        return int(nb.value)

    def save_slots(self, slots: Sequence[int]) -> List[torch.Tensor]:
        """One snapshot per listed busy slot: a ``torch.uint8`` device tensor of ``slot_blob_bytes`` bytes holding the sequence's
        complete state (``smi_llm_slots_save``; the layout is in include/sparkmi.h).  The slots stay as they were.  The caller
        owns the tensors; ``restore_slots`` puts one back, any time later in the same session."""
        arr = np.asarray(list(slots), dtype=np.int32)
        n = len(arr)
        # (sizes first: an unknown slot raises here, before anything is allocated)
        blobs = [torch.empty(self.slot_blob_bytes(int(s)), dtype=torch.uint8, device=self.device) for s in arr]
        ptrs = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in blobs])
        caps = (C.c_size_t * max(n, 1))(*[b.numel() for b in blobs])
        used = (C.c_size_t * max(n, 1))()
        self._lib.check(self._lib.smi_llm_slots_save(self._h, arr.ctypes.data_as(C.POINTER(C.c_int32)), n, ptrs, caps, used,
                                                     self._stream()), "smi_llm_slots_save")
        assert [int(u) for u in used[:n]] == [b.numel() for b in blobs]
        return blobs

    def restore_slots(self, blobs: Sequence[torch.Tensor]) -> List[int]:
        """Each snapshot goes into a free KV slot (the lowest free ones, in order; not necessarily where it came from) and its
        sequence continues exactly where it was saved; returns the slots (``smi_llm_slots_restore``)."""
        blobs = list(blobs)
        n = len(blobs)
        for b in blobs:
            if not (isinstance(b, torch.Tensor) and b.dtype == torch.uint8 and b.is_cuda and b.is_contiguous() and b.dim() == 1):
                raise ValueError("restore_slots: a blob is a contiguous 1-D torch.uint8 device tensor")
        ptrs = (C.c_void_p * max(n, 1))(*[b.data_ptr() for b in blobs])
        nbytes = (C.c_size_t * max(n, 1))(*[b.numel() for b in blobs])
        slots = np.zeros(max(n, 1), dtype=np.int32)
        self._lib.check(self._lib.smi_llm_slots_restore(self._h, ptrs, nbytes, n, slots.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        self._stream()), "smi_llm_slots_restore")
        return slots[:n].tolist()

    def park(self, slots: Sequence[int]) -> List[torch.Tensor]:
        """``save_slots`` followed by ``retire_many``: the sequences leave their slots (and pages) and live on in the returned
        snapshots until ``restore_slots``."""
        blobs = self.save_slots(slots)
        self.retire_many(slots)
        return blobs

    def slots_tokens(self, slots: Sequence[int], cap: int):
        """[(tokens, finished)] of several slots (live or retired and not yet reused) in one device round trip."""
        arr = np.asarray(list(slots), dtype=np.int32)
        out = np.zeros((len(arr), max(cap, 1)), dtype=np.int64)
        n = np.zeros(len(arr), dtype=np.int32)
        fin = np.zeros(len(arr), dtype=np.int32)
        self._lib.check(self._lib.smi_llm_slots_tokens(self._h, arr.ctypes.data_as(C.POINTER(C.c_int32)), len(arr),
                                                  out.ctypes.data_as(C.POINTER(C.c_int64)), max(cap, 1), n.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  fin.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()), "smi_llm_slots_tokens")
        return [(out[i, : n[i]].tolist(), bool(fin[i])) for i in range(len(arr))]

    def poll(self, slots: Sequence[int], from_: Sequence[int], cap: int):
        """[(new ids, count, finished)] of several slots (live, or retired and not yet reused): the ids slot i has emitted from
        its own offset ``from_[i]`` on, at most ``cap`` of them, the tokens it has emitted so far and its eos flag -- one small
        device round trip (``smi_llm_poll``: a gather kernel and one copy of ``len(slots) * (8 + 8 * cap)`` bytes), where
        ``slots_tokens`` copies the whole history.  Equal to ``slots_tokens`` of the same slots, sliced."""
        arr = np.asarray(list(slots), dtype=np.int32)
        frm = np.asarray(list(from_), dtype=np.int32)
        if arr.shape != frm.shape:
            raise ValueError(f"poll: {len(arr)} slots, {len(frm)} offsets")
        cap = int(cap)
        out = np.zeros((len(arr), max(cap, 1)), dtype=np.int64)
        n = np.zeros(len(arr), dtype=np.int32)
        cnt = np.zeros(len(arr), dtype=np.int32)
        fin = np.zeros(len(arr), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_poll(self._h, arr.ctypes.data_as(i32), frm.ctypes.data_as(i32), len(arr),
                                               out.ctypes.data_as(C.POINTER(C.c_int64)), cap, n.ctypes.data_as(i32),
                                               cnt.ctypes.data_as(i32), fin.ctypes.data_as(i32), self._stream()), "smi_llm_poll")
        return [(out[i, : n[i]].tolist(), int(cnt[i]), bool(fin[i])) for i in range(len(arr))]

    def slots_logprobs(self, slots: Sequence[int], cap: int) -> List[np.ndarray]:
        """Per-token log-probabilities (float32, one per token of ``slots_tokens``) of several slots whose sequences were
        admitted with ``return_log_probs``, live or retired and not yet reused, in one device round trip."""
        arr = np.asarray(list(slots), dtype=np.int32)
        out = np.zeros((len(arr), max(cap, 1)), dtype=np.float32)
        n = np.zeros(len(arr), dtype=np.int32)
        self._lib.check(self._lib.smi_llm_slots_logprobs(self._h, arr.ctypes.data_as(C.POINTER(C.c_int32)), len(arr),
                                                    out.ctypes.data_as(C.POINTER(C.c_float)), max(cap, 1),
                                                    n.ctypes.data_as(C.POINTER(C.c_int32)), self._stream()),
                        "smi_llm_slots_logprobs")
        return [out[i, : n[i]].copy() for i in range(len(arr))]

    def slot_tokens(self, slot: int, cap: int):
        """(tokens emitted so far by the sequence in ``slot``, finished flag)."""
        out = np.zeros(max(cap, 1), dtype=np.int64)
        n, fin = C.c_int32(0), C.c_int32(0)
        self._lib.check(self._lib.smi_llm_slot_tokens(self._h, int(slot), out.ctypes.data_as(C.POINTER(C.c_int64)), cap, C.byref(n),
                                                 C.byref(fin), self._stream()), "smi_llm_slot_tokens")
        return out[: n.value].tolist(), bool(fin.value)

    def kv_pages(self):
        """(pages in the pool, pages free) of a paged KV cache; (0, 0) when the cache is not paged."""
        tot, free = C.c_int32(0), C.c_int32(0)
        self._lib.check(self._lib.smi_llm_kv_pages(self._h, C.byref(tot), C.byref(free)), "smi_llm_kv_pages")
        return tot.value, free.value

    def status(self):
        """(tokens emitted, finished flag) per KV slot, as two int32 arrays of SMI_MAX_ROWS -- one device round trip."""
        cnt = np.zeros(_lib.SMI_MAX_ROWS, dtype=np.int32)
        fin = np.zeros(_lib.SMI_MAX_ROWS, dtype=np.int32)
        self._lib.check(self._lib.smi_llm_status(self._h, cnt.ctypes.data_as(C.POINTER(C.c_int32)), fin.ctypes.data_as(C.POINTER(C.c_int32)),
                                            self._stream()), "smi_llm_status")
        return cnt, fin

    def serve(self, requests, max_live: Optional[int] = None, decode_stride: int = 8, return_log_probs: bool = False):
        """In-flight batching driver: ``requests`` yields (key, prompt ids, max_new_tokens, eos id or None -- one eos for
        the session: the first request's[, sampling dict or None]); yields (key, new ids) as each sequence finishes.  New
        requests are admitted whenever a slot is free, so short utterances never wait for long ones.  The optional fifth
        element is that request's own token selection and penalties (``admit``); without it the request follows
        ``set_sampling``, unpenalised.  ``return_log_probs=True`` flags every request, a ``return_log_probs`` key one
        request: a flagged request yields (key, (new ids, float32 log-probabilities, one per id)).  A ``num_return_sequences``
        key (``FORK_KEY``, an int >= 1, at most ``max_live``) asks for that many takes of the prompt, prefilled once
        (``admit(n_return=...)``): the request is admitted whole once that many slots are free and yields (key, [one result
        per take]) when all of its takes have finished."""
        it = iter(requests)
        if return_log_probs:
            it = (tuple(r[:4]) + (dict(r[4] if len(r) > 4 and r[4] is not None else {}, return_log_probs=True),) for r in it)
        max_live = min(max_live or self.max_slots, self.max_slots)

        def split(r):   # (request without the takes key, takes or None)
            d = r[4] if len(r) > 4 else None
            if d is None or FORK_KEY not in d:
                return r, None
            k = num_returns(d[FORK_KEY])
            if k > max_live:
                raise ValueError(f"{FORK_KEY}={k} > max_live={max_live}")
            d = {key: v for key, v in d.items() if key != FORK_KEY}
            return tuple(r[:4]) + (d or None,), k

        live = {}                      # slot -> (key, max_new, log-probabilities wanted, (group, take) or None)
        groups = {}                    # group -> [key, take results]
        group_ids = itertools.count()
        pending = next(it, None)
        pending = split(pending) if pending is not None else None
        started = False
        while pending is not None or live:
            batch = []
            while pending is not None and len(live) + sum(b[1] or 1 for b in batch) + (pending[1] or 1) <= max_live:
                batch.append(pending)
                pending = next(it, None)
                pending = split(pending) if pending is not None else None
            if batch:                      # all free slots are filled by ONE admission (one prefill launch sequence)
                if not started:
                    self.session_begin(batch[0][0][3])
                    started = True
                reqs = [b[0] for b in batch]
                samp = [r[4] if len(r) > 4 else None for r in reqs]
                if any(b[1] is not None for b in batch):
                    nret = [b[1] or 1 for b in batch]
                    slots = self.admit([list(r[1]) for r in reqs], samp, n_return=nret)
                    takes = expand_takes(samp, nret)
                    j = 0
                    for (r, k) in batch:
                        g = None
                        if k is not None:
                            g = next(group_ids)
                            groups[g] = [r[0], [None] * k]
                        for t in range(k or 1):
                            live[slots[j]] = (r[0], int(r[2]), logprob_requested(takes[j] if takes is not None else None),
                                              None if g is None else (g, t))
                            j += 1
                else:
                    slots = self.admit([list(r[1]) for r in reqs], samp)
                    for slot, r, d in zip(slots, reqs, samp):
                        live[slot] = (r[0], int(r[2]), logprob_requested(d), None)
            self.decode(decode_stride)
            cnt, fin = self.status()
            leave = [slot for slot in live if fin[slot] or cnt[slot] >= live[slot][1]]
            if leave:                      # their tokens in one round trip, their rows dropped on the device
                cap = max(live[slot][1] for slot in leave)
                got = self.slots_tokens(leave, cap)
                flagged = [slot for slot in leave if live[slot][2]]
                lps = dict(zip(flagged, self.slots_logprobs(flagged, cap))) if flagged else {}
                self.retire_many(leave)
                for slot, (toks, _) in zip(leave, got):
                    key, max_new, want_lp, take = live.pop(slot)
                    res = (toks[:max_new], lps[slot][:max_new]) if want_lp else toks[:max_new]
                    if take is None:
                        yield key, res
                        continue
                    g, t = take
                    groups[g][1][t] = res
                    if all(x is not None for x in groups[g][1]):
                        key, results = groups.pop(g)
                        yield key, results

    def generate_ragged(self, prompts: Sequence[Sequence[int]], max_new_tokens: Sequence[int], eos_token_id: EosLike = None,
                        check_every: int = 16, on_prefilled=None,
                        sampling: Optional[Sequence[Optional[Mapping]]] = None, return_log_probs: bool = False,
                        n_return: Optional[Sequence[int]] = None) -> List:
        """One batch of prompts with PER-ROW token budgets, rows retired as they finish (their budget, or eos): the decode
        step then runs on the rows still alive instead of padding finished ones to the longest (HF ``generate`` pads; the
        reference's TensorRT-LLM deployment batches in flight, run.sh:50-65).  Rows are independent in every kernel, so
        row i's tokens are exactly those of ``generate_ids`` truncated to its budget.  The captured step of every row
        count is cached in the library, so retiring costs a row-table upload, not a graph capture.  Greedy or the
        sampler set by ``set_sampling``, or per prompt by ``sampling`` (as ``admit``: sampling and penalty keys); ``on_prefilled()`` is called after the
        prompts' prefill was enqueued.  ``return_log_probs=True`` flags every row, a ``return_log_probs`` key in ``sampling``
        one row: a flagged row's result is (tokens, float32 log-probabilities, one per token; include/sparkmi.h,
        smi_llm_admit_logprobs).  ``n_return``: one int >= 1 per prompt -- that many takes of it (``admit``), each with the
        prompt's budget; ``result[b]`` is then a list of ``n_return[b]`` results, each in the shape above."""
        n = len(prompts)
        if return_log_probs:
            sampling = [dict(d or {}, return_log_probs=True) for d in (sampling if sampling is not None else [None] * n)]
        want = [int(w) for w in max_new_tokens]
        if n_return is not None:
            n_return = [num_returns(k, f"n_return[{b}]") for b, k in enumerate(n_return)]
            if len(n_return) != n:
                raise ValueError(f"n_return: {len(n_return)} entries for {n} prompts")
        rows = sum(n_return) if n_return is not None else n
        if n != len(want) or rows > self.max_slots or min(want) < 1:
            raise ValueError("generate_ragged: one budget >= 1 per prompt, at most max_slots sequences")
        if max(len(p) + w for p, w in zip(prompts, want)) > self.max_positions:
            raise ValueError("generate_ragged: prompt + budget exceeds max_positions")
        eos = self._eos_list(eos_token_id)
        self.session_begin(eos or None)
        if n_return is not None:
            slots = self.admit([list(p) for p in prompts], sampling, n_return=n_return)
            owner = [b for b, k in enumerate(n_return) for _ in range(k)]
            row_samp = expand_takes(sampling, n_return)
        else:
            slots = self.admit([list(p) for p in prompts], sampling)
            owner, row_samp = list(range(n)), sampling
        row_want = [want[b] for b in owner]
        if on_prefilled is not None:
            on_prefilled()
        live = {slot: i for i, slot in enumerate(slots)}
        done = 1                                   # tokens every live row has emitted (the prefill emits the first)
        stops = eos or any(d is not None and d.get("stop_sequences") for d in (sampling or ()))   # some row can finish early
        while live:
            fin = None
            if stops:
                _, fin = self.status()             # one device round trip
            leave = [slot for slot, i in live.items() if done >= row_want[i] or (fin is not None and fin[slot])]
            if leave:
                self.retire_many(leave)            # enqueued behind the steps so far: no host round trip
                for slot in leave:
                    del live[slot]
            if not live:
                break
            steps = min(row_want[i] for i in live.values()) - done
            if stops:
                steps = min(steps, check_every)
            self.decode(steps)
            done += steps
        # histories are per KV slot and stay until a slot is reused: all rows in one round trip
        got = self.slots_tokens(slots, max(want))
        res = [t[: row_want[i]] for i, (t, _) in enumerate(got)]
        flagged = [i for i in range(len(slots)) if logprob_requested(row_samp[i] if row_samp is not None else None)]
        if flagged:
            for i, lp in zip(flagged, self.slots_logprobs([slots[i] for i in flagged], max(want))):
                res[i] = (res[i], lp[: row_want[i]])
        if n_return is None:
            return res
        out: List[List] = [[] for _ in range(n)]
        for i, b in enumerate(owner):
            out[b].append(res[i])
        return out

    # ------------------------------------------------------------------ test / bench entries
    def forward_logits(self, ids: Sequence[int]) -> torch.Tensor:
        """Teacher-forced logits (S, V) for one sequence fed at positions 0..S-1."""
        a = np.asarray(ids, dtype=np.int64)
        out = torch.empty((a.shape[0], self.cfg.vocab_size), dtype=torch.float32, device=self.device)
        self._lib.check(self._lib.smi_llm_forward_logits(
            self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), a.shape[0], C.c_void_p(out.data_ptr()),
            self._stream()), "smi_llm_forward_logits")
        return out

    # ------------------------------------------------------------------ diagnostics (include/sparkmi_debug.h; diag=True handles)
    def _need_diag(self, what: str) -> None:
        if not self._lib.is_diag:
            raise _lib.SparkMIError(f"SparkLLM.{what} is a diagnostics entry (include/sparkmi_debug.h): construct the engine with "
                                    "diag=True (libsparkmi_diag.so); the product library does not export it")

    def engine_info(self) -> dict:
        """Whether one-row decode steps run as one persistent launch, and why / why not."""
        self._need_diag("engine_info")
        on = C.c_int32(0)
        info = (C.c_int32 * 4)()
        why = C.create_string_buffer(200)
        self._lib.check(self._lib.smi_llm_engine(self._h, C.byref(on), info, why, 200), "smi_llm_engine")
        return {"enabled": bool(on.value), "built": bool(info[3]), "cus": int(info[0]), "images_per_wave": int(info[1]),
                "lds_bytes": int(info[2]), "why": why.value.decode(errors="replace")}

    def set_engine(self, on: bool) -> None:
        """Runtime switch between the engine and the four-launches-per-layer path (same bits; A/B runs and tests)."""
        self._need_diag("set_engine")
        self._lib.check(self._lib.smi_llm_set_engine(self._h, 1 if on else 0), "smi_llm_set_engine")

    def engine_stamps(self) -> np.ndarray:
        """(3, layers, 16) microseconds of the last engine launch (needs SPARKMI_ENGINE_STAMPS=1 in the environment)."""
        self._need_diag("engine_stamps")
        n = 3 * self.cfg.num_hidden_layers * 16
        out = (C.c_double * n)()
        self._lib.check(self._lib.smi_llm_engine_stamps(self._h, out, n), "smi_llm_engine_stamps")
        return np.array(out, dtype=np.float64).reshape(3, self.cfg.num_hidden_layers, 16)

    def debug_hidden(self) -> np.ndarray:
        """The residual row of row 0 as the last step left it (tests)."""
        self._need_diag("debug_hidden")
        out = np.zeros(self.cfg.hidden_size, dtype=np.float32)
        self._lib.check(self._lib.smi_llm_debug_hidden(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size), "smi_llm_debug_hidden")
        return out

    def debug_read(self, what: int, nbytes: int = 1 << 22) -> np.ndarray:
        """Raw bytes of one scratch buffer (include/sparkmi_debug.h: smi_llm_debug_read); ``nbytes``: room for the buffer asked
        for (the prefill workspace's buffers are sized by their row count)."""
        self._need_diag("debug_read")
        buf = np.zeros(int(nbytes), dtype=np.uint8)
        got = C.c_size_t(0)
        self._lib.check(self._lib.smi_llm_debug_read(self._h, int(what), buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(got)),
                   "smi_llm_debug_read")
        return buf[: got.value].copy()

    # ---- op-level entries (include/sparkmi_debug.h: smi_llm_debug_layer / _set_kv / _get_kv)
    def debug_set_kv(self, layer: int, slot: int, k: np.ndarray, v: np.ndarray, pos0: int = 0) -> None:
        """k, v: (n, num_kv_heads, 64) fp32 in transformers' dim order (keys already rotated) -> cache positions pos0.."""
        self._need_diag("debug_set_kv")
        k = np.ascontiguousarray(k, dtype=np.float32)
        v = np.ascontiguousarray(v, dtype=np.float32)
        assert k.shape == v.shape == (k.shape[0], self.cfg.num_key_value_heads, 64)
        fp = C.POINTER(C.c_float)
        self._lib.check(self._lib.smi_llm_debug_set_kv(self._h, layer, slot, pos0, k.shape[0], k.ctypes.data_as(fp), v.ctypes.data_as(fp)),
                        "smi_llm_debug_set_kv")

    def debug_get_kv(self, layer: int, slot: int, pos0: int, n: int):
        self._need_diag("debug_get_kv")
        k = np.zeros((n, self.cfg.num_key_value_heads, 64), dtype=np.float32)
        v = np.zeros_like(k)
        fp = C.POINTER(C.c_float)
        self._lib.check(self._lib.smi_llm_debug_get_kv(self._h, layer, slot, pos0, n, k.ctypes.data_as(fp), v.ctypes.data_as(fp)),
                        "smi_llm_debug_get_kv")
        return k, v

    def debug_page_table(self, slot: int) -> np.ndarray:
        """The pages ``slot`` holds, in position order (the host's page table; empty on a contiguous cache)."""
        self._need_diag("debug_page_table")
        n = C.c_int32(0)
        ip = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_debug_page_table(self._h, slot, None, 0, C.byref(n)), "smi_llm_debug_page_table")
        out = np.zeros(n.value, dtype=np.int32)
        self._lib.check(self._lib.smi_llm_debug_page_table(self._h, slot, out.ctypes.data_as(ip), out.size, C.byref(n)), "smi_llm_debug_page_table")
        return out

    @staticmethod
    def _from_triples(raw: np.ndarray, K: int, M: int) -> np.ndarray:
        """[K / 32][3][4][M][8] bf16 (hi, mid, lo planes of an exact split) -> (M, K) fp32, k = 32 * tile + 8 * k8 + e."""
        from .weights import bf16_bits_to_f32
        a = bf16_bits_to_f32(raw.view(np.uint16)).reshape(K // 32, 3, 4, M, 8)
        x = (a[:, 0] + a[:, 1]) + a[:, 2]                       # exact: the three terms do not overlap
        return np.ascontiguousarray(x.transpose(2, 0, 1, 3)).reshape(M, K)

    def debug_layer(self, layer: int, rows, hidden: np.ndarray, stage: int) -> dict:
        """One layer's kernels up to ``stage`` on caller rows (``rows``: (slot, pos) pairs; ``hidden``: (M, hidden) fp32) through
        the step's own launch builders; returns that stage's outputs in transformers' layouts:
        0 {"q" (M, heads, 64), "k" / "v" (M, kv heads, 64)}, 1 {"attn" (M, heads * 64)}, 2 {"h" (M, hidden)},
        3 {"act" (M, intermediate)}, 4 {"h" (M, hidden)}."""
        self._need_diag("debug_layer")
        c = self.cfg
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
        M = rows.shape[0]
        hidden = np.ascontiguousarray(hidden, dtype=np.float32)
        assert hidden.shape == (M, c.hidden_size)
        self._lib.check(self._lib.smi_llm_debug_layer(self._h, layer, M, rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      hidden.ctypes.data_as(C.POINTER(C.c_float)), stage), "smi_llm_debug_layer")
        # (fuse_o_now: the row sits in slot 0 and its keys fit one attention segment, kAttnSeg = 1024)
        fused_one = stage == 2 and M == 1 and int(rows[0, 0]) == 0 and int(rows[0, 1]) < 1024 and self.debug_fused_o()
        return self._stage_outputs(layer, stage, M, [(int(s), int(p), 1) for s, p in rows], (0, 1, 2, 8 if fused_one else 4))

    def _stage_outputs(self, layer: int, stage: int, M: int, runs, bufs) -> dict:
        """Stage ``stage``'s outputs for M rows in transformers' layouts.  ``runs``: (slot, first position, rows) of the K/V rows
        the call appended, in row order; ``bufs``: smi_llm_debug_read's ids of (q, attention triples, act triples, h)."""
        c = self.cfg
        nh, Q = c.num_attention_heads, c.num_attention_heads * 64
        unpair = (np.arange(64) >> 1) + 32 * (np.arange(64) & 1)          # kernel row i of a head holds transformers' dim unpair[i]
        if stage == 0:
            qk = self.debug_read(bufs[0], M * Q * 4).view(np.float32).reshape(M, nh, 64)
            q = np.empty_like(qk)
            q[:, :, unpair] = qk
            kv = [self.debug_get_kv(layer, s, p, n) for s, p, n in runs]
            return {"q": q, "k": np.concatenate([k for k, _ in kv]), "v": np.concatenate([v for _, v in kv])}
        if stage == 1:
            t = self._from_triples(self.debug_read(bufs[1], M * Q * 6), Q, M).reshape(M, 2, nh, 32)     # k tile = half * heads + head
            return {"attn": np.ascontiguousarray(t.transpose(0, 2, 1, 3)).reshape(M, Q)}
        if stage == 3:
            return {"act": self._from_triples(self.debug_read(bufs[2], M * c.intermediate_size * 6), c.intermediate_size, M)}
        return {"h": self.debug_read(bufs[3], M * c.hidden_size * 4).view(np.float32).reshape(M, c.hidden_size)[:M].copy()}

    PF_GROUPED, PF_PGEMM = 1, 2      # include/sparkmi_debug.h: SMI_PF_*

    def debug_prefill_layer(self, layer: int, seqs, hidden: np.ndarray, stage: int, family: int = 2) -> dict:
        """One layer of the PROMPT pass up to ``stage`` on caller rows (``smi_llm_debug_prefill_layer``): ``seqs`` = (slot, first
        position, rows) per sequence, ``hidden`` (M, hidden) fp32 for the M = sum of rows, ``family`` PF_PGEMM / PF_GROUPED.
        Returns ``debug_layer``'s dicts for stages 0-4; stage 5 (the layer, then layer + 1's QKV) returns stage 0's dict for
        layer + 1."""
        self._need_diag("debug_prefill_layer")
        c = self.cfg
        seqs = np.ascontiguousarray(np.asarray(seqs, dtype=np.int32).reshape(-1, 3))
        M = int(seqs[:, 2].sum())
        hidden = np.ascontiguousarray(hidden, dtype=np.float32)
        assert hidden.shape == (M, c.hidden_size)
        self._lib.check(self._lib.smi_llm_debug_prefill_layer(self._h, layer, stage, seqs.shape[0], seqs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                              hidden.ctypes.data_as(C.POINTER(C.c_float)), family),
                        "smi_llm_debug_prefill_layer")
        runs = [(int(s), int(p), int(n)) for s, p, n in seqs]
        if stage == 5:
            return self._stage_outputs(layer + 1, 0, M, runs, (16, 17, 18, 20))
        return self._stage_outputs(layer, stage, M, runs, (16, 17, 18, 20))

    def debug_fused_o(self) -> bool:
        """One live row in slot 0 takes the fused attention + o_proj kernel (smi_llm.hip: fuse_o_now) unless SPARKMI_NO_FUSE_O=1 was set
        when the engine was built, the head count has no fused instantiation, or the engine is in the exact-weights mode (every
        GEMM on k_gemm_x, the o_proj included: smi_llm_create leaves fuse_o off)."""
        import os
        return os.environ.get("SPARKMI_NO_FUSE_O") is None and self.cfg.num_attention_heads in (4, 14) and not self._cs.weights_exact

    def debug_sample(self, logits_row: Optional[np.ndarray], n_rows: int, seed: int, use_bound: bool = True) -> np.ndarray:
        """The device sampler alone on a caller's logits row (``smi_llm_debug_sample``): ``n_rows`` independent draws with
        the parameters of the last ``set_sampling``; ``logits_row`` None keeps the previous call's row."""
        self._need_diag("debug_sample")
        out = np.zeros(n_rows, dtype=np.int32)
        ptr = None
        if logits_row is not None:
            row = np.ascontiguousarray(logits_row, dtype=np.float32)
            assert row.shape == (self.cfg.vocab_size,)
            ptr = row.ctypes.data_as(C.POINTER(C.c_float))
        self._lib.check(self._lib.smi_llm_debug_sample(self._h, ptr, int(n_rows), C.c_uint64(int(seed)), 1 if use_bound else 0,
                                                       out.ctypes.data_as(C.POINTER(C.c_int32))), "smi_llm_debug_sample")
        return out

    def debug_penalize(self, logits: np.ndarray, hist: np.ndarray, pens: Sequence[Mapping], emitted: Sequence[int]):
        """The penalty kernel alone (``smi_llm_debug_penalize``) on caller rows: ``logits`` [n][vocab] f32, ``hist`` [n][vocab]
        uint16 history entries (bit 15: in the prompt; bits 0..14: generated count), one penalty dict (``PENALTY_KEYS``) and
        the tokens emitted so far per row; eos ids from the last ``session_begin``.  Returns (processed logits [n][vocab],
        arg-max [n] over the per-set maxima the kernel leaves for k_finalize)."""
        self._need_diag("debug_penalize")
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        hs = np.ascontiguousarray(hist, dtype=np.uint16)
        n = lg.shape[0]
        assert lg.shape == hs.shape == (n, self.cfg.vocab_size)
        recs = (_lib.PenaltyParams * n)()
        for i, d in enumerate(pens):
            recs[i].repetition_penalty = float(d.get("repetition_penalty", 1.0))
            recs[i].presence_penalty = float(d.get("presence_penalty", 0.0))
            recs[i].frequency_penalty = float(d.get("frequency_penalty", 0.0))
            recs[i].min_new_tokens = int(d.get("min_new_tokens", 0))
            recs[i].penalize_prompt = int(bool(d.get("penalize_prompt", True)))
        em = np.ascontiguousarray(emitted, dtype=np.int32)
        out = np.empty_like(lg)
        am = np.zeros(n, dtype=np.int32)
        self._lib.check(self._lib.smi_llm_debug_penalize(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), n,
                                                         hs.ctypes.data_as(C.POINTER(C.c_uint16)), recs,
                                                         em.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         out.ctypes.data_as(C.POINTER(C.c_float)),
                                                         am.ctypes.data_as(C.POINTER(C.c_int32))), "smi_llm_debug_penalize")
        return out, am

    @staticmethod
    def _pack_contexts(contexts: Sequence[Sequence[int]], prompt_lens: Sequence[int]):
        """What ``debug_seqbias`` / ``debug_ngram`` hand the library: the contexts zero-padded to (n, cap) int64, their lengths and
        the prompt lengths as int32, cap (at least 1)."""
        cl = np.asarray([len(c) for c in contexts], dtype=np.int32)
        cap = max(int(cl.max()), 1)
        ctx = np.zeros((len(contexts), cap), dtype=np.int64)
        for i, c in enumerate(contexts):
            ctx[i, : len(c)] = np.asarray(c, dtype=np.int64)
        return ctx, cl, np.ascontiguousarray(prompt_lens, dtype=np.int32), cap

    def debug_seqbias(self, logits: np.ndarray, requests: Sequence[Optional[Mapping]], contexts: Sequence[Sequence[int]],
                      prompt_lens: Sequence[int], min_new: Optional[Sequence[int]] = None):
        """The bias stage and ``k_finalize``'s stop match alone (``smi_llm_debug_seqbias``) on caller rows: ``logits`` [n][vocab]
        f32, one request dict (``SEQ_KEYS``) or None and one context (prompt + generated ids, the first ``prompt_lens[i]`` the
        prompt) per row.  Returns (the rows after the stage, the arg-max token per row, the finished flag per row)."""
        self._need_diag("debug_seqbias")
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        n = lg.shape[0]
        if lg.shape != (n, self.cfg.vocab_size) or len(requests) != n or len(contexts) != n or len(prompt_lens) != n:
            raise ValueError("debug_seqbias: logits [n][vocab], n requests, n contexts, n prompt lengths")
        recs = seq_records(list(requests), n, self.cfg.vocab_size)
        if recs is None:
            recs = (_lib.SeqParams * n)()
        ctx, cl, pl, cap = self._pack_contexts(contexts, prompt_lens)
        mn = None if min_new is None else np.ascontiguousarray(min_new, dtype=np.int32)
        out = np.empty_like(lg)
        tok = np.zeros(n, dtype=np.int32)
        fin = np.zeros(n, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_debug_seqbias(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), n, recs,
                                                        ctx.ctypes.data_as(C.POINTER(C.c_int64)), cl.ctypes.data_as(i32),
                                                        pl.ctypes.data_as(i32), cap, None if mn is None else mn.ctypes.data_as(i32),
                                                        out.ctypes.data_as(C.POINTER(C.c_float)), tok.ctypes.data_as(i32),
                                                        fin.ctypes.data_as(i32)), "smi_llm_debug_seqbias")
        return out, tok, fin

    def debug_head(self, hidden: np.ndarray, reads: Optional[Sequence[int]] = None, allow: Optional[Sequence[Optional[Sequence]]] = None,
                   finalize: bool = True, poison: bool = False, screen: bool = False) -> dict:
        """The head of a decode step alone (``smi_llm_debug_head``): the final RMSNorm, the lm_head and -- ``finalize`` -- the
        token pick, on ``hidden`` (M, hidden) fp32 = the residual rows leaving the last layer, rows in slots 0 .. M - 1.
        ``reads[m]`` = 1: row m reads its logits (a neutral sampling record); ``allow[m]``: the row's (lo, hi) ranges or None
        (no constraint); ``poison``: the logits buffer is filled with NaNs first; ``screen``: ask for the screened lm_head (the int8
        screen, the selection, then the listed tiles only -- DESIGN 3.4.3) where a step could take it: "form" says whether it ran,
        and ``debug_lm_screen`` returns the list it made.  Returns {"form", "grid", "block", "launches",
        "nblk", "logits_lm" (M, vocab), "pval" / "pidx" (M, nblk), and with ``finalize`` "logits_fin", "tokens", "h" (M, hidden),
        "g" (M, hidden: the next first-norm operand, re-summed from its triples), "ss" (M, hidden / 4)}."""
        self._need_diag("debug_head")
        c = self.cfg
        hidden = np.ascontiguousarray(hidden, dtype=np.float32)
        M = hidden.shape[0]
        if hidden.shape != (M, c.hidden_size) or (reads is not None and len(reads) != M) or (allow is not None and len(allow) != M):
            raise ValueError("debug_head: hidden [M][hidden], M read flags, M allow entries")
        io = _lib.HeadIO()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        io.hidden = hidden.ctypes.data_as(fp)
        if reads is not None:
            rd = np.ascontiguousarray(reads, dtype=np.int32)
            io.reads = rd.ctypes.data_as(ip)
        if allow is not None:
            recs = (_lib.AllowParams * M)()
            for i, ranges in enumerate(allow):
                for j, (lo, hi) in enumerate(ranges or ()):
                    recs[i].lo[j], recs[i].hi[j] = int(lo), int(hi)
                recs[i].n_ranges = len(ranges or ())
            io.allow = recs
        io.flags = (_lib.SMI_HEAD_FIN if finalize else 0) | (_lib.SMI_HEAD_POISON if poison else 0) | (_lib.SMI_HEAD_SCREEN if screen else 0)
        cap = ((c.vocab_size + 15) // 16 + 3) // 4   # lm_cap: the most partial columns a row has
        lg_lm = np.empty((M, c.vocab_size), np.float32)
        lg_fin = np.empty((M, c.vocab_size), np.float32)
        pval = np.empty(M * cap, np.float32)
        pidx = np.empty(M * cap, np.int32)
        tok = np.full(M, -1, np.int32)
        io.pcap = M * cap
        io.logits_lm, io.logits_fin = lg_lm.ctypes.data_as(fp), lg_fin.ctypes.data_as(fp)
        io.pval, io.pidx, io.tokens = pval.ctypes.data_as(fp), pidx.ctypes.data_as(ip), tok.ctypes.data_as(ip)
        self._lib.check(self._lib.smi_llm_debug_head(self._h, M, C.byref(io)), "smi_llm_debug_head")
        nblk = int(io.nblk)
        out = {"form": io.form.decode(), "grid": (int(io.grid[0]), int(io.grid[1])), "block": int(io.block), "launches": int(io.launches),
               "nblk": nblk, "logits_lm": lg_lm, "pval": pval[: M * nblk].reshape(M, nblk).copy(),
               "pidx": pidx[: M * nblk].reshape(M, nblk).copy()}
        if finalize:
            H = c.hidden_size
            out.update(logits_fin=lg_fin, tokens=tok,
                       h=self.debug_read(4, M * H * 4).view(np.float32).reshape(M, H).copy(),
                       g=self._from_triples(self.debug_read(3, M * H * 6), H, M),
                       ss=self.debug_read(6, M * H).view(np.float32).reshape(M, H // 4).copy())
        return out

    def debug_lm_screen(self, reset: bool = False):
        """The screened lm_head's last candidate list and its selection log (``smi_llm_debug_lm_screen``): (the vocabulary tiles
        the last selection listed, ascending; the list lengths of the last selections -- at most 4096 -- oldest first).
        ``reset`` empties the log afterwards."""
        self._need_diag("debug_lm_screen")
        nt = (self.cfg.vocab_size + 15) // 16
        tiles, counts = np.zeros(nt, np.int32), np.zeros(4096, np.int32)
        n, nc = C.c_int32(0), C.c_int32(0)
        ip = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_debug_lm_screen(self._h, tiles.ctypes.data_as(ip), nt, C.byref(n), counts.ctypes.data_as(ip), 4096,
                                                          C.byref(nc), 1 if reset else 0), "smi_llm_debug_lm_screen")
        return tiles[: n.value].copy(), counts[: nc.value].copy()

    def debug_ngram(self, logits: np.ndarray, sizes: Sequence[int], contexts: Sequence[Sequence[int]], prompt_lens: Sequence[int]):
        """The n-gram ban, ``k_penalize`` and ``k_finalize`` alone (``smi_llm_debug_ngram``) on caller rows: ``logits`` [n][vocab]
        f32, one ``no_repeat_ngram_size`` and one context (prompt + generated ids, the first ``prompt_lens[i]`` -- 0 or more --
        the prompt) per row.  Returns (the rows after the stage, the arg-max token per row)."""
        self._need_diag("debug_ngram")
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        n = lg.shape[0]
        if lg.shape != (n, self.cfg.vocab_size) or len(sizes) != n or len(contexts) != n or len(prompt_lens) != n:
            raise ValueError("debug_ngram: logits [n][vocab], n sizes, n contexts, n prompt lengths")
        ng = np.asarray([ngram_size(v) for v in sizes], dtype=np.int32)
        ctx, cl, pl, cap = self._pack_contexts(contexts, prompt_lens)
        out = np.empty_like(lg)
        tok = np.zeros(n, dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        self._lib.check(self._lib.smi_llm_debug_ngram(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), n, ng.ctypes.data_as(i32),
                                                      ctx.ctypes.data_as(C.POINTER(C.c_int64)), cl.ctypes.data_as(i32),
                                                      pl.ctypes.data_as(i32), cap, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                      tok.ctypes.data_as(i32)), "smi_llm_debug_ngram")
        return out, tok

    def debug_logprob(self, logits: np.ndarray, temperature: Sequence[float], tokens: Sequence[int]) -> np.ndarray:
        """The log-probability kernels alone (``smi_llm_debug_logprob``: k_logprob and k_finalize's combine) on caller rows:
        ``logits`` [n][vocab] f32 (the processed logits), one temperature (> 0; 1: unscaled) and one emitted id per row.
        Returns [n] float32: z[tok] - logsumexp(z), z = logits / T."""
        self._need_diag("debug_logprob")
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        n = lg.shape[0]
        assert lg.shape == (n, self.cfg.vocab_size)
        t = np.ascontiguousarray(temperature, dtype=np.float32)
        tk = np.ascontiguousarray(tokens, dtype=np.int32)
        assert t.shape == tk.shape == (n,)
        out = np.zeros(n, dtype=np.float32)
        self._lib.check(self._lib.smi_llm_debug_logprob(self._h, lg.ctypes.data_as(C.POINTER(C.c_float)), n,
                                                        t.ctypes.data_as(C.POINTER(C.c_float)),
                                                        tk.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        out.ctypes.data_as(C.POINTER(C.c_float))), "smi_llm_debug_logprob")
        return out

    KERNELS = ("qkv", "attn", "o_proj", "gate_up", "down", "lm_head", "finalize", "step", "layers")

    def time_kernel(self, name: str, iters: int = 48, layer: int = 0, in_sequence: bool = False) -> float:
        """Average milliseconds per launch of one decode-step kernel (HIP events on this stream).
        ``in_sequence`` times a layer kernel where it runs -- after its producers, which prefetch
        part of its weights into L2 -- as (iters layers) - (the same layers without it)."""
        self._need_diag("time_kernel")
        ms = C.c_float(0)
        self._lib.check(self._lib.smi_llm_time_kernel(self._h, self.KERNELS.index(name) + (16 if in_sequence else 0), layer, iters,
                                                 C.byref(ms), self._stream()), "smi_llm_time_kernel")
        return float(ms.value)

    # algorithmic bytes -------------------------------------------------------------------
    def weight_bytes(self) -> dict:
        c = self.cfg
        h, q, kv, i = c.hidden_size, c.q_dim, c.kv_dim, c.intermediate_size
        return {"qkv": 2 * (q + 2 * kv) * h, "o_proj": 2 * h * q, "gate_up": 2 * 2 * i * h, "down": 2 * h * i,
                "lm_head": 2 * c.vocab_size * h}

    def step_weight_bytes(self) -> int:
        w = self.weight_bytes()
        per_layer = w["qkv"] + w["o_proj"] + w["gate_up"] + w["down"]
        return self.cfg.num_hidden_layers * per_layer + w["lm_head"]

    def kv_bytes_per_token(self) -> int:
        esz = 4 if self._cs.kv_dtype else 2
        return self.cfg.num_hidden_layers * 2 * self.cfg.kv_dim * esz
