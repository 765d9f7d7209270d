"""Audio preparation on the device (``smi_rs_*``, ``csrc/smi_audio.hip``): a rational resampler with
``scipy.signal.resample_poly``'s arithmetic and the voice prompt's volume normalisation and reference clip, written into the
buffers ``smi_enc_forward_rows`` reads.  The same resampler brings the vocoder's 16 kHz rows to a caller's output rate.

The device path follows ``resample_poly`` (the host path's resampler, ``encoder.load_audio``), not the reference's soxr VHQ, and
it works in fp32 where the host works in float64: its 16 kHz samples differ from the host path's by fp32 rounding, so prompt ids
may differ between the two at near-ties.  Nothing here imports scipy: the taps are computed with numpy alone.

``StreamJoiner`` (``smi_join_*``) is the streaming form of that output end: overlapping chunks in, contiguous pieces out,
cross-faded and resampled with the state kept across chunk edges on the device.

``DeviceAudio.trim_rows`` / ``concat_rows`` (``smi_trim_rows``, ``smi_concat_rows``) are the audio edge of long-form synthesis:
the speech bounds of vocoded rows, and the trimmed rows as one waveform with pauses and faded edges.

``DeviceAudio.loudness_rows`` / ``gain_rows`` (``smi_loud_rows``, ``smi_gain_rows``) level the output: the programme loudness of
rows after ITU-R BS.1770 and the gain that brings each to a target under a peak ceiling, measured and applied on the device.
``k_weighting`` designs the weighting filter's coefficients for a sample rate with numpy alone.

``DeviceAudio.limit_rows`` (``smi_limit_rows``) is the look-ahead limiter behind them: peaks found on the 4x oversampled signal, a
sliding minimum and an FIR window, feed-forward, so the device is held to ``tests/limit_ref.py`` bit for bit.  ``limiter_reach`` and
``limiter_window`` give its look-ahead and release for a sample rate and its smoothing weights.

``DeviceAudio.tempo_rows`` (``smi_tempo_rows``) changes the speaking rate of rows at unchanged pitch: WSOLA whose similarity
search is exact integer arithmetic, so the device is held to ``tests/tempo_ref.py`` bit for bit.  ``tempo_ratio``,
``tempo_frame`` and ``tempo_window`` give its rational, its frame and radius for a sample rate, and its window.
``StreamTempo`` (``smi_tempos_*``) is its streaming form: the frame places and an input history are kept on the device per
stream, and the pieces' concatenation is ``tempo_rows`` of the whole stream bit for bit, whatever the chunking.

``DeviceAudio.pitch_rows`` (``smi_pitch_rows``) moves the pitch of rows at an unchanged -- or, with a tempo, separately chosen --
length: that stretch at (tp rq) / (tq rp), then the resampler's sum at rq / rp inside the same launch and a cut; the device is
held to ``tests/pitch_ref.py`` bit for bit.  ``pitch_ratio`` gives the frequency ratio of a number of semitones.
``StreamPitch`` (``smi_pitchs_*``) is its streaming form, in ``StreamTempo``'s place: the stretch's state and the tail of the
stretched signal the resampler still reaches are kept on the device per stream, with the stream's taps, and the pieces'
concatenation is ``pitch_rows`` of the whole stream bit for bit, whatever the chunking.

``StreamLoudness`` (``smi_louds_*``) levels joined streams while they arrive.  It is not ``loudness_rows`` chunk by chunk: the gain
follows the running integrated loudness, knot by knot on the stream's absolute hops, at a bounded rate and under the ceiling.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .encoder import grow_reservation

MAX_ROWS = 64            # rows of one smi_rs_* call (their descriptors travel as kernel arguments)
KAISER_BETA = 5.0        # resample_poly's default window


def ratio(sr_in: int, sr_out: int) -> Tuple[int, int]:
    """(up, down) in lowest terms that takes ``sr_in`` to ``sr_out``"""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates must be positive, not {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n: int, up: int, down: int) -> int:
    """ceil(n * up / down): the length ``resample_poly`` returns (``smi_rs_out_len``)"""
    return -((-int(n) * int(up)) // int(down))


def resample_taps(up: int, down: int) -> np.ndarray:
    """float64 [2H + 1], H = 10 max(up, down): ``firwin(2H + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up`` -- the
    low-pass ``resample_poly(x, up, down)`` designs for itself -- with numpy alone: the windowed sinc
    cutoff sinc(cutoff m) kaiser(2H + 1, 5), normalised to unit gain at DC, times ``up``."""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or math.gcd(up, down) != 1:
        raise ValueError(f"up/down = {up}/{down} must be positive and in lowest terms")
    m_rate = max(up, down)
    half = 10 * m_rate
    cutoff = 1.0 / m_rate
    m = np.arange(2 * half + 1, dtype=np.float64) - half
    h = cutoff * np.sinc(cutoff * m) * np.kaiser(2 * half + 1, KAISER_BETA)
    h /= np.sum(h)
    return h * up


# The analog prototypes of BS.1770's two weighting stages, as they are commonly restated from the standard's 48 kHz table: a
# high shelf (1681.97 Hz, +3.9998 dB, Q 0.70718) and a high pass (38.135 Hz, Q 0.50033), to the digits that reproduce the table.
K_SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)
K_SHELF_VB = 0.4996667741545416      # the band gain is the shelf gain to this power
K_HIGHPASS = (38.13547087602444, 0.5003270373238773)
PEAK_CEILING = 10 ** (-1 / 20)      # -1 dBFS, a sample peak


def k_weighting(sr: int) -> np.ndarray:
    """float64 [10]: ``b0 b1 b2 a1 a2`` of the high shelf, then of the high pass, of BS.1770's K-weighting at ``sr`` Hz -- the
    bilinear transform of the analog prototypes with pre-warping (K = tan(pi f0 / sr)).  At 48 kHz this is the standard's own
    table; ``smi_loud_rows`` takes the coefficients as data."""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"sample rate must be positive, not {sr}")
    f0, gain_db, q = K_SHELF
    if 2 * f0 >= sr:
        raise ValueError(f"sample rate {sr} is below twice the shelf's corner ({f0:.0f} Hz)")
    k = math.tan(math.pi * f0 / sr)
    vh = 10.0 ** (gain_db / 20.0)
    vb = vh ** K_SHELF_VB
    a0 = 1.0 + k / q + k * k
    shelf = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0,
             2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    f0, q = K_HIGHPASS
    k = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + k / q + k * k
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0], dtype=np.float64)


def loudness_block(sr: int) -> int:
    """the sample count of a 400 ms block at ``sr`` Hz, as four whole hops: ``4 * round(0.1 * sr)``"""
    return 4 * int(round(0.1 * int(sr)))


def check_loudness(loudness, peak_ceiling, max_gain_db) -> None:
    """the three loudness arguments of the ``SparkTTS`` calls, checked before anything reaches the device"""
    def number(name, v):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, not {v!r}")
    if loudness is not None:
        number("loudness", loudness)
    number("peak_ceiling", peak_ceiling)
    number("max_gain_db", max_gain_db)
    if not peak_ceiling > 0:
        raise ValueError(f"peak_ceiling must be > 0, not {peak_ceiling!r}")
    if max_gain_db < 0:
        raise ValueError(f"max_gain_db must be >= 0, not {max_gain_db!r}")


LIMITER_MODES = ("true", "sample")   # peak detection: on the 4x oversampled signal, or on the samples alone
LIMITER_PHASES = 4
LIMITER_MAX_LOOKAHEAD, LIMITER_MAX_RELEASE = 256, 2048   # samples (include/sparkmi.h, smi_limit_rows)


def limiter_window(A: int, R: int) -> np.ndarray:
    """float64 [A + R + 1], non-negative, unit sum: the smoothing weights ``smi_limit_rows`` takes as data -- a Hann shape over
    A + R + 2 intervals with the end zeros dropped, ``0.5 - 0.5 cos(2 pi (j + 1) / (A + R + 2))``, normalised"""
    A, R = int(A), int(R)
    if not 0 <= A <= LIMITER_MAX_LOOKAHEAD or not 0 <= R <= LIMITER_MAX_RELEASE:
        raise ValueError(f"lookahead must lie in 0..{LIMITER_MAX_LOOKAHEAD} and release in 0..{LIMITER_MAX_RELEASE} samples, not {A}, {R}")
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(1, A + R + 2, dtype=np.float64) / (A + R + 2))
    return w / np.sum(w)


def limiter_reach(sr: int, lookahead_ms: float = 2.5, release_ms: float = 25.0) -> Tuple[int, int]:
    """(A, R) in samples at ``sr`` Hz, rounded: 40 and 400 at 16 kHz"""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"sample rate must be positive, not {sr}")
    for name, v in (("lookahead_ms", lookahead_ms), ("release_ms", release_ms)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, not {v!r}")
    A, R = int(round(lookahead_ms * sr / 1000.0)), int(round(release_ms * sr / 1000.0))
    if A > LIMITER_MAX_LOOKAHEAD or R > LIMITER_MAX_RELEASE:
        raise ValueError(f"at {sr} Hz lookahead_ms={lookahead_ms!r} and release_ms={release_ms!r} are {A} and {R} samples; the limiter "
                         f"takes at most {LIMITER_MAX_LOOKAHEAD} and {LIMITER_MAX_RELEASE}")
    return A, R


def check_limiter(limiter, peak_ceiling=PEAK_CEILING, lookahead_ms: float = 2.5, release_ms: float = 25.0, sr: int = 16000):
    """the limiter arguments of the ``SparkTTS`` calls, checked before anything reaches the device; returns (A, R) in samples"""
    if limiter is not None and (not isinstance(limiter, str) or limiter not in LIMITER_MODES):
        raise ValueError(f"limiter must be None, \"true\" or \"sample\", not {limiter!r}")
    if isinstance(peak_ceiling, bool) or not isinstance(peak_ceiling, (int, float, np.integer, np.floating)) or not math.isfinite(peak_ceiling) \
            or not peak_ceiling > 0:
        raise ValueError(f"peak_ceiling must be a finite number > 0, not {peak_ceiling!r}")
    return limiter_reach(sr, lookahead_ms, release_ms)


TEMPO_MIN, TEMPO_MAX = 0.5, 2.0


def tempo_ratio(tempo: float) -> Tuple[int, int]:
    """(p, q) in lowest terms for a tempo in [0.5, 2.0] (> 1: faster), to a hundredth: ``round(tempo * 100) / 100``"""
    if isinstance(tempo, bool) or not isinstance(tempo, (int, float, np.integer, np.floating)) or not math.isfinite(tempo):
        raise ValueError(f"tempo must be a finite number, not {tempo!r}")
    if not TEMPO_MIN <= tempo <= TEMPO_MAX:
        raise ValueError(f"tempo must lie in [{TEMPO_MIN}, {TEMPO_MAX}], not {tempo!r}")
    p = int(round(float(tempo) * 100))
    g = math.gcd(p, 100)
    return p // g, 100 // g


PITCH_MIN, PITCH_MAX = -12.0, 12.0
PITCH_TAP_CACHE = 32     # ratios whose fp32 taps ``DeviceAudio.pitch_rows`` keeps on the device at a time
PITCH_TAP_SLOT = 4096    # floats a cached ratio may take: the longest filter of a hundredth ratio (199/100) has 3981 taps


def pitch_ratio(semitones: float) -> Tuple[int, int]:
    """(p, q) in lowest terms, the frequency ratio of a shift of ``semitones`` in [-12.0, 12.0] (> 0: higher) to a hundredth:
    ``round(2 ** (semitones / 12) * 100) / 100``.  +2 -> 28/25, -2 -> 89/100, +7 -> 3/2, +12 -> 2/1.  The resolution is a
    hundredth of the ratio: about 9 cents near 1.0 and about 17 cents at 0.5, so shifts of a few cents round to 1/1."""
    if (isinstance(semitones, bool) or not isinstance(semitones, (int, float, np.integer, np.floating))
            or not math.isfinite(semitones)):
        raise ValueError(f"pitch_shift must be a finite number, not {semitones!r}")
    if not PITCH_MIN <= semitones <= PITCH_MAX:
        raise ValueError(f"pitch_shift must lie in [{PITCH_MIN}, {PITCH_MAX}] semitones, not {semitones!r}")
    p = int(round(2.0 ** (float(semitones) / 12.0) * 100))
    g = math.gcd(p, 100)
    return p // g, 100 // g


def tempo_window(N: int) -> np.ndarray:
    """float64 [N]: the periodic Hann window ``0.5 - 0.5 cos(2 pi i / N)`` that ``smi_tempo_rows`` takes as data; its two
    halves sum to one, so frames half a window apart overlap-add to unit gain"""
    N = int(N)
    if N < 2 or N % 2:
        raise ValueError(f"the frame must be even and positive, not {N}")
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def tempo_frame(sr: int) -> Tuple[int, int]:
    """(N, D) at ``sr`` Hz: a frame of 32 ms as two halves, ``2 * round(0.016 * sr)``, and a search radius of 15 ms"""
    sr = int(sr)
    if sr < 1:
        raise ValueError(f"sample rate must be positive, not {sr}")
    return 2 * int(round(0.016 * sr)), int(round(0.015 * sr))


def tempo_len(L: int, p: int, q: int) -> int:
    """ceil(L * q / p): the samples a span of ``L`` has at tempo p / q (``smi_tempo_layout``)"""
    return -((-int(L) * int(q)) // int(p))


class DeviceAudio:
    """Owns one ``smi_rs`` handle: registers a ratio's taps on first use and keeps (rows, input samples, output samples) as a
    reservation that only grows (``encoder.grow_reservation``).  A grown reservation is a new handle, so its ratios are
    registered again as they come.  ``lib``: the loaded library (tests pass a stand-in to watch the bookkeeping)."""

    def __init__(self, device="cuda:0", diag: bool = False, lib=None):
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("DeviceAudio runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self._h = C.c_void_p()
        self.reserved: Optional[Tuple[int, int, int]] = None
        self.registered: set = set()

    # ---- handle, reservation, filters
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_rs_destroy(self._h)
            self._h = C.c_void_p()
            self.registered = set()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, rows: int, n_in: int, n_out: int) -> None:
        if rows > MAX_ROWS:
            raise ValueError(f"{rows} rows in one call, the device audio path takes at most {MAX_ROWS}")
        new = grow_reservation(self.reserved, (int(rows), int(n_in), int(n_out)))
        if new is None:
            return
        self.close()
        h = C.c_void_p()
        self._lib.check(self._lib.smi_rs_create(*new, C.byref(h)), "smi_rs_create")
        self._h, self.reserved = h, new

    def register(self, up: int, down: int) -> None:
        key = (int(up), int(down))
        if key == (1, 1) or key in self.registered:
            return
        taps = np.ascontiguousarray(resample_taps(*key), dtype=np.float64)
        self._lib.check(self._lib.smi_rs_register(self._h, key[0], key[1], taps.ctypes.data_as(C.POINTER(C.c_double)), taps.size),
                        "smi_rs_register")
        self.registered.add(key)

    def _prepare(self, n_in: Sequence[int], ups: Sequence[int], downs: Sequence[int]) -> List[int]:
        if not (len(n_in) == len(ups) == len(downs)) or not len(n_in):
            raise ValueError("one (up, down) per row, at least one row")
        n_out = [out_len(n, u, d) for n, u, d in zip(n_in, ups, downs)]
        self.reserve(len(n_in), max(n_in), max(n_out))
        for u, d in zip(ups, downs):
            self.register(u, d)
        return n_out

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- device calls
    def resample_rows(self, x, n_in: Sequence[int], ups: Sequence[int], downs: Sequence[int], out_stride: Optional[int] = None):
        """``x``: [B][in_stride] float32 on the device, row b valid for ``n_in[b]``.  Returns (y [B][out_stride] float32 on the
        device -- row b holds its ``n_out[b]`` samples, then zeros --, n_out)."""
        import torch
        B = len(n_in)
        if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
            raise ValueError("resample_rows takes a contiguous [B][in_stride] float32 tensor on the device")
        n_out = self._prepare(n_in, ups, downs)
        stride = max(n_out) if out_stride is None else int(out_stride)
        y = torch.empty((B, stride), dtype=torch.float32, device=self.device)
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        self._lib.check(self._lib.smi_rs_resample_rows(self._h, C.c_void_p(x.data_ptr()), x.shape[1], i32(n_in), i32(ups), i32(downs), B,
                                                       C.c_void_p(y.data_ptr()), stride, self._stream()), "smi_rs_resample_rows")
        return y, n_out

    def prompt_rows(self, raw, n_in: Sequence[int], ups: Sequence[int], downs: Sequence[int], ref_len: Sequence[int],
                    normalize: bool = True, wav_stride: Optional[int] = None, ref_stride: Optional[int] = None):
        """``raw``: [B][in_stride] float32 mono rows on the device at their own rates.  Returns (wav [B][wav_stride], ref
        [B][ref_stride], gain [B] float64, n_out): what ``load_audio(..., volume_normalize)`` + ``get_ref_clip`` give row by
        row, zero-padded like ``pack_rows``, all on the device."""
        import torch
        B = len(n_in)
        if raw.dim() != 2 or raw.shape[0] != B or raw.dtype != torch.float32 or not raw.is_contiguous() or not raw.is_cuda:
            raise ValueError("prompt_rows takes a contiguous [B][in_stride] float32 tensor on the device")
        if len(ref_len) != B:
            raise ValueError("one reference length per row")
        n_out = self._prepare(n_in, ups, downs)
        ws = max(n_out) if wav_stride is None else int(wav_stride)
        rs = max(int(r) for r in ref_len) if ref_stride is None else int(ref_stride)
        wav = torch.empty((B, ws), dtype=torch.float32, device=self.device)
        ref = torch.empty((B, rs), dtype=torch.float32, device=self.device)
        gain = torch.empty((B,), dtype=torch.float64, device=self.device)
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        got = (C.c_int32 * B)()
        self._lib.check(self._lib.smi_rs_prompt_rows(self._h, C.c_void_p(raw.data_ptr()), raw.shape[1], i32(n_in), i32(ups), i32(downs), B,
                                                     int(bool(normalize)), C.c_void_p(wav.data_ptr()), ws, i32(ref_len),
                                                     C.c_void_p(ref.data_ptr()), rs, C.c_void_p(gain.data_ptr()), got, self._stream()),
                        "smi_rs_prompt_rows")
        assert list(got) == n_out, (list(got), n_out)
        return wav, ref, gain, n_out

    def _rows(self, x, n: Sequence[int], who: str) -> int:
        import torch
        B = len(n)
        if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
            raise ValueError(f"{who} takes a contiguous [B][stride] float32 tensor on the device, one length per row")
        return B

    def trim_rows(self, x, n: Sequence[int], window: int, step: int, threshold: float, margin: int) -> List[Tuple[int, int]]:
        """The speech bounds of rows (include/sparkmi.h, smi_trim_rows; ``detect_speech_boundaries``' arithmetic).  ``x``:
        [B][stride] float32 on the device, row b valid for ``n[b]``.  Returns [(start, end)] per row: (0, n) for a row shorter
        than ``window``, (0, 0) for a row without a speech window.  Two launches and one copy of 8 B bytes to the host, which
        waits for it: the only synchronisation of the long-form path."""
        import torch
        B = self._rows(x, n, "trim_rows")
        need = self._lib.smi_trim_work_len(max(0, max(int(v) for v in n)) if B else 0, int(window), int(step), max(1, min(B, MAX_ROWS)))
        work = torch.empty((max(2, int(need)),), dtype=torch.int32, device=self.device)
        bounds = torch.empty((max(1, B), 2), dtype=torch.int32, device=self.device)
        self._lib.check(self._lib.smi_trim_rows(C.c_void_p(x.data_ptr()), x.shape[1], (C.c_int32 * B)(*[int(v) for v in n]), B, int(window),
                                                int(step), float(threshold), int(margin), C.c_void_p(work.data_ptr()), work.numel(),
                                                C.c_void_p(bounds.data_ptr()), self._stream()), "smi_trim_rows")
        return [(int(a), int(b)) for a, b in bounds.cpu().tolist()]

    def concat_layout(self, bounds: Sequence[Tuple[int, int]], gaps: Sequence[int]) -> Tuple[List[int], int]:
        """(the offset of every piece in the assembled waveform, its total length): ``smi_concat_layout``, pure host arithmetic"""
        B = len(bounds)
        if len(gaps) != B:
            raise ValueError("one gap per row")
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        off = (C.c_longlong * max(1, B))()
        total = self._lib.smi_concat_layout(i32(b[0] for b in bounds), i32(b[1] for b in bounds), i32(gaps), B, off)
        if total < 0:
            raise ValueError(f"concat_layout: 1..{MAX_ROWS} rows with 0 <= start <= end and gap >= 0, not {list(bounds)}, {list(gaps)}")
        return list(off)[:B], int(total)

    def concat_rows(self, x, bounds: Sequence[Tuple[int, int]], gaps: Sequence[int], fade: int, out=None,
                    n: Optional[Sequence[int]] = None):
        """Pieces ``x[b, start_b : end_b]`` into one waveform on the device, each non-empty piece behind ``gaps[b]`` zeros, its
        first and last min(``fade``, length // 2) samples weighted (include/sparkmi.h, smi_concat_rows).  ``n``: the rows' valid
        lengths (end <= n is checked; None: the stride).  ``out``: a contiguous 1-D float32 tensor on the device to write to (zeros from the total
        length to its end); None: one of exactly the total length (at least one sample).  Returns (out, total).  One launch,
        nothing waits."""
        import torch
        if n is None:
            n = [x.shape[1]] * len(bounds)
        B = self._rows(x, n, "concat_rows")
        if len(bounds) != B or len(gaps) != B:
            raise ValueError("one (start, end) and one gap per row")
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        st, en, gp = i32(b[0] for b in bounds), i32(b[1] for b in bounds), i32(gaps)
        if out is None:
            total = self._lib.smi_concat_layout(st, en, gp, B, None)
            out = torch.empty((max(1, int(total)),), dtype=torch.float32, device=self.device)   # (a bad row: the call below names it)
        elif out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("concat_rows: out must be a contiguous 1-D float32 tensor on the device")
        total = C.c_longlong()
        self._lib.check(self._lib.smi_concat_rows(C.c_void_p(x.data_ptr()), x.shape[1], i32(n), st, en, gp, B, int(fade),
                                                  C.c_void_p(out.data_ptr()), out.numel(), None, C.byref(total), self._stream()),
                        "smi_concat_rows")
        return out, int(total.value)

    def _spans(self, spans, B: int):
        if spans is None:
            return None, None
        if len(spans) != B:
            raise ValueError("one (start, end) per row")
        return (C.c_int32 * B)(*[int(s[0]) for s in spans]), (C.c_int32 * B)(*[int(s[1]) for s in spans])

    def loudness_rows(self, x, n: Sequence[int], spans: Optional[Sequence[Tuple[int, int]]] = None,
                      targets: Optional[Sequence[Optional[float]]] = None, max_gain_db: float = 20.0, ceiling: float = PEAK_CEILING,
                      sr: int = 16000, block: Optional[int] = None, coef: Optional[np.ndarray] = None):
        """The programme loudness (BS.1770; include/sparkmi.h, smi_loud_rows) of rows and the gain that brings each to its target.
        ``x``: [B][stride] float32 on the device, row b valid for ``n[b]``; ``spans``: (start, end) per row, None: the whole
        rows; ``targets``: LUFS per row, None (the row, or all of them): measure only, gain 1.  ``sr`` gives the weighting
        (``k_weighting``) and the block (``loudness_block``); ``coef`` / ``block`` replace them.  Returns stats [B][4] float64 on
        the device: (loudness, peak, gain, limit -- 0 none, 1 ``max_gain_db``, 2 ``ceiling``).  Four launches, nothing waits and
        nothing is copied.  The scratch is the object's own and only grows."""
        import torch
        B = self._rows(x, n, "loudness_rows")
        st, en = self._spans(spans, B)
        block = loudness_block(sr) if block is None else int(block)
        coef = np.ascontiguousarray(k_weighting(sr) if coef is None else coef, dtype=np.float64)
        if coef.shape != (10,):
            raise ValueError("coef holds b0 b1 b2 a1 a2 of two stages: 10 values")
        tg = [None] * B if targets is None else list(targets)
        if len(tg) != B:
            raise ValueError("one target per row")
        tg = (C.c_double * B)(*[math.nan if t is None else float(t) for t in tg])
        need = self._lib.smi_loud_work_len(max(0, max(int(v) for v in n)) if B else 0, block, max(1, min(B, MAX_ROWS)))
        work = getattr(self, "_loud_work", None)
        if work is None or work.numel() < need:
            work = self._loud_work = torch.empty((max(1, int(need)),), dtype=torch.float64, device=self.device)
        stats = torch.empty((max(1, B), 4), dtype=torch.float64, device=self.device)
        self._lib.check(self._lib.smi_loud_rows(C.c_void_p(x.data_ptr()), x.shape[1], (C.c_int32 * B)(*[int(v) for v in n]), st, en, B,
                                                coef.ctypes.data_as(C.POINTER(C.c_double)), block, tg, float(max_gain_db), float(ceiling),
                                                C.c_void_p(work.data_ptr()), work.numel(), C.c_void_p(stats.data_ptr()), self._stream()),
                        "smi_loud_rows")
        return stats

    def gain_rows(self, x, n: Sequence[int], stats, spans: Optional[Sequence[Tuple[int, int]]] = None, out=None):
        """Rows times their gain (include/sparkmi.h, smi_gain_rows): row b's span becomes fl32(fl64(x) * stats[b, 2]), the gain read
        on the device; the rest of the row is copied and the row is zeros from ``n[b]`` to the stride.  ``out``: None: a new
        [B][stride] tensor; ``x`` itself: in place; another contiguous [B][out_stride] float32 tensor on the device that does not
        overlap ``x``.  Returns ``out``.  One launch, nothing waits."""
        import torch
        B = self._rows(x, n, "gain_rows")
        st, en = self._spans(spans, B)
        if stats.dim() != 2 or stats.shape[0] < B or stats.shape[1] != 4 or stats.dtype != torch.float64 or not stats.is_contiguous() or not stats.is_cuda:
            raise ValueError("gain_rows takes the [B][4] float64 stats of loudness_rows, on the device")
        if out is None:
            out = torch.empty_like(x)
        elif out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("gain_rows: out must be a contiguous [B][out_stride] float32 tensor on the device")
        self._lib.check(self._lib.smi_gain_rows(C.c_void_p(x.data_ptr()), x.shape[1], (C.c_int32 * B)(*[int(v) for v in n]), st, en, B,
                                                C.c_void_p(stats.data_ptr()), C.c_void_p(out.data_ptr()), out.shape[1], self._stream()),
                        "smi_gain_rows")
        return out

    def limit_rows(self, x, n: Sequence[int], gains=None, spans: Optional[Sequence[Tuple[int, int]]] = None, ceiling: float = PEAK_CEILING,
                   mode: str = "true", lookahead: int = 40, release: int = 400, out=None):
        """The look-ahead limiter (include/sparkmi.h, smi_limit_rows): row b's span times its gain and a smoothed reduction that
        keeps every sample at or under ``ceiling``, the rest of the row copied, zeros from ``n[b]`` to the stride.  ``gains``:
        None: 1; the [B][4] float64 stats of ``loudness_rows`` (their gain is applied here, so ``gain_rows`` is not needed); or
        a [B] float64 tensor -- on the device, read there.  ``mode``: "true": peaks of the 4x oversampled signal
        (``resample_taps(4, 1)``); "sample": of the samples alone.  ``lookahead`` / ``release``: samples (``limiter_reach``); the
        window is ``limiter_window``.  ``out``: as in ``gain_rows`` (``x`` itself: in place).  Returns (out, stats [B][4]
        float64 on the device: the true peak going in, the gain, the smallest factor, the samples reduced).  A launch or more for
        the window, then three; nothing waits and nothing is copied.  The scratch is the object's own and only grows."""
        import torch
        B = self._rows(x, n, "limit_rows")
        st, en = self._spans(spans, B)
        if mode not in LIMITER_MODES:
            raise ValueError(f"mode must be \"true\" or \"sample\", not {mode!r}")
        A, R = int(lookahead), int(release)
        gp, gs = C.c_void_p(0), 0
        if gains is not None:
            ok = gains.dtype == torch.float64 and gains.is_contiguous() and gains.is_cuda and gains.shape[0] >= B
            if ok and gains.dim() == 2 and gains.shape[1] == 4:
                gp, gs = C.c_void_p(gains.data_ptr() + 16), 4
            elif ok and gains.dim() == 1:
                gp, gs = C.c_void_p(gains.data_ptr()), 1
            else:
                raise ValueError("limit_rows: gains is None, the [B][4] float64 stats of loudness_rows or a [B] float64 tensor, on the device")
        taps = np.ascontiguousarray(resample_taps(LIMITER_PHASES, 1), dtype=np.float64) if mode == "true" else None
        wins = self.__dict__.setdefault("_limit_windows", {})
        if (A, R) not in wins:
            wins[(A, R)] = np.ascontiguousarray(limiter_window(A, R), dtype=np.float64)
        win = wins[(A, R)]
        if out is None:
            out = torch.empty_like(x)
        elif out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("limit_rows: out must be a contiguous [B][out_stride] float32 tensor on the device")
        need = self._lib.smi_limit_work_len(max(0, max(int(v) for v in n)) if B else 0, max(1, min(B, MAX_ROWS)))
        work = getattr(self, "_limit_work", None)
        if work is None or work.numel() < need:
            work = self._limit_work = torch.empty((max(1, int(need)),), dtype=torch.float64, device=self.device)
        stats = torch.empty((max(1, B), 4), dtype=torch.float64, device=self.device)
        self._lib.check(self._lib.smi_limit_rows(C.c_void_p(x.data_ptr()), x.shape[1], (C.c_int32 * B)(*[int(v) for v in n]), st, en, B, gp, gs,
                                                 float(ceiling), None if taps is None else taps.ctypes.data_as(C.POINTER(C.c_double)),
                                                 0 if taps is None else taps.size, LIMITER_PHASES, A, R,
                                                 win.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(work.data_ptr()), work.numel(),
                                                 C.c_void_p(out.data_ptr()), out.shape[1], C.c_void_p(stats.data_ptr()), self._stream()),
                        "smi_limit_rows")
        return out, stats

    def tempo_rows(self, x, n: Sequence[int], tempos: Sequence, spans: Optional[Sequence[Tuple[int, int]]] = None, out=None,
                   sr: int = 16000, frame: Optional[Tuple[int, int]] = None):
        """A pitch-preserving time-scale change of rows (WSOLA; include/sparkmi.h, smi_tempo_rows).  ``x``: [B][stride] float32
        on the device, row b valid for ``n[b]``; ``tempos``: per row a number in [0.5, 2.0] (``tempo_ratio``; > 1: faster) or
        a (p, q) pair; ``spans``: (start, end) per row, None: the whole rows -- nothing outside a span is read.  ``sr`` gives
        the frame and the search radius (``tempo_frame``); ``frame`` = (N, D) replaces them.  ``out``: None: a new
        [B][max(1, longest output)] tensor; or a contiguous [B][out_stride] float32 tensor on the device that does not overlap
        ``x``.  Returns (y -- row b holds its ``m[b]`` samples, then zeros --, m, pos [B][frames] int32 on the device: every
        frame's place in its span).  Two launches, nothing waits and nothing is copied back."""
        import torch
        B = self._rows(x, n, "tempo_rows")
        st, en = self._spans(spans, B)
        if len(tempos) != B:
            raise ValueError("one tempo per row")
        pq = [(int(t[0]), int(t[1])) if isinstance(t, (tuple, list)) else tempo_ratio(t) for t in tempos]
        N, D = tempo_frame(sr) if frame is None else (int(frame[0]), int(frame[1]))
        lens = [int(s[1]) - int(s[0]) for s in spans] if spans is not None else [int(v) for v in n]
        frames = (C.c_longlong)()
        m_max = k_max = 0
        for (p, q), L in zip(pq, lens):   # (a bad row: the call below names it)
            m = self._lib.smi_tempo_layout(max(0, L), p, q, N, C.byref(frames))
            if m >= 0:
                m_max, k_max = max(m_max, int(m)), max(k_max, int(frames.value))
        wins = self.__dict__.setdefault("_tempo_windows", {})
        if N not in wins and N >= 2 and N % 2 == 0:
            wins[N] = torch.from_numpy(tempo_window(N)).to(self.device)
        win = wins.get(N)
        if out is None:
            out = torch.empty((max(1, B), max(1, m_max)), dtype=torch.float32, device=self.device)
        elif out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("tempo_rows: out must be a contiguous [B][out_stride] float32 tensor on the device")
        pos = torch.empty((max(1, B), max(1, k_max)), dtype=torch.int32, device=self.device)
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        got = (C.c_int32 * max(1, B))()
        self._lib.check(self._lib.smi_tempo_rows(C.c_void_p(x.data_ptr()), x.shape[1], i32(n), st, en, B, i32(a[0] for a in pq),
                                                 i32(a[1] for a in pq), N, D, C.c_void_p(win.data_ptr() if win is not None else 0),
                                                 C.c_void_p(pos.data_ptr()), pos.shape[1], C.c_void_p(out.data_ptr()), out.shape[1],
                                                 got, self._stream()), "smi_tempo_rows")
        return out, list(got)[:B], pos

    def _pitch_taps(self, ratios: Sequence[Tuple[int, int]]):
        """(pool tensor, {(up, down): (offset, count)}) with the fp32 taps of every (up, down) in ``ratios``: the object's own
        small cache, apart from the resampler handle's registration pool, which a long-lived server with per-request pitches
        must not fill.  The pool has ``PITCH_TAP_CACHE`` slots and is allocated once; a new ratio that finds no free slot takes
        the slot of the ratio that has been unused the longest and is not of this call.  The copy into a slot is enqueued on
        the stream the earlier launches that read the slot were enqueued on, so it runs behind them and nothing waits -- which
        holds only while every ``pitch_rows`` call of one ``DeviceAudio`` is made on the same HIP stream: keep them on one
        stream (as the ``Stream*`` classes ask), or give each stream a ``DeviceAudio`` of its own; a copy enqueued on another
        stream could overwrite taps that a launch in flight still reads.  Only a call with more distinct ratios than the pool
        has slots gets a larger pool."""
        import torch
        cache = self.__dict__.setdefault("_pitch_cache", {"pool": None, "where": {}})
        keys = list(dict.fromkeys(ratios))
        if cache["pool"] is None or len(keys) > cache["pool"].numel() // PITCH_TAP_SLOT:
            slots = max(PITCH_TAP_CACHE, len(keys))
            cache.update(pool=torch.empty((slots * PITCH_TAP_SLOT,), dtype=torch.float32, device=self.device), where={})
        where = cache["where"]
        slots = cache["pool"].numel() // PITCH_TAP_SLOT
        for k in keys:
            if k in where:
                where[k] = where.pop(k)      # (used now: to the end of the order)
                continue
            if len(where) < slots:
                off = len(where) * PITCH_TAP_SLOT
            else:
                off = where.pop(next(o for o in where if o not in keys))[0]
            t = np.ascontiguousarray(resample_taps(*k).astype(np.float32))
            cache["pool"][off: off + t.size].copy_(torch.from_numpy(t))
            where[k] = (off, t.size)
        return cache["pool"], where

    def pitch_rows(self, x, n: Sequence[int], tempos: Sequence, pitches: Sequence, spans: Optional[Sequence[Tuple[int, int]]] = None,
                   out=None, sr: int = 16000, frame: Optional[Tuple[int, int]] = None):
        """A pitch shift of rows, with a tempo in the same pass (include/sparkmi.h, smi_pitch_rows): row b's span is stretched
        once by WSOLA at tempo (tp rq) / (tq rp), resampled by rq / rp on the way out and cut to ``tempo_len(L, tp, tq)``
        samples -- its own length where it has no tempo.  ``x``, ``n``, ``spans``, ``sr``, ``frame`` and ``out`` as in
        ``tempo_rows``; ``tempos``: per row None (1/1), a number in [0.5, 2.0] (``tempo_ratio``) or a (p, q) pair; ``pitches``:
        per row None (1/1), a number of semitones in [-12, 12] (``pitch_ratio``; > 0: higher) or the frequency ratio as a
        (p, q) pair.  A row at pitch 1/1 is ``tempo_rows``' row bit for bit.  The formants move with the pitch.  Returns (y --
        row b holds its ``m[b]`` samples, then zeros --, m, pos [B][frames] int32 on the device: the stretch's frame places).
        Two launches, nothing waits and nothing is copied back; a ratio's taps are copied to the device on its first use, into
        a cache of ``PITCH_TAP_CACHE`` slots that are taken over in turn: make all calls of one object on one HIP stream."""
        import torch
        B = self._rows(x, n, "pitch_rows")
        st, en = self._spans(spans, B)
        if len(tempos) != B or len(pitches) != B:
            raise ValueError("one tempo and one pitch per row")
        pair = lambda v, f: (1, 1) if v is None else (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else f(v)   # noqa: E731
        tt = [pair(t, tempo_ratio) for t in tempos]
        rr = [pair(r, pitch_ratio) for r in pitches]
        N, D = tempo_frame(sr) if frame is None else (int(frame[0]), int(frame[1]))
        lens = [int(s[1]) - int(s[0]) for s in spans] if spans is not None else [int(v) for v in n]
        frames, up, down = C.c_longlong(), C.c_int(), C.c_int()
        m_max = k_max = 0
        updown: List[Optional[Tuple[int, int]]] = []
        for (tp, tq), (rp, rq), L in zip(tt, rr, lens):   # (a bad row: the call below names it)
            m = self._lib.smi_pitch_layout(max(0, L), tp, tq, rp, rq, N, None, None, None, C.byref(frames), C.byref(up), C.byref(down))
            updown.append((up.value, down.value) if m >= 0 and (up.value, down.value) != (1, 1) else None)
            if m >= 0:
                m_max, k_max = max(m_max, int(m)), max(k_max, int(frames.value))
            if updown[-1] is not None and 20 * max(updown[-1]) + 1 > PITCH_TAP_SLOT:
                raise ValueError(f"pitch_rows: the pitch ratio {rp}/{rq} needs a filter of {20 * max(updown[-1]) + 1} taps, above the "
                                 f"{PITCH_TAP_SLOT} a cached ratio may take (ratios of hundredths need at most 3981)")
        pool, where = self._pitch_taps([k for k in updown if k is not None]) if any(k is not None for k in updown) else (None, {})
        wins = self.__dict__.setdefault("_tempo_windows", {})
        if N not in wins and N >= 2 and N % 2 == 0:
            wins[N] = torch.from_numpy(tempo_window(N)).to(self.device)
        win = wins.get(N)
        if out is None:
            out = torch.empty((max(1, B), max(1, m_max)), dtype=torch.float32, device=self.device)
        elif out.dim() != 2 or out.shape[0] != B or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("pitch_rows: out must be a contiguous [B][out_stride] float32 tensor on the device")
        pos = torch.empty((max(1, B), max(1, k_max)), dtype=torch.int32, device=self.device)
        i32 = lambda v: (C.c_int32 * B)(*[int(a) for a in v])   # noqa: E731
        got = (C.c_int32 * max(1, B))()
        self._lib.check(self._lib.smi_pitch_rows(C.c_void_p(x.data_ptr()), x.shape[1], i32(n), st, en, B, i32(a[0] for a in tt),
                                                 i32(a[1] for a in tt), i32(a[0] for a in rr), i32(a[1] for a in rr), N, D,
                                                 C.c_void_p(win.data_ptr() if win is not None else 0),
                                                 C.c_void_p(pool.data_ptr() if pool is not None else 0), 0 if pool is None else pool.numel(),
                                                 i32(where[k][0] if k is not None else 0 for k in updown),
                                                 i32(where[k][1] if k is not None else 0 for k in updown),
                                                 C.c_void_p(pos.data_ptr()), pos.shape[1], C.c_void_p(out.data_ptr()), out.shape[1],
                                                 got, self._stream()), "smi_pitch_rows")
        return out, list(got)[:B], pos


class StreamJoiner:
    """Owns one ``smi_join`` handle (include/sparkmi.h): the overlapping chunks of streamed requests become contiguous, playable
    pieces on the device, cross-faded over ``overlap`` samples and, with ``up/down`` other than 1/1, resampled with the filter's
    state kept across chunk edges.  Request keys map to the handle's stream slots: ``open(key)`` takes a free slot, ``push``
    sends one poll's ready chunks, and a key's slot is free again after its last push.  ``max_streams`` slots suffice for a
    caller that never has more than that many requests between their ``open`` and their last ``push`` -- ``serve_stream`` sizes
    it as max(max_open, max_batch), the requests that can be admitted and unfinished at once.  All pushes go to the current HIP
    stream at the time of the call: keep them on one stream.  ``lib``: a stand-in library (tests watch the bookkeeping)."""

    def __init__(self, max_streams: int, max_chunk: int, overlap: int, up: int = 1, down: int = 1, device="cuda:0",
                 diag: bool = False, lib=None):
        from .streaming import join_history
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("StreamJoiner runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.max_streams, self.max_chunk, self.overlap = int(max_streams), int(max_chunk), int(overlap)
        self.up, self.down = int(up), int(down)
        if math.gcd(self.up, self.down) != 1:
            raise ValueError(f"up/down = {up}/{down} must be in lowest terms")
        copy = self.up == 1 and self.down == 1
        taps = np.zeros(1) if copy else np.ascontiguousarray(resample_taps(self.up, self.down), dtype=np.float64)
        self.half = 0 if copy else taps.size // 2
        self.history = join_history(self.up, self.down, self.half)
        fi = np.ascontiguousarray(np.linspace(0, 1, self.overlap), dtype=np.float64)
        fo = np.ascontiguousarray(np.linspace(1, 0, self.overlap), dtype=np.float64)
        pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_join_create(self.max_streams, self.max_chunk, self.overlap, pd(fi), pd(fo), self.up, self.down,
                                                  pd(taps), 1 if copy else int(taps.size), C.byref(self._h)), "smi_join_create")
        self._free: List[int] = list(range(self.max_streams))   # (open() hands out the lowest free slot)
        self._open: dict = {}       # key -> [slot, chunks pushed, N, K]
        self.calls = 0              # smi_join_push_rows calls so far: one launch each

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_join_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """forget every open key (an abandoned stream's slots come back)"""
        self._free = list(range(self.max_streams))
        self._open = {}

    def slot(self, key) -> Optional[int]:
        return self._open[key][0] if key in self._open else None

    def open(self, key) -> int:
        if key in self._open:
            raise ValueError(f"request {key}: already open")
        if not self._free:
            raise ValueError(f"StreamJoiner: all {self.max_streams} stream slots are in use")
        s = min(self._free)
        self._free.remove(s)
        self._lib.check(self._lib.smi_join_open(self._h, s), "smi_join_open")
        self._open[key] = [s, 0, 0, 0]
        return s

    def piece_lengths(self, rows: Sequence[Tuple]) -> List[int]:
        """the piece lengths ``push(x, rows)`` would return, without pushing (pure host arithmetic)"""
        from .streaming import join_piece_len
        state = {k: list(v) for k, v in self._open.items()}
        out = []
        for key, length, last in rows:
            st = state.setdefault(key, [None, 0, 0, 0])
            piece, st[2], st[3] = join_piece_len(self.overlap, self.up, self.down, self.half, st[1] == 0, st[2], st[3], length, last)
            st[1] += 1
            out.append(piece)
        return out

    def push(self, x, rows: Sequence[Tuple]):
        """``x``: [B][stride] float32 on the device, row b the ready chunk of request ``rows[b] = (key, length, last)``; a key not
        open yet is opened.  Returns (out [B][out_stride] float32 on the device -- row b holds its piece, then zeros --, the
        pieces' lengths); a length may be 0.  A request that appears twice (its last full chunk and its flush) makes two device
        calls (``streaming.split_calls``), each one launch; everything is enqueued on the current stream and nothing waits."""
        from .streaming import join_piece_len, split_calls
        B = len(rows)
        if not B:
            raise ValueError("push takes at least one row")
        if not self._fake:
            import torch
            if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("push takes a contiguous [B][stride] float32 tensor on the device, one row per chunk")
        want = self.piece_lengths(rows)      # raises for a bad length before anything is opened or pushed
        for key, _, _ in rows:
            if key not in self._open:
                self.open(key)
        stride = max(1, max(want))
        in_stride = 1 if self._fake else int(x.shape[1])
        out = None
        if not self._fake:
            out = torch.empty((B, stride), dtype=torch.float32, device=self.device)
        got_all: List[int] = []
        for a, b in split_calls([r[0] for r in rows]):
            n = b - a
            i32 = lambda v: (C.c_int32 * n)(*[int(t) for t in v])   # noqa: E731
            got = (C.c_int32 * n)()
            src = C.c_void_p(0 if self._fake else x.data_ptr() + 4 * a * in_stride)
            dst = C.c_void_p(0 if self._fake else out.data_ptr() + 4 * a * stride)
            self._lib.check(self._lib.smi_join_push_rows(self._h, src, in_stride, i32(self._open[r[0]][0] for r in rows[a:b]),
                                                         i32(r[1] for r in rows[a:b]), i32(bool(r[2]) for r in rows[a:b]), n, dst, stride,
                                                         got, None if self._fake else self._stream()), "smi_join_push_rows")
            self.calls += 1
            got_all += list(got)
            for key, length, last in rows[a:b]:
                st = self._open[key]
                _, st[2], st[3] = join_piece_len(self.overlap, self.up, self.down, self.half, st[1] == 0, st[2], st[3], length, last)
                st[1] += 1
                if last:
                    self._free.append(self._open.pop(key)[0])
        if not self._fake:
            assert got_all == want, (got_all, want)
        return out, want

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class StreamTempo:
    """Owns one ``smi_tempos`` handle (include/sparkmi.h): the speaking rate of joined streams is changed at unchanged pitch while
    they are still arriving -- WSOLA with the frame places and an input history kept on the device per stream, so that the
    concatenation of a stream's pieces is, bit for bit, ``DeviceAudio.tempo_rows`` of its whole input, whatever the chunking.
    Request keys map to the handle's stream slots as in ``StreamJoiner``: ``open(key, p, q)`` takes a free slot, ``push`` sends
    one poll's chunks, and a key's slot is free again after its last push.  A key that ``push`` meets unopened is opened at
    1/1, which copies its chunks with no latency.  ``frame`` = (N, D) (``tempo_frame``).  All pushes go to the current HIP
    stream at the time of the call: keep them on one stream.  ``lib``: a stand-in library (tests watch the bookkeeping)."""

    def __init__(self, max_streams: int, max_chunk: int, frame: Tuple[int, int], device="cuda:0", diag: bool = False, lib=None):
        from .streaming import tempo_history
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("StreamTempo runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.max_streams, self.max_chunk = int(max_streams), int(max_chunk)
        self.N, self.D = int(frame[0]), int(frame[1])
        self.history = tempo_history(self.N, self.D)
        win = np.ascontiguousarray(tempo_window(self.N), dtype=np.float64)
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_tempos_create(self.max_streams, self.max_chunk, self.N, self.D,
                                                    win.ctypes.data_as(C.POINTER(C.c_double)), C.byref(self._h)), "smi_tempos_create")
        self._free: List[int] = list(range(self.max_streams))   # (open() hands out the lowest free slot)
        self._open: dict = {}       # key -> [slot, p, q, n, frames emitted]
        self.calls = 0              # smi_tempos_push_rows calls so far: two launches each

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_tempos_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """forget every open key (an abandoned stream's slots come back)"""
        self._free = list(range(self.max_streams))
        self._open = {}

    def slot(self, key) -> Optional[int]:
        return self._open[key][0] if key in self._open else None

    def open(self, key, p: int = 1, q: int = 1) -> int:
        if key in self._open:
            raise ValueError(f"request {key}: already open")
        if not self._free:
            raise ValueError(f"StreamTempo: all {self.max_streams} stream slots are in use")
        s = min(self._free)
        self._lib.check(self._lib.smi_tempos_open(self._h, s, int(p), int(q)), "smi_tempos_open")
        self._free.remove(s)
        self._open[key] = [s, int(p), int(q), 0, 0]
        return s

    def piece_lengths(self, rows: Sequence[Tuple]) -> List[int]:
        """the piece lengths ``push(x, rows)`` would return, without pushing (pure host arithmetic)"""
        from .streaming import tempo_piece_len
        state = {k: list(v) for k, v in self._open.items()}
        out = []
        for key, length, last in rows:
            st = state.setdefault(key, [None, 1, 1, 0, 0])
            piece, st[3], st[4] = tempo_piece_len(st[1], st[2], self.N, self.D, st[3], st[4], length, last)
            out.append(piece)
        return out

    def push(self, x, rows: Sequence[Tuple], return_places: bool = False):
        """``x``: [B][stride] float32 on the device, row b the new samples of request ``rows[b] = (key, length, last)``.
        Returns (out [B][out_stride] float32 on the device -- row b holds its piece, then zeros --, the pieces' lengths); a
        length may be 0.  ``return_places``: also (pos [B][frames] int32 on the device, the places of the frames each push made
        final, and their counts).  A request that appears twice makes two device calls (``streaming.split_calls``), each two
        launches; everything is enqueued on the current stream, nothing waits and nothing is copied back."""
        from .streaming import split_calls, tempo_piece_len
        B = len(rows)
        if not B:
            raise ValueError("push takes at least one row")
        if not self._fake:
            import torch
            if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("push takes a contiguous [B][stride] float32 tensor on the device, one row per chunk")
        for _, length, _ in rows:
            if not 0 <= int(length) <= self.max_chunk:
                raise ValueError(f"a chunk of {length} samples is outside 0..max_chunk={self.max_chunk}")
        want = self.piece_lengths(rows)      # raises for a bad length before anything is opened or pushed
        for key, _, _ in rows:
            if key not in self._open:
                self.open(key)
        nf, state = [], {k: list(v) for k, v in self._open.items()}
        for key, length, last in rows:       # the frames every push makes final, for the places
            st = state[key]
            f0 = st[4]
            _, st[3], st[4] = tempo_piece_len(st[1], st[2], self.N, self.D, st[3], st[4], length, last)
            nf.append(st[4] - f0)
        stride, pstride = max(1, max(want)), max(1, max(nf))
        in_stride = 1 if self._fake else int(x.shape[1])
        out = pos = None
        if not self._fake:
            out = torch.empty((B, stride), dtype=torch.float32, device=self.device)
            if return_places:
                pos = torch.empty((B, pstride), dtype=torch.int32, device=self.device)
        got_all: List[int] = []
        for a, b in split_calls([r[0] for r in rows]):
            n = b - a
            i32 = lambda v: (C.c_int32 * n)(*[int(t) for t in v])   # noqa: E731
            got = (C.c_int32 * n)()
            src = C.c_void_p(0 if self._fake else x.data_ptr() + 4 * a * in_stride)
            dst = C.c_void_p(0 if self._fake else out.data_ptr() + 4 * a * stride)
            pdst = C.c_void_p(0 if pos is None else pos.data_ptr() + 4 * a * pstride)
            self._lib.check(self._lib.smi_tempos_push_rows(self._h, src, in_stride, i32(self._open[r[0]][0] for r in rows[a:b]),
                                                           i32(r[1] for r in rows[a:b]), i32(bool(r[2]) for r in rows[a:b]), n, pdst,
                                                           pstride, dst, stride, got, None if self._fake else self._stream()),
                            "smi_tempos_push_rows")
            self.calls += 1
            got_all += list(got)
            for key, length, last in rows[a:b]:
                st = self._open[key]
                _, st[3], st[4] = tempo_piece_len(st[1], st[2], self.N, self.D, st[3], st[4], length, last)
                if last:
                    self._free.append(self._open.pop(key)[0])
        if not self._fake:
            assert got_all == want, (got_all, want)
        return (out, want, pos, nf) if return_places else (out, want)

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


PITCH_STREAM_TAPS = 3981    # the longest filter of a hundredth ratio (199/100): what a ``StreamPitch`` slot holds by default


class StreamPitch:
    """Owns one ``smi_pitchs`` handle (include/sparkmi.h): the pitch of joined streams is moved, with a tempo in the same stretch
    pass, while they are still arriving -- ``StreamTempo``'s state at the stretch (tp rq) / (tq rp) plus the tail of the stretched
    signal the resampler's next outputs still reach, kept on the device per stream, so that the concatenation of a stream's
    pieces is, bit for bit, ``DeviceAudio.pitch_rows`` of its whole input, whatever the chunking.  The twin of ``StreamTempo``:
    ``open(key, tempo=(p, q), pitch=(rp, rq))`` takes a free slot and hands the slot the ratio's taps (``resample_taps(up,
    down)`` rounded to fp32 once), ``push`` sends one poll's chunks, and a key's slot is free again after its last push.  A key
    that ``push`` meets unopened is opened at 1/1 and 1/1, which copies its chunks with no latency; a key at the pitch ratio
    1/1 is ``StreamTempo``'s stream bit for bit.  ``frame`` = (N, D) (``tempo_frame``); ``max_taps``: the longest filter a
    stream may bring.  ``history`` and ``max_chunk`` bound a push's piece (``longest``).  All opens and pushes go to the
    current HIP stream at the time of the call: keep them on one stream.  ``lib``: a stand-in library (tests watch the
    bookkeeping)."""

    def __init__(self, max_streams: int, max_chunk: int, frame: Tuple[int, int], max_taps: int = PITCH_STREAM_TAPS, device="cuda:0",
                 diag: bool = False, lib=None):
        from .streaming import tempo_history
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("StreamPitch runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.max_streams, self.max_chunk, self.max_taps = int(max_streams), int(max_chunk), int(max_taps)
        self.N, self.D = int(frame[0]), int(frame[1])
        self.history = tempo_history(self.N, self.D)
        win = np.ascontiguousarray(tempo_window(self.N), dtype=np.float64)
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_pitchs_create(self.max_streams, self.max_chunk, self.N, self.D,
                                                    win.ctypes.data_as(C.POINTER(C.c_double)), self.max_taps, C.byref(self._h)),
                        "smi_pitchs_create")
        self._free: List[int] = list(range(self.max_streams))   # (open() hands out the lowest free slot)
        self._open: dict = {}       # key -> [slot, tp, tq, rp, rq, taps, n, frames emitted, outputs emitted]
        self._taps: dict = {}       # (up, down) -> the fp32 taps, built once
        self.calls = 0              # smi_pitchs_push_rows calls so far: two launches each

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_pitchs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """forget every open key (an abandoned stream's slots come back)"""
        self._free = list(range(self.max_streams))
        self._open = {}

    def slot(self, key) -> Optional[int]:
        return self._open[key][0] if key in self._open else None

    def longest(self) -> int:
        """what a push emits at most, whatever the streams' ratios: the stretch's longest piece (include/sparkmi.h, tempo of
        joined streams), resampled by at most 2 in the pipeline's range of ratios, and the stretched tail behind it"""
        return 2 * (4 * (self.history + self.max_chunk) + self.N) + self.max_taps + 2

    def open(self, key, tempo: Tuple[int, int] = (1, 1), pitch: Tuple[int, int] = (1, 1)) -> int:
        from .streaming import pitch_plan
        if key in self._open:
            raise ValueError(f"request {key}: already open")
        if not self._free:
            raise ValueError(f"StreamPitch: all {self.max_streams} stream slots are in use")
        tp, tq, rp, rq = int(tempo[0]), int(tempo[1]), int(pitch[0]), int(pitch[1])
        _, _, up, down = pitch_plan(tp, tq, rp, rq)
        taps = None
        if (up, down) != (1, 1):
            if (up, down) not in self._taps:
                self._taps[(up, down)] = np.ascontiguousarray(resample_taps(up, down).astype(np.float32))
            taps = self._taps[(up, down)]
        s = min(self._free)
        self._lib.check(self._lib.smi_pitchs_open(self._h, s, tp, tq, rp, rq,
                                                  None if taps is None else taps.ctypes.data_as(C.POINTER(C.c_float)),
                                                  0 if taps is None else int(taps.size), None if self._fake else self._stream()),
                        "smi_pitchs_open")
        self._free.remove(s)
        self._open[key] = [s, tp, tq, rp, rq, 0 if taps is None else int(taps.size), 0, 0, 0]
        return s

    def _step(self, st, length, last) -> int:
        """one push of ``length`` samples through the counters ``st`` (changed in place): its piece's length"""
        from .streaming import pitch_piece_len
        piece, st[6], st[7], st[8] = pitch_piece_len(st[1], st[2], st[3], st[4], self.N, self.D, st[5], st[6], st[7], st[8], length, last)
        return piece

    def _walk(self, rows: Sequence[Tuple]) -> List[Tuple]:
        """per row (piece length, frames made final, the counters after it): the pushes in order over a copy of the counters,
        so the frames are walked once a push"""
        state = {k: list(v) for k, v in self._open.items()}
        out = []
        for key, length, last in rows:
            st = state.setdefault(key, [None, 1, 1, 1, 1, 0, 0, 0, 0])
            f0 = st[7]
            piece = self._step(st, length, last)
            out.append((piece, st[7] - f0, tuple(st[6:9])))
        return out

    def piece_lengths(self, rows: Sequence[Tuple]) -> List[int]:
        """the piece lengths ``push(x, rows)`` would return, without pushing (pure host arithmetic)"""
        return [w[0] for w in self._walk(rows)]

    def push(self, x, rows: Sequence[Tuple], return_places: bool = False):
        """``x``: [B][stride] float32 on the device, row b the new samples of request ``rows[b] = (key, length, last)``.
        Returns (out [B][out_stride] float32 on the device -- row b holds its piece, then zeros --, the pieces' lengths); a
        length may be 0.  ``return_places``: also (pos [B][frames] int32 on the device, the places of the stretch's frames each
        push made final, and their counts).  A request that appears twice makes two device calls (``streaming.split_calls``),
        each two launches; everything is enqueued on the current stream, nothing waits and nothing is copied back."""
        from .streaming import split_calls
        B = len(rows)
        if not B:
            raise ValueError("push takes at least one row")
        if not self._fake:
            import torch
            if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("push takes a contiguous [B][stride] float32 tensor on the device, one row per chunk")
        for _, length, _ in rows:
            if not 0 <= int(length) <= self.max_chunk:
                raise ValueError(f"a chunk of {length} samples is outside 0..max_chunk={self.max_chunk}")
        walk = self._walk(rows)              # raises for a bad length before anything is opened or pushed
        want, nf = [w[0] for w in walk], [w[1] for w in walk]
        for key, _, _ in rows:
            if key not in self._open:
                self.open(key)
        stride, pstride = max(1, max(want)), max(1, max(nf))
        in_stride = 1 if self._fake else int(x.shape[1])
        out = pos = None
        if not self._fake:
            out = torch.empty((B, stride), dtype=torch.float32, device=self.device)
            if return_places:
                pos = torch.empty((B, pstride), dtype=torch.int32, device=self.device)
        got_all: List[int] = []
        for a, b in split_calls([r[0] for r in rows]):
            n = b - a
            i32 = lambda v: (C.c_int32 * n)(*[int(t) for t in v])   # noqa: E731
            got = (C.c_int32 * n)()
            src = C.c_void_p(0 if self._fake else x.data_ptr() + 4 * a * in_stride)
            dst = C.c_void_p(0 if self._fake else out.data_ptr() + 4 * a * stride)
            pdst = C.c_void_p(0 if pos is None else pos.data_ptr() + 4 * a * pstride)
            self._lib.check(self._lib.smi_pitchs_push_rows(self._h, src, in_stride, i32(self._open[r[0]][0] for r in rows[a:b]),
                                                           i32(r[1] for r in rows[a:b]), i32(bool(r[2]) for r in rows[a:b]), n, pdst,
                                                           pstride, dst, stride, got, None if self._fake else self._stream()),
                            "smi_pitchs_push_rows")
            self.calls += 1
            got_all += list(got)
            for (key, _, last), w in zip(rows[a:b], walk[a:b]):
                self._open[key][6:9] = w[2]
                if last:
                    self._free.append(self._open.pop(key)[0])
        if not self._fake:
            assert got_all == want, (got_all, want)
        return (out, want, pos, nf) if return_places else (out, want)

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class StreamLoudness:
    """Owns one ``smi_louds`` handle (include/sparkmi.h): joined streams are brought to a programme-loudness target while they
    are still arriving.  The gain follows the running BS.1770 loudness of what has arrived, knot by knot on the stream's absolute
    hops, moves at most ``max_slew_db`` a hop and stays under the peak ceiling; the filter's state, the hop sums, the blocks so
    far, the last knot and the input not yet emitted are kept on the device per stream, so that the concatenation of a stream's
    pieces does not depend, by a bit, on how the stream was chunked.  A piece leaves at most five hops (500 ms) behind its
    input.  Request keys map to the handle's stream slots as in ``StreamTempo``: ``open(key, target, ...)`` takes a free slot,
    ``push`` sends one poll's chunks, and a key's slot is free again after its last push.  A key that ``push`` meets unopened
    is opened without a target, which measures and copies.  ``max_seconds`` bounds a stream (its blocks are kept).  All pushes
    go to the current HIP stream at the time of the call: keep them on one stream.  ``lib``: a stand-in library."""

    def __init__(self, max_streams: int, max_chunk: int, sr: int = 16000, block: Optional[int] = None, coef: Optional[np.ndarray] = None,
                 max_seconds: float = 600.0, max_blocks: Optional[int] = None, device="cuda:0", diag: bool = False, lib=None):
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("StreamLoudness runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.max_streams, self.max_chunk = int(max_streams), int(max_chunk)
        self.block = loudness_block(sr) if block is None else int(block)
        if self.block < 4 or self.block % 4:
            raise ValueError(f"block={self.block} must be a positive multiple of 4")
        self.hop = self.block // 4
        self.max_blocks = int(max_blocks) if max_blocks is not None else max(1, int(math.ceil(max_seconds * sr / self.hop)))
        coef = np.ascontiguousarray(k_weighting(sr) if coef is None else coef, dtype=np.float64)
        if coef.shape != (10,):
            raise ValueError("coef holds b0 b1 b2 a1 a2 of two stages: 10 values")
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_louds_create(self.max_streams, self.max_chunk, self.block, coef.ctypes.data_as(C.POINTER(C.c_double)),
                                                   self.max_blocks, C.byref(self._h)), "smi_louds_create")
        self._free: List[int] = list(range(self.max_streams))   # (open() hands out the lowest free slot)
        self._open: dict = {}       # key -> [slot, n]
        self.calls = 0              # smi_louds_push_rows calls so far: five launches each
        self.last_stats = None      # [B][4] float64 on the device: the stats of the last push's rows

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_louds_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """forget every open key (an abandoned stream's slots come back)"""
        self._free = list(range(self.max_streams))
        self._open = {}

    def slot(self, key) -> Optional[int]:
        return self._open[key][0] if key in self._open else None

    def open(self, key, target: Optional[float] = None, max_gain_db: float = 20.0, ceiling: float = PEAK_CEILING,
             max_slew_db: float = 1.0) -> int:
        if key in self._open:
            raise ValueError(f"request {key}: already open")
        if not self._free:
            raise ValueError(f"StreamLoudness: all {self.max_streams} stream slots are in use")
        s = min(self._free)
        self._lib.check(self._lib.smi_louds_open(self._h, s, math.nan if target is None else float(target), float(max_gain_db),
                                                 float(ceiling), float(max_slew_db)), "smi_louds_open")
        self._free.remove(s)
        self._open[key] = [s, 0]
        return s

    def _walk(self, rows: Sequence[Tuple]):
        """(piece lengths, knots made) of ``push(x, rows)``, pure host arithmetic"""
        from .streaming import loudness_knots, loudness_piece_len
        state = {k: v[1] for k, v in self._open.items()}
        pieces, knots = [], []
        for key, length, last in rows:
            n = state.get(key, 0)
            piece, state[key], k = loudness_piece_len(self.block, n, length, last)
            pieces.append(piece)
            knots.append(k - loudness_knots(n, self.hop))
        return pieces, knots

    def piece_lengths(self, rows: Sequence[Tuple]) -> List[int]:
        """the piece lengths ``push(x, rows)`` would return, without pushing (pure host arithmetic)"""
        return self._walk(rows)[0]

    def push(self, x, rows: Sequence[Tuple], return_gains: bool = False):
        """``x``: [B][stride] float32 on the device, row b the new samples of request ``rows[b] = (key, length, last)``.
        Returns (out [B][out_stride] float32 on the device -- row b holds its piece, then zeros --, the pieces' lengths); a
        length may be 0.  ``return_gains``: also (gains [B][knots][2] float64 on the device -- (G_j, flags) of the knots each
        push made final --, their counts, and stats [B][4] float64 on the device: the loudness of the latest whole block (after
        a stream's last push: of the whole stream), the peak so far, the latest gain, the OR of the flags).  The stats are kept
        in ``last_stats`` either way.  A request that appears twice makes two device calls (``streaming.split_calls``), each
        five launches; everything is enqueued on the current stream, nothing waits and nothing is copied back."""
        from .streaming import split_calls
        B = len(rows)
        if not B:
            raise ValueError("push takes at least one row")
        if not self._fake:
            import torch
            if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("push takes a contiguous [B][stride] float32 tensor on the device, one row per chunk")
        for _, length, _ in rows:
            if not 0 <= int(length) <= self.max_chunk:
                raise ValueError(f"a chunk of {length} samples is outside 0..max_chunk={self.max_chunk}")
        want, nk = self._walk(rows)          # raises for a bad length before anything is opened or pushed
        for key, _, _ in rows:
            if key not in self._open:
                self.open(key)
        stride, gstride = max(1, max(want)), max(1, max(nk))
        in_stride = 1 if self._fake else int(x.shape[1])
        out = gains = stats = None
        if not self._fake:
            out = torch.empty((B, stride), dtype=torch.float32, device=self.device)
            stats = torch.empty((B, 4), dtype=torch.float64, device=self.device)
            if return_gains:
                gains = torch.empty((B, gstride, 2), dtype=torch.float64, device=self.device)
        got_all: List[int] = []
        for a, b in split_calls([r[0] for r in rows]):
            n = b - a
            i32 = lambda v: (C.c_int32 * n)(*[int(t) for t in v])   # noqa: E731
            got = (C.c_int32 * n)()
            src = C.c_void_p(0 if self._fake else x.data_ptr() + 4 * a * in_stride)
            dst = C.c_void_p(0 if self._fake else out.data_ptr() + 4 * a * stride)
            gdst = C.c_void_p(0 if gains is None else gains.data_ptr() + 16 * a * gstride)
            sdst = C.c_void_p(0 if stats is None else stats.data_ptr() + 32 * a)
            self._lib.check(self._lib.smi_louds_push_rows(self._h, src, in_stride, i32(self._open[r[0]][0] for r in rows[a:b]),
                                                          i32(r[1] for r in rows[a:b]), i32(bool(r[2]) for r in rows[a:b]), n, gdst,
                                                          2 * gstride, dst, stride, got, sdst, None if self._fake else self._stream()),
                            "smi_louds_push_rows")
            self.calls += 1
            got_all += list(got)
            for key, length, last in rows[a:b]:
                self._open[key][1] += int(length)
                if last:
                    self._free.append(self._open.pop(key)[0])
        if not self._fake:
            assert got_all == want, (got_all, want)
        self.last_stats = stats
        return (out, want, gains, nk, stats) if return_gains else (out, want)

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)


class StreamLimiter:
    """Owns one ``smi_limits`` handle (include/sparkmi.h): the look-ahead limiter of ``DeviceAudio.limit_rows`` for joined
    streams that are still arriving.  The limiter is feed-forward, so nothing is defined anew: the concatenation of a stream's
    pieces is ``limit_rows`` of its whole input at gain 1, bit for bit, however the stream was chunked; the input that a later
    sample can still read (at most ``2 (A + R) + 19`` samples) and the running stats are kept on the device per stream.  A piece
    leaves ``A + R + 10`` samples (28 ms at 16 kHz) behind its input, in both modes.  Request keys map to the handle's stream
    slots as in ``StreamLoudness``: ``open(key, mode, ceiling)`` takes a free slot, ``push`` sends one poll's chunks, and a
    key's slot is free again after its last push.  A key that ``push`` meets unopened is opened in the "true" mode at
    ``PEAK_CEILING``.  All pushes go to the current HIP stream at the time of the call: keep them on one stream.  ``lib``: a
    stand-in library."""

    def __init__(self, max_streams: int, max_chunk: int, sr: int = 16000, lookahead_ms: float = 2.5, release_ms: float = 25.0,
                 device="cuda:0", diag: bool = False, lib=None):
        self._lib = lib if lib is not None else _lib.pick(diag)
        self._fake = lib is not None
        self.device = device
        if not self._fake:
            import torch
            self.device = torch.device(device)
            if self.device.type != "cuda":
                raise _lib.SparkMIError("StreamLimiter runs on an MI355X only (device must be cuda:N); there is no CPU path")
        self.max_streams, self.max_chunk = int(max_streams), int(max_chunk)
        self.lookahead, self.release = limiter_reach(sr, lookahead_ms, release_ms)
        self.delay = self.lookahead + self.release + 10     # samples a piece leaves behind its input
        win = np.ascontiguousarray(limiter_window(self.lookahead, self.release), dtype=np.float64)
        taps = np.ascontiguousarray(resample_taps(LIMITER_PHASES, 1), dtype=np.float64)
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        self._h = C.c_void_p()
        self._lib.check(self._lib.smi_limits_create(self.max_streams, self.max_chunk, self.lookahead, self.release, dp(win), dp(taps),
                                                    taps.size, LIMITER_PHASES, C.byref(self._h)), "smi_limits_create")
        self._free: List[int] = list(range(self.max_streams))   # (open() hands out the lowest free slot)
        self._open: dict = {}       # key -> [slot, n]
        self.calls = 0              # smi_limits_push_rows calls so far: three launches each
        self.last_stats = None      # [B][4] float64 on the device: the stats of the last push's rows

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.smi_limits_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """forget every open key (an abandoned stream's slots come back)"""
        self._free = list(range(self.max_streams))
        self._open = {}

    def slot(self, key) -> Optional[int]:
        return self._open[key][0] if key in self._open else None

    def open(self, key, mode: str = "true", ceiling: float = PEAK_CEILING) -> int:
        if key in self._open:
            raise ValueError(f"request {key}: already open")
        if not isinstance(mode, str) or mode not in LIMITER_MODES:
            raise ValueError(f"mode must be \"true\" or \"sample\", not {mode!r}")
        if not self._free:
            raise ValueError(f"StreamLimiter: all {self.max_streams} stream slots are in use")
        s = min(self._free)
        self._lib.check(self._lib.smi_limits_open(self._h, s, int(mode == "true"), float(ceiling)), "smi_limits_open")
        self._free.remove(s)
        self._open[key] = [s, 0]
        return s

    def piece_lengths(self, rows: Sequence[Tuple]) -> List[int]:
        """the piece lengths ``push(x, rows)`` would return, without pushing (pure host arithmetic)"""
        from .streaming import limiter_piece_len
        state = {k: v[1] for k, v in self._open.items()}
        pieces = []
        for key, length, last in rows:
            piece, state[key] = limiter_piece_len(self.lookahead, self.release, state.get(key, 0), length, last)
            pieces.append(piece)
        return pieces

    def push(self, x, rows: Sequence[Tuple]):
        """``x``: [B][stride] float32 on the device, row b the new samples of request ``rows[b] = (key, length, last)``.
        Returns (out [B][out_stride] float32 on the device -- row b holds its piece, then zeros --, the pieces' lengths); a
        length may be 0.  ``last_stats`` holds [B][4] float64 on the device: the peak going in, 1, the smallest factor and the
        samples reduced, over what each row's stream has emitted so far (after its last push: over the whole stream).  A request
        that appears twice makes two device calls (``streaming.split_calls``), each three launches; everything is enqueued on
        the current stream, nothing waits and nothing is copied back."""
        from .streaming import split_calls
        B = len(rows)
        if not B:
            raise ValueError("push takes at least one row")
        if not self._fake:
            import torch
            if x.dim() != 2 or x.shape[0] != B or x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda:
                raise ValueError("push takes a contiguous [B][stride] float32 tensor on the device, one row per chunk")
        for _, length, _ in rows:
            if not 0 <= int(length) <= self.max_chunk:
                raise ValueError(f"a chunk of {length} samples is outside 0..max_chunk={self.max_chunk}")
        want = self.piece_lengths(rows)      # raises for a bad length before anything is opened or pushed
        for key, _, _ in rows:
            if key not in self._open:
                self.open(key)
        stride = max(1, max(want))
        in_stride = 1 if self._fake else int(x.shape[1])
        out = stats = None
        if not self._fake:
            out = torch.empty((B, stride), dtype=torch.float32, device=self.device)
            stats = torch.empty((B, 4), dtype=torch.float64, device=self.device)
        got_all: List[int] = []
        for a, b in split_calls([r[0] for r in rows]):
            n = b - a
            i32 = lambda v: (C.c_int32 * n)(*[int(t) for t in v])   # noqa: E731
            got = (C.c_int32 * n)()
            src = C.c_void_p(0 if self._fake else x.data_ptr() + 4 * a * in_stride)
            dst = C.c_void_p(0 if self._fake else out.data_ptr() + 4 * a * stride)
            sdst = C.c_void_p(0 if stats is None else stats.data_ptr() + 32 * a)
            self._lib.check(self._lib.smi_limits_push_rows(self._h, src, in_stride, i32(self._open[r[0]][0] for r in rows[a:b]),
                                                           i32(r[1] for r in rows[a:b]), i32(bool(r[2]) for r in rows[a:b]), n, dst,
                                                           stride, got, sdst, None if self._fake else self._stream()),
                            "smi_limits_push_rows")
            self.calls += 1
            got_all += list(got)
            for key, length, last in rows[a:b]:
                self._open[key][1] += int(length)
                if last:
                    self._free.append(self._open.pop(key)[0])
        if not self._fake:
            assert got_all == want, (got_all, want)
        self.last_stats = stats
        return out, want

    def _stream(self) -> C.c_void_p:
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
