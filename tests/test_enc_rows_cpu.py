"""The host side of BiCodecEncoder.tokenize_rows on plain arrays, the device calls stubbed out: sort / pad / unsort, the frame
counts, the growth rule of the rows reservation, and the ValueErrors that must come before any device call."""
import numpy as np
import pytest
import torch

from sparkmi import config_tok as T
from sparkmi.encoder import BiCodecEncoder, grow_reservation, pack_rows, plan_rows


def test_plan_rows_sorts_stably_by_length_and_inverts():
    w = T.tiny_wav2vec2()
    ns = [5000, 720, 48000, 720, 20880]
    nr = [800, 900, 129, 300, 800]
    p = plan_rows(w, ns, nr)
    assert p["order"] == [3, 1, 0, 4, 2]                       # (720, 300), (720, 900), 5000, 20880, 48000
    assert p["n_samples"] == [720, 720, 5000, 20880, 48000] and p["n_ref"] == [300, 900, 800, 800, 129]
    assert p["frames"] == [w.frames(n) for n in p["n_samples"]] == [2, 2, 15, 65, 149]
    assert [p["order"][j] for j in p["inverse"]] == list(range(5))
    assert (p["wav_stride"], p["ref_stride"], p["sem_stride"]) == (48000, 900, 149)
    with pytest.raises(ValueError):
        plan_rows(w, [], [])
    with pytest.raises(ValueError):
        plan_rows(w, [720, 800], [300])


def test_pack_rows_pads_with_zeros_in_the_planned_order():
    a = [np.arange(1, 4, dtype=np.float64), np.arange(10, 15, dtype=np.float32).reshape(1, 5)]
    out = pack_rows(a, [1, 0], 6)
    assert out.dtype == np.float32 and out.shape == (2, 6)
    assert out.tolist() == [[10, 11, 12, 13, 14, 0], [1, 2, 3, 0, 0, 0]]


def test_reservation_grows_only_when_exceeded_and_never_shrinks():
    assert grow_reservation(None, (2, 1000, 500)) == (2, 1000, 500)
    assert grow_reservation((2, 1000, 500), (2, 1000, 500)) is None
    assert grow_reservation((2, 1000, 500), (1, 10, 5)) is None
    assert grow_reservation((2, 1000, 500), (3, 10, 5)) == (3, 1000, 500)
    assert grow_reservation((2, 1000, 500), (1, 1001, 600)) == (2, 1001, 600)


class _Stub(BiCodecEncoder):
    """tokenize_rows with the two device calls replaced: records them, returns ids that name the row they came from"""

    def __init__(self, max_samples=48000, max_ref=16256):
        self.wcfg, self.tcfg = T.tiny_wav2vec2(), T.tiny_tok()
        self.max_samples, self.max_ref = max_samples, max_ref
        self.reserves, self.calls = [], []
        self._h = None

    def _rows_reserve(self, rows, samples, ref):
        self.reserves.append((rows, samples, ref))

    def _rows_forward(self, wav, n_samples, ref, n_ref, sem_stride):
        self.calls.append((wav.copy(), list(n_samples), ref.copy(), list(n_ref), sem_stride))
        frames = [self.wcfg.frames(n) for n in n_samples]
        sem = torch.full((len(n_samples), sem_stride), -1, dtype=torch.int64)
        glob = torch.zeros((len(n_samples), self.tcfg.spk_token_num), dtype=torch.int32)
        for j, (n, f) in enumerate(zip(n_samples, frames)):
            sem[j, :f] = int(wav[j, 0])              # the first sample names the prompt
            glob[j] = int(ref[j, 0])
        return sem, glob, frames


def test_tokenize_rows_sorts_pads_and_unsorts():
    e = _Stub()
    ns, nr = [5000, 720, 20880], [800, 129, 300]
    wavs = [np.full(n, 10.0 + i, np.float32) for i, n in enumerate(ns)]
    refs = [np.full(n, 20.0 + i, np.float32) for i, n in enumerate(nr)]
    out = e.tokenize_rows(wavs, refs)
    wav, cns, ref, cnr, sstride = e.calls[0]
    assert cns == [720, 5000, 20880] and cnr == [129, 800, 300] and sstride == 65
    assert wav.shape == (3, 20880) and ref.shape == (3, 800)
    assert (wav[0, :720] == 11.0).all() and not wav[0, 720:].any() and (ref[1] == 20.0).all() and not ref[2, 300:].any()
    for i, (g, s) in enumerate(out):                                              # the caller's order
        assert g.shape == (1, 1, 8) and g.dtype == torch.int32 and (g == 20 + i).all()
        assert s.shape == (1, e.wcfg.frames(ns[i])) and s.dtype == torch.int64 and (s == 10 + i).all()
    assert e.reserves == [(3, 20880, 800)]
    e.tokenize_rows(wavs[:2], refs[:2])                                           # fits
    assert e.reserves == [(3, 20880, 800)]
    e.tokenize_rows(wavs + wavs[:1], [refs[0][:900 - 100]] * 3 + [np.zeros(900, np.float32)])   # one more row, a longer reference
    assert e.reserves == [(3, 20880, 800), (4, 20880, 900)]


def test_tokenize_rows_refuses_before_any_device_call():
    e = _Stub()
    ok, ref = np.zeros(720, np.float32), np.zeros(400, np.float32)
    with pytest.raises(ValueError, match="max_samples"):
        e.tokenize_rows([ok, np.zeros(48001, np.float32)], [ref, ref])
    with pytest.raises(ValueError, match="max_ref_samples"):
        e.tokenize_rows([ok], [np.zeros(16257, np.float32)])
    with pytest.raises(ValueError):
        e.tokenize_rows([ok, ok], [ref])
    with pytest.raises(ValueError):
        e.tokenize_rows([], [])
    assert e.reserves == [] and e.calls == []
