"""smi_voc_forward_rows (BiCodecVocoder.detokenize_rows): a ragged batch whose rows carry their solo bits.  Row b equals, bit
for bit, ``detokenize`` of that row alone (B = 1, T_max = its length) on a handle of the same config -- whatever else is in the
call, wherever the row sits, whatever the padding holds; samples past hop * length are zero."""
import numpy as np
import pytest
import torch

from sparkmi import config as C, weights as W

pytestmark = pytest.mark.gpu

# lengths that land in different launch plans (32- and 64-column tiles, channel split or not, small-grid kernel forms) and
# include partial tiles; equal lengths share a launch sequence, 50 / 400 are a scheduler's own chunk sizes
LENS = [50, 50, 400, 23, 97, 150]


def _voc(cfg, sd, **kw):
    from sparkmi.bicodec import BiCodecVocoder
    return BiCodecVocoder(cfg, sd, device="cuda:0", **kw)


def _check(cfg, sd, lens, max_frames, seed, folded=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    B, T = len(lens), max(lens)
    sem = rng.integers(0, cfg.codebook_size, size=(B, T))
    glob = rng.integers(0, 4096, size=(B, 1, cfg.spk_token_num))
    voc = _voc(cfg, sd, max_batch=B, max_frames=max_frames, state_is_folded=folded)
    one = _voc(cfg, sd, max_batch=1, max_frames=max_frames, state_is_folded=folded, arena=voc.arena)
    hop = cfg.hop
    solo = [one.detokenize(torch.from_numpy(sem[b:b + 1, :n]), torch.from_numpy(glob[b:b + 1])).cpu().numpy()[0, 0] for b, n in enumerate(lens)]
    wav = voc.detokenize_rows(torch.from_numpy(sem), torch.from_numpy(glob), lengths=lens).cpu().numpy()
    assert wav.shape == (B, 1, hop * T)
    compared = 0
    for b, n in enumerate(lens):
        assert solo[b].shape == (n * hop,) and np.abs(solo[b]).max() > 0
        assert np.array_equal(wav[b, 0, : n * hop], solo[b]), f"row {b} ({n} frames) differs from its solo run: max |diff| {np.abs(wav[b, 0, : n * hop] - solo[b]).max()}"
        assert not wav[b, 0, n * hop:].any(), f"row {b}: tail not zero"
        compared += 1
    assert compared == B
    # the same rows permuted, behind other padding garbage, in a wider call with other neighbours: the same bits
    perm = list(rng.permutation(B))
    extra = [7, 64]
    T2 = T + 19
    sem2 = rng.integers(0, cfg.codebook_size, size=(B + len(extra), T2))
    glob2 = rng.integers(0, 4096, size=(B + len(extra), 1, cfg.spk_token_num))
    lens2 = []
    for i, b in enumerate(perm):
        sem2[i + 1, : lens[b]] = sem[b, : lens[b]]     # rows 1 .. B; row 0 and the last row are strangers
        glob2[i + 1] = glob[b]
        lens2.append(lens[b])
    lens2 = [extra[0]] + lens2 + [extra[1]]
    wide = _voc(cfg, sd, max_batch=B + len(extra), max_frames=max_frames, state_is_folded=folded, arena=voc.arena)
    wav2 = wide.detokenize_rows(torch.from_numpy(sem2), torch.from_numpy(glob2), lengths=lens2).cpu().numpy()
    for i, b in enumerate(perm):
        n = lens[b]
        assert np.array_equal(wav2[i + 1, 0, : n * hop], solo[b]), f"row {b} changed at position {i + 1} of a wider call"
        assert not wav2[i + 1, 0, n * hop:].any()
    # more rows than the handle's max_batch: several calls, the same bits
    small = _voc(cfg, sd, max_batch=4, max_frames=max_frames, state_is_folded=folded, arena=voc.arena)
    wav3 = small.detokenize_rows(torch.from_numpy(sem), torch.from_numpy(glob), lengths=lens).cpu().numpy()
    assert np.array_equal(wav3, wav)
    # and the existing entry is what it was: a batched row is its solo run up to fp32 re-association
    plain = voc.detokenize(torch.from_numpy(sem), torch.from_numpy(glob), lengths=lens).cpu().numpy()
    for b, n in enumerate(lens):
        assert np.abs(plain[b, 0, : n * hop] - solo[b]).max() < 1e-4


def test_rows_carry_their_solo_bits_tiny():
    cfg = C.tiny_bicodec()
    _check(cfg, W.bicodec_detok_state(cfg), LENS, 512, seed=11)
    _check(cfg, W.bicodec_detok_state(cfg), [1, 33, 2, 64, 65, 31, 32, 128], 160, seed=12)


def test_rows_carry_their_solo_bits_full_size(full_voc):
    cfg, _, folded = full_voc
    _check(cfg, folded, LENS, 400, seed=13, folded=True)


def test_bad_arguments_are_reported():
    from sparkmi._lib import SparkMIError
    cfg = C.tiny_bicodec()
    voc = _voc(cfg, W.bicodec_detok_state(cfg), max_batch=2, max_frames=16)
    g = torch.zeros((1, 1, cfg.spk_token_num), dtype=torch.long)
    with pytest.raises(SparkMIError):
        voc.detokenize_rows(torch.zeros((1, 17), dtype=torch.long), g)
    with pytest.raises(SparkMIError):
        voc.detokenize_rows(torch.zeros((1, 8), dtype=torch.long), g, lengths=[0])
    with pytest.raises(ValueError):
        voc.detokenize_rows(torch.zeros((1, 8), dtype=torch.long), torch.zeros((1, 1, 3), dtype=torch.long))
