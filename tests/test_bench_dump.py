"""bench.py --dump-outputs on the host: the files, dtypes and padding it writes for a ragged batch, and the fixed sample
that replaces a waveform over the size budget."""
import os

import numpy as np
import torch

import bench


def _fake_step(B=3, hop=4, lens=(5, 2, 4)):
    g = np.random.Generator(np.random.PCG64(7))
    T = max(lens)
    wav = torch.from_numpy(g.standard_normal((B, 1, hop * T)).astype(np.float32))
    toks = [g.integers(0, 1000, size=n).tolist() for n in lens]
    return wav, toks


def test_dump_writes_the_step_results(tmp_path):
    wav, toks = _fake_step()
    info = bench.dump_outputs(str(tmp_path / "d"), wav, toks, 0, 1)
    assert sorted(info["files"]) == ["tokens.npy", "wav.npy"]
    w = np.load(tmp_path / "d" / "wav.npy")
    t = np.load(tmp_path / "d" / "tokens.npy")
    assert w.dtype == np.float32 and np.array_equal(w, wav.numpy())
    assert t.dtype == np.float64 and t.shape == (3, 5)
    for b, r in enumerate(toks):
        assert t[b, : len(r)].tolist() == r and (t[b, len(r):] == -1).all()


def test_dump_samples_a_waveform_over_budget_the_same_way_every_time(tmp_path, monkeypatch):
    wav, toks = _fake_step(hop=400)
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4000)
    for d in ("a", "b"):
        info = bench.dump_outputs(str(tmp_path / d), wav, toks, 1, 2)
        assert sorted(info["files"]) == ["tokens_rank1.npy", "wav_sample_index_rank1.npy", "wav_sample_rank1.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) - 128 for f in info["files"]) <= 4000 // 2
    v, i = (np.load(tmp_path / "a" / f"{n}_rank1.npy") for n in ("wav_sample", "wav_sample_index"))
    assert v.dtype == np.float32 and i.dtype == np.float64 and len(v) == len(i) > 0 and (np.diff(i) > 0).all()
    assert np.array_equal(v, wav.numpy().reshape(-1)[i.astype(np.int64)])
    for n in ("wav_sample", "wav_sample_index", "tokens"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}_rank1.npy"), np.load(tmp_path / "b" / f"{n}_rank1.npy"))
