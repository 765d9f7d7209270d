"""tests/enc_cases.py checked on the host, no GPU: (1) every float64 restatement agrees with the existing fp32 oracle of the
same operation to fp32 noise, so the GPU tests compare against the operation the product is meant to compute; (2) every
acceptance bound passes the float64 reference rounded to fp32 and REJECTS every corruption -- a subtly wrong kernel's result
-- at the shapes the GPU tests run, so no bound is loose enough to hide the failure it is there to catch."""
import dataclasses

import numpy as np
import pytest
import torch

import enc_cases as ec
from oracle.tokenize_ref import BiCodecTokRef, mel_spectrogram
from oracle.wav2vec2_ref import Wav2Vec2Ref, zero_mean_unit_var
from sparkmi import config as C, config_tok as T, weights as W

F32_NOISE = 2e-5     # relative to the largest magnitude of the compared tensor: fp32 re-association of O(100)-term sums


def _close(a64, b32, tol=F32_NOISE):
    a64, b32 = np.asarray(a64, np.float64), np.asarray(b32, np.float64)
    assert a64.shape == b32.shape, (a64.shape, b32.shape)
    err = np.abs(a64 - b32).max()
    assert err <= tol * max(1.0, np.abs(a64).max()), err


def _check(ref, bnd, corruptions, what):
    """the reference rounded to fp32 passes; every corruption fails"""
    ok, r = ec.accept(np.asarray(ref, np.float32), ref, bnd)
    assert ok, f"{what}: the fp32-rounded reference misses its own bound (ratio {r})"
    assert corruptions, what
    for name, bad in corruptions.items():
        ok, r = ec.accept(np.asarray(bad, np.float32), ref, bnd)
        assert not ok, f"{what}: corruption '{name}' passes the bound (worst ratio {r})"


@pytest.fixture(scope="module")
def tiny():
    wcfg, tcfg, vcfg = ec.tiny_cfgs()
    wsd = W.wav2vec2_state(wcfg)
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    return wcfg, tcfg, W.fold_pos_conv_weight_norm(wsd), tsd, Wav2Vec2Ref(wcfg, wsd), BiCodecTokRef(tcfg, tsd)


def _lin(x_ct, w, b=None):
    y = np.asarray(w, np.float64) @ x_ct
    return y if b is None else y + np.asarray(b, np.float64)[:, None]


# ------------------------------------------------------------------ (1) restatements against the fp32 oracles
def test_wavnorm_restates_zero_mean_unit_var():
    for name in ec.WAVNORM_CASES:
        x = ec.wavnorm_inputs(name)
        ref = ec.wavnorm_ref(x)
        got = zero_mean_unit_var(x)
        # the oracle's fp32 mean / variance of a clip with a large offset are themselves only good to ~n U |mean| / spread
        n, mean, spread = ec.WAVNORM_CASES[name]
        tol = max(F32_NOISE, 64 * n * ec.U * abs(mean) / max(spread, 3.2e-4))
        _close(ref, got, tol)


def test_conv0_and_feature_ln_restate_the_feature_encoder(tiny):
    wcfg, _, wsd, _, _, _ = tiny
    x = ec.normal("cpu.conv0", 400 + 5 * 37)
    W0, b0 = wsd["feature_extractor.conv_layers.0.conv.weight"][:, 0], wsd["feature_extractor.conv_layers.0.conv.bias"]
    T0 = (len(x) - 10) // 5 + 1
    y, _ = ec.conv0_ref(x, W0, b0, 5, T0)
    want = torch.nn.functional.conv1d(torch.from_numpy(x)[None, None], torch.from_numpy(wsd["feature_extractor.conv_layers.0.conv.weight"]),
                                      torch.from_numpy(b0), stride=5)[0]
    _close(y, want.numpy())
    g, bb = wsd["feature_extractor.conv_layers.0.layer_norm.weight"], wsd["feature_extractor.conv_layers.0.layer_norm.bias"]
    z, _ = ec.ln_ref(want.numpy(), g, bb, 1e-5, gelu=True)
    want2 = torch.nn.functional.gelu(torch.nn.functional.layer_norm(want.T, (want.shape[0],), torch.from_numpy(g), torch.from_numpy(bb), 1e-5)).T
    _close(z, want2.numpy())


def test_posconv_restates_the_oracle(tiny):
    wcfg, _, wsd, _, w2v, _ = tiny
    for Tn in (2, 21):
        x = ec.normal(f"cpu.posconv.{Tn}", (wcfg.hidden_size, Tn))
        ref, _, _ = ec.posconv_ref(x, wsd["encoder.pos_conv_embed.conv.weight"], wsd["encoder.pos_conv_embed.conv.bias"],
                                   wcfg.num_conv_pos_embedding_groups)
        h = torch.from_numpy(x.T.copy())[None]
        _close(ref, (h + w2v.pos_conv(h))[0].numpy().T)


def test_ln_mha_restate_a_transformer_layer(tiny):
    wcfg, _, wsd, _, w2v, _ = tiny
    H, Tn, heads = wcfg.hidden_size, 23, wcfg.num_attention_heads
    h = ec.normal("cpu.layer", (H, Tn))
    p = "encoder.layers.1"
    x, _ = ec.ln_ref(h, wsd[p + ".layer_norm.weight"], wsd[p + ".layer_norm.bias"], wcfg.layer_norm_eps)
    q, k, v = (_lin(x, wsd[f"{p}.attention.{n}_proj.weight"], wsd[f"{p}.attention.{n}_proj.bias"]) for n in "qkv")
    o, _, _ = ec.mha_ref(q, k, v, heads)
    h1 = h + _lin(o, wsd[p + ".attention.out_proj.weight"], wsd[p + ".attention.out_proj.bias"])
    x, _ = ec.ln_ref(h1, wsd[p + ".final_layer_norm.weight"], wsd[p + ".final_layer_norm.bias"], wcfg.layer_norm_eps)
    x = ec.gelu64(_lin(x, wsd[p + ".feed_forward.intermediate_dense.weight"], wsd[p + ".feed_forward.intermediate_dense.bias"]))
    h2 = h1 + _lin(x, wsd[p + ".feed_forward.output_dense.weight"], wsd[p + ".feed_forward.output_dense.bias"])
    want = w2v.layer(torch.from_numpy(h.T.copy())[None], 1)[0].numpy().T
    _close(h2, want)
    # the three taps: ((a + b) + c) / 3, the oracle's association order
    a, b, c = (ec.normal(f"cpu.tap{i}", (7, 5)) for i in range(3))
    acc = ec.tap_ref(b, ec.tap_ref(a, a, 0), 1)
    _close(ec.tap_ref(c, acc, 2), (torch.from_numpy(a) + torch.from_numpy(b) + torch.from_numpy(c)).numpy() / 3)


def test_mha_geglu_rmsn_restate_the_perceiver(tiny):
    _, tcfg, _, tsd, _, tok = tiny
    Tm, Nt, Ld, heads, FI = 13, tcfg.spk_token_num, tcfg.spk_latent_dim, tcfg.perceiver_heads, tcfg.ff_inner
    feats = ec.normal("cpu.perceiver", (tcfg.ecapa_out, Tm), 0.5)
    ps = "speaker_encoder.perceiver_sampler"
    ctx = np.concatenate([np.asarray(tsd[ps + ".latents"], np.float64).T, _lin(feats, tsd[ps + ".proj_context.weight"], tsd[ps + ".proj_context.bias"])], axis=1)
    for i in range(tcfg.perceiver_depth):
        a, f = f"{ps}.layers.{i}.0", f"{ps}.layers.{i}.1"
        q = _lin(ctx[:, :Nt], tsd[a + ".to_q.weight"])
        kv = _lin(ctx, tsd[a + ".to_kv.weight"])
        o, _, _ = ec.mha_ref(q, kv[:heads * 64], kv[heads * 64:], heads)
        ctx[:, :Nt] += _lin(o, tsd[a + ".to_out.weight"])
        ff = _lin(ctx[:, :Nt], tsd[f + ".0.weight"], tsd[f + ".0.bias"])
        ctx[:, :Nt] += _lin(ec.geglu_ref(ff, FI), tsd[f + ".2.weight"], tsd[f + ".2.bias"])
    out = ec.rmsn_ref(ctx[:, :Nt], tsd[ps + ".norm.gamma"])
    want = tok.perceiver(torch.from_numpy(feats.T.copy())[None])[0].numpy().T
    _close(out, want)


@pytest.mark.parametrize("levels", ec.FSQ_LEVEL_SETS, ids=lambda l: "x".join(map(str, l)))
def test_fsq_restates_the_oracle(levels):
    _, tcfg, vcfg = ec.tiny_cfgs(fsq_levels=list(levels))
    tsd = W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim))
    tok = BiCodecTokRef(tcfg, tsd)
    X = ec.normal("cpu.fsq", (tcfg.spk_latent_dim, 40))
    Wp, bp = tsd["speaker_encoder.quantizer.project_in.weight"], tsd["speaker_encoder.quantizer.project_in.bias"]
    ids, bd, _, margin = ec.fsq_ref(X, Wp, bp, levels)
    bo = []
    want = tok.fsq_indices(torch.from_numpy(X.T.copy())[None], bo)[0].numpy()
    _close(bd, bo[0][0].numpy())
    assert (margin > ec.ID_MARGIN).all()          # normal inputs leave every decision clear (the issue's measurement)
    np.testing.assert_array_equal(ids, want)


@pytest.mark.parametrize("ncode,D", ec.VQ_SHAPES + ((8192, 8),))
def test_vq_restates_the_oracle(ncode, D):
    _, tcfg, vcfg = ec.tiny_cfgs(codebook_size=ncode, codebook_dim=D)
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    tok = BiCodecTokRef(tcfg, tsd)
    z = ec.normal("cpu.vq", (1, tcfg.enc_out_channels, 300))
    ze = torch.nn.functional.conv1d(torch.from_numpy(z), torch.from_numpy(tsd["quantizer.in_project.weight"]),
                                    torch.from_numpy(tsd["quantizer.in_project.bias"]))[0].numpy()
    ids, margin, tie = ec.vq_ref(ze, tsd["quantizer.codebook.weight"])
    want = tok.vq_tokenize(torch.from_numpy(z))[0].numpy()
    safe = margin > ec.ID_MARGIN
    assert safe.mean() >= 0.95 and not tie.any()
    np.testing.assert_array_equal(ids[safe], want[safe])


def test_frames_mag_restate_the_mel_spectrogram(tiny):
    from sparkmi.encoder import dft_basis, mel_filterbank
    _, tcfg, _, _, _, _ = tiny
    for n in (tcfg.n_fft // 2 + 1, 800, 1003):
        x = ec.normal(f"cpu.mel.{n}", n, 0.2)
        fr = ec.frames_ref(x, tcfg.n_fft, tcfg.hop_length)
        assert fr.dtype == np.float32 and fr.shape == (tcfg.n_fft, n // tcfg.hop_length + 1)
        pad = torch.nn.functional.pad(torch.from_numpy(x)[None, None], (tcfg.n_fft // 2,) * 2, mode="reflect")[0, 0].numpy()
        np.testing.assert_array_equal(fr, np.lib.stride_tricks.sliding_window_view(pad, tcfg.n_fft)[::tcfg.hop_length].T)
        mag = ec.mag_ref(dft_basis(tcfg).astype(np.float64) @ fr.astype(np.float64))
        mel = mel_filterbank(tcfg).astype(np.float64) @ mag
        _close(mel, mel_spectrogram(torch.from_numpy(x)[None], tcfg)[0].numpy(), 1e-4)


# ------------------------------------------------------------------ (2) the bounds reject the corruptions
@pytest.mark.parametrize("name", list(ec.WAVNORM_CASES))
def test_wavnorm_bound(name):
    x = ec.wavnorm_inputs(name)
    _check(ec.wavnorm_ref(x), ec.wavnorm_bound(x), ec.wavnorm_corruptions(name), name)


def test_conv0_bound(tiny):
    wsd = tiny[2]
    W0, b0 = wsd["feature_extractor.conv_layers.0.conv.weight"][:, 0], wsd["feature_extractor.conv_layers.0.conv.bias"]
    x = ec.normal("conv0", ec.samples_for(9))
    T0 = (len(x) - 10) // 5 + 1
    ref, mag = ec.conv0_ref(x, W0, b0, 5, T0)
    W1 = W0.copy(); W1[:, -1] = 0
    _check(ref, ec.conv0_bound(mag, 10), {"last tap dropped": ec.conv0_ref(x, W1, b0, 5, T0)[0],
                                          "stride 4": ec.conv0_ref(x, W0, b0, 4, T0)[0]}, "conv0")


def _posconv_check(wcfg, wsd, Tn, tag):
    x = ec.normal(f"posconv.{tag}.{Tn}", (wcfg.hidden_size, Tn))
    Wp, bp, G = wsd["encoder.pos_conv_embed.conv.weight"], wsd["encoder.pos_conv_embed.conv.bias"], wcfg.num_conv_pos_embedding_groups
    ref, pre, mag = ec.posconv_ref(x, Wp, bp, G)
    _check(ref, ec.posconv_bound(x, pre, mag, Wp.shape[1] * Wp.shape[2]), ec.posconv_corruptions(x, Wp, bp, G), f"posconv {tag} T={Tn}")


@pytest.mark.parametrize("Tn", ec.POSCONV_TINY_T)
def test_posconv_bound_tiny(tiny, Tn):
    _posconv_check(tiny[0], tiny[2], Tn, "tiny")


def test_posconv_bound_wide():
    wcfg, _, _ = ec.wide_cfgs()
    wsd = W.fold_pos_conv_weight_norm(W.wav2vec2_state(wcfg))
    for Tn in ec.POSCONV_WIDE_T:
        _posconv_check(wcfg, wsd, Tn, "wide")


def _mha_check(name, heads, Tq, Tk):
    q, k, v, planted = ec.mha_inputs(name, heads, Tq, Tk)
    ref, probs, bnd = ec.mha_ref(q, k, v, heads)
    for j, r in planted:                       # every boundary key holds at least 10 % of some row's softmax mass
        assert probs[:, r, j].min() >= 0.1, (name, j, r, probs[:, r, j])
    assert {j for j, _ in planted} == set(ec.mha_boundaries(Tk))
    _check(ref, bnd, ec.mha_corruptions(q, k, v, heads), name)


@pytest.mark.parametrize("Tn", ec.MHA_SELF_T)
def test_mha_bound_self(Tn):
    _mha_check(f"self.{Tn}", 2, Tn, Tn)


@pytest.mark.parametrize("Nt,heads,n_ref", ec.MHA_CROSS)
def test_mha_bound_cross(Nt, heads, n_ref):
    _mha_check(f"cross.{Nt}.{heads}.{n_ref}", heads, Nt, Nt + n_ref // ec.REF_HOP + 1)


def test_mha_cross_table_covers_the_issue():
    tks = {(Nt, Nt + n // ec.REF_HOP + 1) for Nt, _, n in ec.MHA_CROSS}
    assert {Nt for Nt, _ in tks} == {5, 8, 70} and {h for _, h, _ in ec.MHA_CROSS} == {2, 3}
    assert any(tk == Nt + 3 for Nt, tk in tks) and any(65 <= tk <= 127 for _, tk in tks) and any(tk > 256 for _, tk in tks)
    assert all(n > ec.REF_NFFT // 2 for _, _, n in ec.MHA_CROSS)


def test_elementwise_bounds():
    h, acc = ec.normal("tap.h", (128, 9)), ec.normal("tap.acc", (128, 9), 2.0)
    assert ec.accept_equal(ec.tap_ref(h, acc, 0).astype(np.float32), h)
    ok, _ = ec.accept((acc + h), ec.tap_ref(h, acc, 1), ec.tap_bound(h, acc, 1))
    assert ok
    _check(ec.tap_ref(h, acc, 2), ec.tap_bound(h, acc, 2), ec.tap_corruptions(h, acc), "tap mode 2")
    D = ec.normal("mag", (2 * 129, 11), 3.0)
    _check(ec.mag_ref(D), ec.mag_bound(D), ec.mag_corruptions(D), "mag")
    for Tm in ec.ROWMEAN_TM:
        X = ec.normal(f"rowmean.{Tm}", (64, Tm), 1.0, 0.3)
        _check(ec.rowmean_ref(X), ec.rowmean_bound(X), ec.rowmean_corruptions(X), f"rowmean {Tm}")
        xin, y, s = ec.normal(f"se.x.{Tm}", (64, Tm)), ec.normal(f"se.y.{Tm}", (64, Tm)), ec.normal(f"se.s.{Tm}", 64, 0.2, 0.5)
        _check(ec.se_ref(xin, y, s), ec.se_bound(xin, y, s), ec.se_corruptions(xin, y, s), f"se {Tm}")
    for Nt in ec.SPK_TOKEN_NUMS:
        X = ec.normal(f"geglu.{Nt}", (2 * 42, Nt), 1.5)
        _check(ec.geglu_ref(X, 42), ec.geglu_bound(X, 42), ec.geglu_corruptions(X, 42), f"geglu {Nt}")
        X, g = ec.normal(f"rmsn.{Nt}", (16, Nt), 2.0), ec.normal("rmsn.g", 16, 0.1, 1.0)
        _check(ec.rmsn_ref(X, g), ec.rmsn_bound(X, g), ec.rmsn_corruptions(X, g), f"rmsn {Nt}")


def test_frames_selection_rejects_an_off_by_one_reflection():
    for n in (ec.REF_NFFT // 2 + 1, 800, 1003):
        x = ec.normal(f"frames.{n}", n, 0.2)
        ref = ec.frames_ref(x, ec.REF_NFFT, ec.REF_HOP)
        assert ec.accept_equal(ref.copy(), ref)
        for name, bad in ec.frames_corruptions(x, ec.REF_NFFT, ec.REF_HOP).items():
            assert not ec.accept_equal(bad, ref), (n, name)


@pytest.mark.parametrize("C_,eps,gelu,triple", [(32, 1e-5, True, False), (512, 1e-5, True, False), (512, 1e-5, False, False),
                                                (1024, 1e-5, False, False), (384, 1e-6, False, True), (32, 1e-6, False, True),
                                                (128, 1e-5, False, False)])
def test_ln_bound(C_, eps, gelu, triple):
    X = ec.normal(f"ln.{C_}.{gelu}.{triple}", (C_, 13), 1.5, 0.2)
    w, b = ec.normal("ln.w", C_, 0.1, 1.0), ec.normal("ln.b", C_, 0.05)
    ref, bnd = ec.ln_ref(X, w, b, eps, gelu, triple)
    _check(ref, bnd, ec.ln_corruptions(X, w, b, eps, gelu, triple), f"ln C={C_}")


@pytest.mark.parametrize("ncode,D", ec.VQ_SHAPES)
def test_vq_ids_and_ties(ncode, D):
    pairs = ec.vq_dup_pairs(ncode)
    cb = ec.vq_codebook(f"{ncode}.{D}", ncode, D, pairs)
    Ze = ec.vq_inputs(f"{ncode}.{D}", cb, 67, pairs)
    ids, margin, tie = ec.vq_ref(Ze, cb)
    assert tie[1:1 + len(pairs)].all() and (ids[1:1 + len(pairs)] == [i for i, _ in pairs]).all()     # the planted frames pick the kept (lowest) row
    assert (margin[1:] > ec.ID_MARGIN).mean() >= 0.95
    held = np.ones(67, bool); held[0] = False                      # the all-zero frame: every code ties in exact arithmetic
    ok, excl = ec.accept_ids(ids[held], ids[held], margin[held])
    assert ok and excl <= ec.ID_EXCLUDED_MAX
    cor = ec.vq_corruptions(Ze, cb)
    assert "higher index returned on a tie" in cor and (ncode % 256 == 0 or "last ragged trip of codes ignored" in cor)
    for name, bad in cor.items():
        assert not ec.accept_ids(bad[held], ids[held], margin[held])[0], name


@pytest.mark.parametrize("levels", ec.FSQ_LEVEL_SETS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("Nt", ec.SPK_TOKEN_NUMS)
def test_fsq_bound_and_ids(levels, Nt):
    name = f"{'x'.join(map(str, levels))}.{Nt}"
    Wp, bp = ec.fsq_weights(name, levels, 16)
    X, cand = ec.fsq_inputs(name, levels, 16, Nt)
    exact = np.zeros((Nt, len(levels)), bool)
    if cand:
        exact[cand[1], 0] = True               # on the host: the candidate built from numpy's own atanh
    ids, bd, bnd, margin = ec.fsq_ref(X, Wp, bp, levels, exact_half=exact)
    if cand:
        assert bd[cand[1], 0] == -0.5
    ok, r = ec.accept(bd.astype(np.float32), bd, bnd)
    assert ok, r
    planted = exact.any(axis=1)
    keep = np.ones(Nt, bool)
    keep[[t for t in cand if not planted[t]]] = False      # the probes one ulp off the boundary
    ids, margin, planted = ids[keep], margin[keep], planted[keep]
    ok, excl = ec.accept_ids(ids, ids, margin, planted)
    assert ok, excl
    cor = ec.fsq_corruptions(X, Wp, bp, levels, exact_half=exact)
    if len(levels) > 1 or levels[0] % 2:
        assert cor
    if any(L % 2 for L in levels):
        assert "an odd level treated as even" in cor
    if cand:
        assert "round half away from zero on the planted -0.5" in cor
    for cname, bad in cor.items():
        assert not ec.accept_ids(bad[keep], ids, margin, planted)[0], (name, cname)
