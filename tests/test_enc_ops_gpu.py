"""The prompt encoder's own kernels, one launch of a real launch list at a time, against float64 (tests/enc_cases.py has the
restatements, the derived bounds and the corruptions; tests/test_enc_ops_cpu.py checks on the host that every bound rejects
them).  Every test builds the launch list of an encode of a chosen (n_samples, n_ref) with `debug_build` -- the list the
graph path builds -- writes seeded inputs into the launch's input buffers, runs that ONE launch (found by name) with
`debug_run`, reads its output buffer and holds it to the restatement of the same inputs; it also asserts the grid / block /
dynamic LDS `debug_launches` reports, so that a case provably reaches the path it is named for.  RATIO lines carry the worst
|got - ref| / bound of each case (DESIGN.md 4.2.1 records them)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import enc_cases as ec
from oracle.tokenize_ref import BiCodecTokRef, get_ref_clip
from oracle.wav2vec2_ref import Wav2Vec2Ref
from sparkmi import weights as W
from sparkmi._lib import SparkMIError

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(12345.0)
PS = "speaker_encoder.perceiver_sampler"
SE2 = "speaker_encoder.speaker_encoder.layer2.se_res2block"
N_REF_MIN = ec.REF_NFFT // 2 + 1


def _make(wcfg, tcfg, vcfg, edit=None, **kw):
    from sparkmi.encoder import BiCodecEncoder
    wsd = W.wav2vec2_state(wcfg)
    tsd = dict(W.fold_weight_norm(W.bicodec_tok_state(tcfg, vcfg.vq_input_dim)))
    if edit:
        tsd.update(edit)
    wf = W.fold_pos_conv_weight_norm(wsd)
    enc = BiCodecEncoder(wcfg, tcfg, wf, tsd, "cuda:0", diag=True, **kw)
    return enc, wsd, wf, tsd


@functools.lru_cache(maxsize=None)
def _tiny(spk=8, heads=2, max_seconds=3.0):
    """tiny handle; ref_seconds 1.5 reaches Tk > 256 perceiver keys"""
    wcfg, tcfg, vcfg = ec.tiny_cfgs(spk_token_num=spk, perceiver_heads=heads)
    return _make(wcfg, tcfg, vcfg, max_seconds=max_seconds, ref_seconds=1.5) + (wcfg, tcfg)


@functools.lru_cache(maxsize=None)
def _long():
    """tiny handle that admits the kernel's 2040-frame limit (and one frame more, for the refusal)"""
    return _tiny(8, 2, 41.0)


@functools.lru_cache(maxsize=None)
def _wide():
    wcfg, tcfg, vcfg = ec.wide_cfgs()
    return _make(wcfg, tcfg, vcfg, max_seconds=3.0, ref_seconds=1.0) + (wcfg, tcfg)


def _launch(enc, name):
    hits = [l for l in enc.debug_launches() if l["name"] == name]
    assert len(hits) == 1, (name, [l["name"] for l in enc.debug_launches()])
    return hits[0]


def _run(enc, name):
    l = _launch(enc, name)
    enc.debug_run(l["index"])
    return l


def _ratio(kernel, case, r):
    print(f"RATIO {kernel} {case} worst error/bound {r:.4f}")


def _accept(kernel, case, got, ref, bnd):
    ok, r = ec.accept(got, ref, bnd)
    _ratio(kernel, case, r)
    assert ok, f"{kernel} {case}: worst |got - ref| / bound = {r}"


# ------------------------------------------------------------------ k_mha
def _mha_self(Tn):
    enc = _long()[0]
    frames, _ = enc.debug_build(ec.samples_for(Tn), 200)
    assert frames == Tn
    q, k, v, _ = ec.mha_inputs(f"self.{Tn}", 2, Tn, Tn)
    enc.debug_io("wide", np.concatenate([q, k, v], axis=0))
    enc.debug_io("att", np.full((128, Tn), SENTINEL))
    l = _run(enc, "w2v.encoder.layers.0.attention")
    assert l["kind"] == 9 and l["grid"] == ((Tn + 7) // 8, 2, 1) and l["block"] == 256 and l["lds"] == ec.mha_lds(Tn)
    got = enc.debug_io("att", count=128 * Tn).reshape(128, Tn)
    ref, _, bnd = ec.mha_ref(q, k, v, 2)
    _accept("k_mha", f"self T={Tn} lds={l['lds']}", got, ref, bnd)
    return l


@pytest.mark.parametrize("Tn", ec.MHA_SELF_T)
def test_mha_self_attention(Tn):
    """T = 9: one partial block of queries; 65: a second V tile of one key; 257: a second trip of the 256-thread score loop;
    1499: the default 30 s limit, 66,656 B of dynamic LDS -- above the 64 KB default window; 2040: the kernel's limit"""
    l = _mha_self(Tn)
    if Tn == 1499:
        assert l["lds"] == 66656 > 64 * 1024
    if Tn == 2040:
        assert l["lds"] == 83968 <= 96 * 1024


def test_mha_2041_frames_are_refused_on_the_host():
    enc = _long()[0]
    assert enc.max_samples >= ec.samples_for(2041)
    with pytest.raises(SparkMIError, match=r"code -1.*2041 frames"):
        enc.debug_build(ec.samples_for(2041), 200)
    with pytest.raises(SparkMIError, match=r"code -1.*2041 frames"):          # the product entry: the same check, before any launch
        enc.tokenize_arrays(np.zeros(ec.samples_for(2041), np.float32), np.zeros(200, np.float32))
    assert enc.debug_build(ec.samples_for(2040), 200)[0] == 2040             # the limit itself builds


@pytest.mark.parametrize("Nt,heads,n_ref", ec.MHA_CROSS)
def test_mha_cross_attention(Nt, heads, n_ref):
    enc = _tiny(Nt, heads)[0]
    enc.debug_build(ec.samples_for(2), n_ref)
    Tk, inner = Nt + n_ref // ec.REF_HOP + 1, heads * 64
    q, k, v, _ = ec.mha_inputs(f"cross.{Nt}.{heads}.{n_ref}", heads, Nt, Tk)
    enc.debug_io("pq", q)
    enc.debug_io("pkv", np.concatenate([k, v], axis=0))
    enc.debug_io("po", np.full((inner, Nt), SENTINEL))
    l = _run(enc, PS + ".layers.0.0.attend")
    assert l["grid"] == ((Nt + 7) // 8, heads, 1) and l["block"] == 256 and l["lds"] == ec.mha_lds(Tk)
    got = enc.debug_io("po", count=inner * Nt).reshape(inner, Nt)
    ref, _, bnd = ec.mha_ref(q, k, v, heads)
    _accept("k_mha", f"cross Nt={Nt} heads={heads} Tk={Tk}", got, ref, bnd)


# ------------------------------------------------------------------ k_posconv
def _posconv(handle, tag, Tn, Cg, K):
    enc, _, wf, _, wcfg, _ = handle
    enc.debug_build(ec.samples_for(Tn), 200)
    H = wcfg.hidden_size
    x = ec.normal(f"posconv.{tag}.{Tn}", (H, Tn))
    enc.debug_io("x", x)
    enc.debug_io("h", np.full((H, Tn), SENTINEL))
    l = _run(enc, "w2v.pos_conv+gelu+res")
    assert l["grid"] == ((Tn + 63) // 64, H // 16, 1) and l["block"] == 256 and l["lds"] == ec.posconv_lds(Cg, K)
    got = enc.debug_io("h", count=H * Tn).reshape(H, Tn)
    Wp, bp = wf["encoder.pos_conv_embed.conv.weight"], wf["encoder.pos_conv_embed.conv.bias"]
    assert Wp.shape == (H, Cg, K)
    ref, pre, mag = ec.posconv_ref(x, Wp, bp, wcfg.num_conv_pos_embedding_groups)
    _accept("k_posconv", f"{tag} Cg={Cg} K={K} T={Tn}", got, ref, ec.posconv_bound(x, pre, mag, Cg * K))
    return l


@pytest.mark.parametrize("Tn", ec.POSCONV_TINY_T)
def test_posconv_tiny(Tn):
    _posconv(_long(), "tiny", Tn, 32, 16)


@pytest.mark.parametrize("Tn", ec.POSCONV_WIDE_T)
def test_posconv_product_group_shape(Tn):
    """64 channels per group x 128 taps: the product's 48,896 B staged window"""
    assert _posconv(_wide(), "wide", Tn, 64, 128)["lds"] == 48896


# ------------------------------------------------------------------ k_dwln as the encoder uses it
LN_CASES = {   # name -> (handle, frames, launch, input buffer, output buffer, weights prefix (w2v / tok), eps, gelu, triple, k_dwln<cpt>)
    "wide.conv0.ln+gelu": ("wide", 3, "w2v.conv0.ln+gelu", "cf0", "cf1", ("w", "feature_extractor.conv_layers.0.layer_norm"), 1e-5, 1, 0, 16),
    "wide.feature_projection.ln": ("wide", 65, "w2v.feature_projection.ln", "cf1", "cf0", ("w", "feature_projection.layer_norm"), 1e-5, 0, 0, 16),
    "wide.ln1": ("wide", 65, "w2v.encoder.layers.0.ln1", "h", "x", ("w", "encoder.layers.0.layer_norm"), 1e-5, 0, 0, 32),
    "wide.final_layer_norm.3x": ("wide", 65, "encoder.encoder.final_layer_norm", "e2", "e1", ("t", "encoder.encoder.final_layer_norm"), 1e-6, 0, 1, 12),
    "tiny.conv0.ln+gelu": ("tiny", 3, "w2v.conv0.ln+gelu", "cf0", "cf1", ("w", "feature_extractor.conv_layers.0.layer_norm"), 1e-5, 1, 0, 2),
    "tiny.feature_projection.ln": ("tiny", 9, "w2v.feature_projection.ln", "cf1", "cf0", ("w", "feature_projection.layer_norm"), 1e-5, 0, 0, 2),
    "tiny.ln1": ("tiny", 9, "w2v.encoder.layers.0.ln1", "h", "x", ("w", "encoder.layers.0.layer_norm"), 1e-5, 0, 0, 4),
    "tiny.final_layer_norm.3x": ("tiny", 9, "encoder.encoder.final_layer_norm", "e2", "e1", ("t", "encoder.encoder.final_layer_norm"), 1e-6, 0, 1, 2),
}


@pytest.mark.parametrize("name", list(LN_CASES))
def test_layernorm_as_the_encoder_launches_it(name):
    hname, frames, launch, src, dst, (which, pfx), eps, gelu, triple, cpt = LN_CASES[name]
    enc, wsd, _, tsd, wcfg, tcfg = _wide() if hname == "wide" else _long()
    n = ec.samples_for(frames)
    enc.debug_build(n, 200)
    Tn = (n - 10) // 5 + 1 if "conv0" in launch else frames
    assert Tn % 8
    sd = wsd if which == "w" else tsd
    w, b = sd[pfx + ".weight"], sd[pfx + ".bias"]
    C_ = len(w)
    X = ec.normal("ln." + name, (C_, Tn), 1.5, 0.2)
    enc.debug_io(src, X)
    enc.debug_io(dst, np.full((C_, Tn), SENTINEL))
    l = _run(enc, launch)
    assert l["kind"] == 1 and l["grid"] == ((Tn + 7) // 8, 1, 1) and l["block"] == 256 and l["cpt"] == cpt
    got = enc.debug_io(dst, count=C_ * Tn).reshape(C_, Tn)
    ref, bnd = ec.ln_ref(X, w, b, eps, bool(gelu), bool(triple))
    _accept(f"k_dwln<{cpt}>", f"{name} C={C_} T={Tn} gelu={gelu} triple={triple}", got, ref, bnd)


# ------------------------------------------------------------------ k_wavnorm / k_conv0 / k_tap
@pytest.mark.parametrize("name", list(ec.WAVNORM_CASES))
def test_wavnorm(name):
    enc = _long()[0]
    x = ec.wavnorm_inputs(name)
    enc.debug_build(len(x), 200)
    enc.debug_io("in_wav", x)
    enc.debug_io("wavn", np.full(len(x) + 8, SENTINEL))
    l = _run(enc, "w2v.normalize")
    assert l["grid"] == (1, 1, 1) and l["block"] == 1024
    got = enc.debug_io("wavn", count=len(x) + 8)
    assert (got[len(x):] == SENTINEL).all()
    _accept("k_wavnorm", f"{name} n={len(x)}", got[:len(x)], ec.wavnorm_ref(x), ec.wavnorm_bound(x))


def test_conv0():
    enc, _, wf, _, wcfg, _ = _long()
    n = ec.samples_for(9)
    enc.debug_build(n, 200)
    T0, CD = (n - 10) // 5 + 1, wcfg.conv_dim[0]
    assert T0 % 256 and T0 > 256
    x = ec.normal("conv0", n)
    enc.debug_io("wavn", x)
    enc.debug_io("cf0", np.full((CD, T0), SENTINEL))
    l = _run(enc, "w2v.conv0")
    assert l["grid"] == ((T0 + 255) // 256, CD, 1) and l["block"] == 256
    got = enc.debug_io("cf0", count=CD * T0).reshape(CD, T0)
    ref, mag = ec.conv0_ref(x, wf["feature_extractor.conv_layers.0.conv.weight"][:, 0], wf["feature_extractor.conv_layers.0.conv.bias"], 5, T0)
    _accept("k_conv0", f"T0={T0}", got, ref, ec.conv0_bound(mag, 10))


def test_tap_three_modes():
    enc, _, _, _, wcfg, _ = _long()
    Tn, H = 9, wcfg.hidden_size
    enc.debug_build(ec.samples_for(Tn), 200)
    n = H * Tn
    assert n % 256
    h, acc0 = ec.normal("tap.h", (H, Tn)), ec.normal("tap.acc", (H, Tn), 2.0)
    a, b, c = wcfg.taps
    # mode 0 (first tap): acc = h, the same bits
    enc.debug_io("h", h); enc.debug_io("acc", np.full((H, Tn), SENTINEL))
    l = _run(enc, f"w2v.tap{a}")
    assert l["grid"] == ((Tn + 255) // 256, H, 1) and l["block"] == 256            # (channel, frame): the form the rows list runs
    assert ec.accept_equal(enc.debug_io("acc", count=n).reshape(H, Tn), h)
    # mode 1 (second tap): acc += h, in place -- one run
    enc.debug_io("acc", acc0)
    _run(enc, f"w2v.tap{b}")
    _accept("k_tap", "mode 1", enc.debug_io("acc", count=n).reshape(H, Tn), ec.tap_ref(h, acc0, 1), ec.tap_bound(h, acc0, 1))
    # mode 2 (third tap): feat = (acc + h) / 3
    enc.debug_io("acc", acc0); enc.debug_io("feat", np.full((H, Tn), SENTINEL))
    _run(enc, f"w2v.tap{c}")
    _accept("k_tap", "mode 2", enc.debug_io("feat", count=n).reshape(H, Tn), ec.tap_ref(h, acc0, 2), ec.tap_bound(h, acc0, 2))
    assert ec.accept_equal(enc.debug_io("acc", count=n).reshape(H, Tn), acc0)


# ------------------------------------------------------------------ k_frames / k_mag
@pytest.mark.parametrize("n_ref", [N_REF_MIN, 800, 1003, 80 * 260 + 5])
def test_frames_and_magnitude(n_ref):
    """the shortest accepted clip (n_fft / 2 + 1: both reflections inside one frame), a multiple of the hop, one that is not,
    and more than 256 frames (a second block)"""
    enc, _, _, _, _, tcfg = _tiny()
    enc.debug_build(ec.samples_for(2), n_ref)
    nfft, hop, nf = tcfg.n_fft, tcfg.hop_length, tcfg.n_fft // 2 + 1
    Tm = n_ref // hop + 1
    assert Tm % 256
    x = ec.normal(f"frames.{n_ref}", n_ref, 0.2)
    enc.debug_io("in_ref", x)
    enc.debug_io("frames", np.full((nfft, Tm), SENTINEL))
    l = _run(enc, "mel.frames")
    assert l["grid"] == ((Tm + 255) // 256, nfft, 1) and l["block"] == 256
    assert ec.accept_equal(enc.debug_io("frames", count=nfft * Tm).reshape(nfft, Tm), ec.frames_ref(x, nfft, hop))
    D = ec.normal(f"mag.{n_ref}", (2 * nf, Tm), 3.0)
    enc.debug_io("dft", D)
    enc.debug_io("mag", np.full((nf, Tm), SENTINEL))
    l = _run(enc, "mel.magnitude")
    assert l["grid"] == ((Tm + 255) // 256, nf, 1)
    _accept("k_mag", f"Tm={Tm}", enc.debug_io("mag", count=nf * Tm).reshape(nf, Tm), ec.mag_ref(D), ec.mag_bound(D))


def test_reference_clip_of_half_a_window_is_refused_on_the_host():
    enc = _tiny()[0]
    with pytest.raises(SparkMIError, match=r"code -1.*n_ref=128"):
        enc.debug_build(ec.samples_for(2), ec.REF_NFFT // 2)
    with pytest.raises(SparkMIError, match=r"code -1.*n_ref=128"):
        enc.tokenize_arrays(np.zeros(ec.samples_for(2), np.float32), np.zeros(ec.REF_NFFT // 2, np.float32))


# ------------------------------------------------------------------ k_rowmean / k_se / k_copy2d
@pytest.mark.parametrize("Tm", ec.ROWMEAN_TM)
def test_rowmean_se_and_res2_passthrough(Tm):
    enc, _, _, _, _, tcfg = _tiny()
    enc.debug_build(ec.samples_for(2), ec.REF_HOP * (Tm - 1) + 5)
    C_ = tcfg.ecapa_channels
    Wd = C_ // 8
    y = ec.normal(f"rowmean.{Tm}", (C_, Tm), 1.0, 0.3)
    enc.debug_io("ec_b", y)
    enc.debug_io("ec_vec", np.full(4 * (C_ + 128), SENTINEL))
    l = _run(enc, SE2 + ".3.mean")
    assert l["grid"] == ((C_ + 3) // 4, 1, 1) and l["block"] == 256
    vec = enc.debug_io("ec_vec", count=4 * (C_ + 128))
    assert (vec[C_:] == SENTINEL).all()
    _accept("k_rowmean", f"Tm={Tm}", vec[:C_], ec.rowmean_ref(y), ec.rowmean_bound(y))
    # SE tail: out = xin + y * s
    xin, s = ec.normal(f"se.x.{Tm}", (C_, Tm)), ec.normal(f"se.s.{Tm}", C_, 0.2, 0.5)
    enc.debug_io("ec_a", xin)
    enc.debug_io("ec_vec", s, offset=C_ + 128)
    enc.debug_io("ec_cat", np.full((C_, Tm), SENTINEL))
    l = _run(enc, SE2 + ".3.scale+res")
    assert l["grid"] == ((Tm + 255) // 256, C_, 1)
    _accept("k_se", f"Tm={Tm}", enc.debug_io("ec_cat", count=C_ * Tm).reshape(C_, Tm), ec.se_ref(xin, y, s), ec.se_bound(xin, y, s))
    # Res2 pass-through: the last branch's slice of y0 copied into y1, nothing else written
    enc.debug_io("ec_c", np.full((C_, Tm), SENTINEL))
    l = _run(enc, SE2 + ".1.passthrough")
    assert l["grid"] == ((Tm + 255) // 256, Wd, 1)
    got = enc.debug_io("ec_c", count=C_ * Tm).reshape(C_, Tm)
    assert ec.accept_equal(got[7 * Wd:], y[7 * Wd:]) and (got[:7 * Wd] == SENTINEL).all()


@pytest.mark.parametrize("Nt", ec.SPK_TOKEN_NUMS)
def test_latents_copy(Nt):
    enc, _, _, tsd, _, tcfg = _tiny(Nt, 2)
    n_ref = 800
    enc.debug_build(ec.samples_for(2), n_ref)
    Ld, Tk = tcfg.spk_latent_dim, Nt + n_ref // ec.REF_HOP + 1
    enc.debug_io("pctx", np.full((Ld, Tk), SENTINEL))
    l = _run(enc, PS + ".latents")
    assert l["grid"] == ((Nt + 255) // 256, Ld, 1)
    got = enc.debug_io("pctx", count=Ld * Tk).reshape(Ld, Tk)
    assert ec.accept_equal(got[:, :Nt], np.ascontiguousarray(tsd[PS + ".latents"].T)) and (got[:, Nt:] == SENTINEL).all()


# ------------------------------------------------------------------ k_geglu / k_rmsn
@pytest.mark.parametrize("Nt", ec.SPK_TOKEN_NUMS)
def test_geglu_and_rmsnorm(Nt):
    enc, _, _, tsd, _, tcfg = _tiny(Nt, 2)
    n_ref = 800
    enc.debug_build(ec.samples_for(2), n_ref)
    FI, Ld, Tk = tcfg.ff_inner, tcfg.spk_latent_dim, Nt + n_ref // ec.REF_HOP + 1
    X = ec.normal(f"geglu.{Nt}", (2 * FI, Nt), 1.5)
    enc.debug_io("pff", X)
    enc.debug_io("pg", np.full((FI, Nt), SENTINEL))
    l = _run(enc, PS + ".layers.0.1.geglu")
    assert l["grid"] == (1, FI, 1) and l["block"] == 64 * ((Nt + 63) // 64)
    _accept("k_geglu", f"Nt={Nt}", enc.debug_io("pg", count=FI * Nt).reshape(FI, Nt), ec.geglu_ref(X, FI), ec.geglu_bound(X, FI))
    ctx = ec.normal(f"rmsn.{Nt}", (Ld, Tk), 2.0)
    enc.debug_io("pctx", ctx)
    enc.debug_io("pout", np.full((Ld, Nt), SENTINEL))
    l = _run(enc, PS + ".norm")
    assert l["grid"] == ((Nt + 63) // 64, 1, 1) and l["block"] == 64
    g = tsd[PS + ".norm.gamma"]
    _accept("k_rmsn", f"Nt={Nt}", enc.debug_io("pout", count=Ld * Nt).reshape(Ld, Nt), ec.rmsn_ref(ctx[:, :Nt], g), ec.rmsn_bound(ctx[:, :Nt], g))


# ------------------------------------------------------------------ k_fsq_quant
@pytest.mark.parametrize("levels", ec.FSQ_LEVEL_SETS, ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("Nt", ec.SPK_TOKEN_NUMS)
def test_fsq_quant(levels, Nt):
    """even and odd levels, 1 / 5 / 6 / 8 dimensions; with an even first level one token sits exactly on -0.5 (see
    enc_cases.fsq_inputs) and must round to even; every id is also the half-to-even rounding of the kernel's OWN bounded values"""
    name = f"{'x'.join(map(str, levels))}.{Nt}"
    wcfg, tcfg, vcfg = ec.tiny_cfgs(spk_token_num=Nt, fsq_levels=list(levels))
    Ld, nd = tcfg.spk_latent_dim, len(levels)
    Wp, bp = ec.fsq_weights(name, levels, Ld)
    enc = _make(wcfg, tcfg, vcfg, edit={"speaker_encoder.quantizer.project_in.weight": Wp, "speaker_encoder.quantizer.project_in.bias": bp},
                max_seconds=1.0, ref_seconds=1.0)[0]
    enc.debug_build(ec.samples_for(2), 200)
    X, cand = ec.fsq_inputs(name, levels, Ld, Nt)
    enc.debug_io("pout", X)
    enc.debug_io("fsqb", np.full(Nt * 8, SENTINEL))
    l = _run(enc, "speaker_encoder.quantizer")
    assert l["grid"] == ((Nt + 63) // 64, 1, 1) and l["block"] == 64
    got_bd = enc.debug_io("fsqb", count=Nt * nd).reshape(Nt, nd)
    got = enc.debug_io("out_glob", count=Nt, dtype=np.int32)
    exact = np.zeros((Nt, nd), bool)
    for t in cand:
        exact[t, 0] = got_bd[t, 0] == np.float32(-0.5)
    if cand:
        assert exact.any(), f"no probe landed on -0.5: {got_bd[cand, 0]!r}"      # the half-to-even case is reached
    ids, bd, bnd, margin = ec.fsq_ref(X, Wp, bp, levels, exact_half=exact)
    _accept("k_fsq_quant", f"bounded {name}", got_bd, bd, bnd)
    planted = exact.any(axis=1)
    keep = np.ones(Nt, bool)
    keep[[t for t in cand if not planted[t]]] = False
    ok, excl = ec.accept_ids(got[keep], ids[keep], margin[keep], planted[keep])
    assert ok, f"ids differ from the float64 decision (excluded {excl}): {got[keep]} vs {ids[keep]}"
    lv = np.asarray(levels)
    basis = np.cumprod(np.concatenate([[1], lv[:-1]]))
    own = ((np.rint(got_bd.astype(np.float64)) + lv // 2) * basis).sum(axis=1).astype(np.int32)
    np.testing.assert_array_equal(got, own)
    for cname, bad in ec.fsq_corruptions(X, Wp, bp, levels, exact_half=exact).items():
        assert not np.array_equal(got[keep], bad[keep]), cname


# ------------------------------------------------------------------ k_cbnorm + k_vq
@pytest.mark.parametrize("ncode,D", ec.VQ_SHAPES)
def test_vq_argmax_ties_and_ragged_codebook(ncode, D):
    name = f"{ncode}.{D}"
    pairs = ec.vq_dup_pairs(ncode)
    cb = ec.vq_codebook(name, ncode, D, pairs)
    wcfg, tcfg, vcfg = ec.tiny_cfgs(codebook_size=ncode, codebook_dim=D)
    enc = _make(wcfg, tcfg, vcfg, edit={"quantizer.codebook.weight": cb}, max_seconds=2.0, ref_seconds=1.0)[0]   # k_cbnorm runs at create
    Tn = 67
    enc.debug_build(ec.samples_for(Tn), 200)
    Ze = ec.vq_inputs(name, cb, Tn, pairs)
    enc.debug_io("e0", Ze)
    enc.debug_io("out_sem", np.full(Tn, -7, dtype=np.int64))
    l = _run(enc, "quantizer.argmax")
    assert l["grid"] == (Tn, 1, 1) and l["block"] == 256
    got = enc.debug_io("out_sem", count=2 * Tn, dtype=np.int64)
    ids, margin, tie = ec.vq_ref(Ze, cb)
    assert 0 <= got[0] < ncode                                    # the all-zero frame: max(norm, 1e-12), a valid id
    n = len(pairs)
    assert tie[1:1 + n].all() and got[1:1 + n].tolist() == [i for i, _ in pairs], (got[1:1 + n], pairs)   # lowest index of every tie
    ok, excl = ec.accept_ids(got[1:], ids[1:], margin[1:])
    print(f"RATIO k_vq {name} excluded {excl:.4f}")
    assert ok, f"ids differ from the float64 decision (excluded {excl})"
    for cname, bad in ec.vq_corruptions(Ze, cb).items():
        assert not np.array_equal(got[1:], bad[1:]), cname


# ------------------------------------------------------------------ host refusals (no launch)
def test_perceiver_key_count_and_token_count_are_refused_on_the_host():
    from sparkmi import _lib
    from sparkmi.encoder import enc_cfg_struct
    import ctypes
    wcfg, tcfg, vcfg = ec.tiny_cfgs()
    d = _lib.diag()
    ok = enc_cfg_struct(wcfg, tcfg, 16000, 16000)
    assert d.smi_enc_arena_bytes(ctypes.byref(ok)) > 0
    # k_geglu's block is 64 * ceil(spk_tokens / 64) threads: 1024 is the last launchable count
    for spk, fine in ((1024, True), (1025, False)):
        cs = enc_cfg_struct(wcfg, dataclasses.replace(tcfg, spk_token_num=spk), 16000, 16000)
        assert (d.smi_enc_arena_bytes(ctypes.byref(cs)) > 0) == fine
    # create: spk_tokens + the mel frames of the longest reference clip must fit k_mha's 2040 keys (hop 80: 8 + 2033 > 2040)
    with pytest.raises(SparkMIError, match=r"code -1.*2040-key"):
        _make(wcfg, tcfg, vcfg, max_seconds=1.0, ref_seconds=(2032 * 80 - 256 + 0.5) / 16000.0)
    enc = _make(wcfg, tcfg, vcfg, max_seconds=1.0, ref_seconds=(2031 * 80 - 256 + 0.5) / 16000.0)[0]
    assert enc.max_ref // 80 + 1 + 8 == 2040
    frames, n = enc.debug_build(ec.samples_for(2), enc.max_ref)             # the limit itself builds: Tk = 2040
    assert _launch(enc, PS + ".layers.0.0.attend")["lds"] == 83968


# ------------------------------------------------------------------ whole encodes at the lengths the product allows
def _whole(enc, wcfg, tcfg, w2v, tok, Tn, seed):
    wav = (0.1 * np.random.default_rng(seed).standard_normal(ec.samples_for(Tn))).astype(np.float32)
    ref = get_ref_clip(wav, 16000, 1.0, tcfg.hop_length).astype(np.float32)
    glob, sem = enc.tokenize_arrays(wav, ref)
    assert sem.shape == (1, Tn)
    feat = w2v.features(wav)
    got_feat = enc.debug_stage("feat").cpu().numpy()
    err = np.abs(got_feat - feat[0].numpy().T).max()
    print(f"RATIO whole-encode T={Tn} max |feat - oracle| {err:.3e} (bar 3e-4)")
    assert err < 3e-4
    ost = {}
    osem, oglob = tok.tokenize(feat, torch.from_numpy(ref)[None], ost)
    safe = ost["vq_margin"].numpy() > ec.ID_MARGIN
    np.testing.assert_array_equal(sem.cpu().numpy()[safe], osem.numpy()[safe])
    bd = ost["fsq_bounded"][0].numpy()
    safe_g = (np.abs(bd - np.floor(bd) - 0.5) > ec.ID_MARGIN).all(axis=1)
    np.testing.assert_array_equal(glob.cpu().numpy()[0, 0][safe_g], oglob.numpy()[0, 0][safe_g])
    return wav, ref, glob, sem, got_feat


def test_whole_encode_at_the_default_30_s_limit_eager_capture_and_replay(monkeypatch):
    """T = 1499: k_mha's 66,656 B launch eagerly, then captured into a hipGraph (second call of the shape) and replayed
    (third): ids and feat bits equal an eager handle's (SPARKMI_ENC_GRAPH=0)."""
    wcfg, tcfg, vcfg = ec.tiny_cfgs()
    enc, wsd, _, tsd = _make(wcfg, tcfg, vcfg, ref_seconds=1.0)            # max_seconds = 30, the default
    w2v, tok = Wav2Vec2Ref(wcfg, wsd), BiCodecTokRef(tcfg, tsd)
    wav, ref, glob, sem, feat = _whole(enc, wcfg, tcfg, w2v, tok, 1499, 31)
    assert _launch(enc, "w2v.encoder.layers.0.attention")["lds"] == 66656
    monkeypatch.setenv("SPARKMI_ENC_GRAPH", "0")
    eager = _make(wcfg, tcfg, vcfg, ref_seconds=1.0)[0]
    ge, se = eager.tokenize_arrays(wav, ref)
    feat_e = eager.debug_stage("feat").cpu().numpy()
    assert torch.equal(ge, glob) and torch.equal(se, sem) and np.array_equal(feat_e, feat)
    for what in ("capture", "replay"):
        g2, s2 = enc.tokenize_arrays(wav, ref)
        assert torch.equal(g2, ge) and torch.equal(s2, se), what
        assert np.array_equal(enc.debug_stage("feat").cpu().numpy(), feat_e), what


def test_whole_encode_at_the_2040_frame_limit():
    enc, wsd, _, tsd, wcfg, tcfg = _long()
    _whole(enc, wcfg, tcfg, Wav2Vec2Ref(wcfg, wsd), BiCodecTokRef(tcfg, tsd), 2040, 32)
    assert _launch(enc, "w2v.encoder.layers.0.attention")["lds"] == 83968
