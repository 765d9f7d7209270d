"""The case table of tests/test_conv_forms_cpu.py and tests/test_conv_forms_gpu.py: one conv layer + call shape per kernel
form the launch builder (make_conv / run_launch, csrc/smi_net.h) can pick, the block shapes that reach k_resunit, k_convbT
and the wide k_dwln forms, the float64 reference, and the derived acceptance bound.  DESIGN.md 4.0.1 has the derivations.

Shapes are the smallest that meet each form's thresholds in make_conv:
  qb = 1      L <= 32, or fewer than 256 blocks at 64-column tiles          qb = 2   otherwise
  ks          nq * ceil(cot / 4) * B * S < 512 and Cin >= 8   (cot = 32-row output tiles, nq = time tiles)
  3 waves     exact pipe, not ks, cot in {3, 6, 9, ..} not a multiple of 4, nq * ceil(cot / 4) * B * S >= 2048
  chg = 4     K = 1, Cin >= 128 and (ks, or split pipe with a staged row <= 64 columns)
  chg = 2     split pipe: ks with several taps or Cin < 128; not ks with Cin >= 128, <= 3 taps, 64 < row <= 128 columns
  nc          staged row = (32 qb - 1) * istr + 1 + (K - 1) * dil columns, in units of 64
  WPF / WALL  ks forms on a grid of at most 512 blocks (WALL: stride 1, >= 4 taps)
  k_convbT    split pipe, not ks, S in {4, 8, 5}, Cin >= 64, >= 2048 blocks of 32 columns x (4 or 5) phases
Every case is ragged, its L is no multiple of 32, its Cin no multiple of the form's chunk, and a row ends inside a tile."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU, ACT_TANH, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3, 4


def _c(form, Cout, Cin, K=1, dil=1, S=1, istr=1, bf=False, B=2, L=45, lens=None, **kw):
    d = dict(form=form, Cout=Cout, Cin=Cin, K=K, dil=dil, S=S, istr=istr, bf=bf, B=B, L=L, lens=lens, gemv=False, c1=False, act=ACT_NONE)
    d.update(kw)
    return d


# name -> case; "form" is the kernel form the builder must pick (sparkmi.bicodec.form_name).  L = input positions of the longest row.
CONV_CASES = {
    # ---- k_conv: exact-fp32 matrix pipe
    "x_q1_co":        _c("k_conv<qb1,co,chg1,nc2>", 40, 20, 3, B=512, L=27),
    "x_q2_co":        _c("k_conv<qb2,co,chg1,nc2>", 40, 20, 3, B=16, L=2021),
    "x_q1_ks":        _c("k_conv<qb1,ks,chg1,nc2>", 40, 20, 3, B=3, L=45),
    "x_q1_ks_dil":    _c("k_conv<qb1,ks,chg1,nc2>", 40, 44, 7, dil=9, B=2, L=77),
    "x_q2_ks":        _c("k_conv<qb2,ks,chg1,nc2>", 250, 20, 3, B=4, L=499),
    "x_q1_co_s5":     _c("k_conv<qb1,co,chg1,nc3>", 40, 12, 8, istr=5, B=512, L=138),
    "x_q2_co_s2":     _c("k_conv<qb2,co,chg1,nc3>", 40, 12, 3, istr=2, B=16, L=4043),
    "x_q1_ks_s5":     _c("k_conv<qb1,ks,chg1,nc3>", 40, 20, 8, istr=5, B=3, L=228),
    "x_q2_ks_s2":     _c("k_conv<qb2,ks,chg1,nc3>", 250, 20, 3, istr=2, B=4, L=999),
    "x_q1_ks_s2":     _c("k_conv<qb1,ks,chg1,nc2>", 40, 20, 2, istr=2, B=3, L=91),
    "x_q1_3w":        _c("k_conv<qb1,co,chg1,nc2,3w>", 96, 12, 3, B=2048, L=27),
    "x_q2_3w":        _c("k_conv<qb2,co,chg1,nc2,3w>", 96, 12, 3, B=32, L=4070),
    "x_q1_3w_s5":     _c("k_conv<qb1,co,chg1,nc3,3w>", 96, 12, 8, istr=5, B=2048, L=138),
    "x_q2_3w_s2":     _c("k_conv<qb2,co,chg1,nc3,3w>", 96, 12, 3, istr=2, B=32, L=8141),
    "x_q1_ks_c4":     _c("k_conv<qb1,ks,chg4,nc1>", 250, 136, 1, B=100, L=27),
    "x_q2_ks_c4":     _c("k_conv<qb2,ks,chg4,nc1>", 250, 136, 1, B=10, L=583),
    "x_q1_wpf":       _c("k_conv<qb1,ks,chg4,nc1,wpf>", 250, 136, 1, B=3, L=45),
    "x_q1_wpf_3ch":   _c("k_conv<qb1,ks,chg4,nc1,wpf>", 70, 300, 1, B=2, L=45),
    "x_q2_wpf":       _c("k_conv<qb2,ks,chg4,nc1,wpf>", 250, 136, 1, B=4, L=499),
    "x_convT8_ks":    _c("k_conv<qb1,ks,chg1,nc2>", 40, 20, 16, S=8, B=2, L=45),
    "x_convT5_ks":    _c("k_conv<qb1,ks,chg1,nc2>", 40, 20, 11, S=5, B=2, L=45),
    # ---- k_convb: bf16-split matrix pipe
    "b_q1_co":        _c("k_convb<qb1,co,chg1,nc1>", 40, 40, 3, bf=True, B=512, L=27),
    "b_q1_co_wide":   _c("k_convb<qb1,co,chg1,nc2>", 40, 40, 7, dil=6, bf=True, B=512, L=27),
    "b_q2_co":        _c("k_convb<qb2,co,chg1,nc2>", 40, 40, 7, bf=True, B=16, L=2021),
    "b_q1_co_c2":     _c("k_convb<qb1,co,chg2,nc2>", 40, 136, 3, dil=17, bf=True, B=512, L=27),
    "b_q2_co_c2":     _c("k_convb<qb2,co,chg2,nc2>", 40, 136, 3, bf=True, B=16, L=2021),
    "b_q2_co_c2_T2":  _c("k_convb<qb2,co,chg2,nc2>", 40, 136, 4, S=2, bf=True, B=16, L=1003),
    "b_q1_co_c4":     _c("k_convb<qb1,co,chg4,nc1>", 40, 136, 1, bf=True, B=512, L=27),
    "b_q2_co_c4":     _c("k_convb<qb2,co,chg4,nc1>", 40, 136, 1, bf=True, B=16, L=2021),
    "b_q1_ks":        _c("k_convb<qb1,ks,chg2,nc1>", 40, 40, 3, bf=True, B=3, L=45),
    "b_q1_ks_wide":   _c("k_convb<qb1,ks,chg2,nc2>", 40, 40, 3, dil=17, bf=True, B=3, L=45),
    "b_q2_ks":        _c("k_convb<qb2,ks,chg2,nc2>", 250, 40, 3, bf=True, B=4, L=499),
    "b_q1_ks_T5":     _c("k_convb<qb1,ks,chg2,nc1>", 40, 40, 11, S=5, bf=True, B=2, L=45),
    "b_q1_wall":      _c("k_convb<qb1,ks,chg2,nc1,wall>", 40, 40, 7, bf=True, B=3, L=45),
    "b_q1_wall_wide": _c("k_convb<qb1,ks,chg2,nc2,wall>", 40, 40, 7, dil=9, bf=True, B=3, L=45),
    "b_q2_wall":      _c("k_convb<qb2,ks,chg2,nc2,wall>", 250, 40, 7, bf=True, B=4, L=499),
    "b_q1_ks_c4":     _c("k_convb<qb1,ks,chg4,nc1>", 250, 136, 1, bf=True, B=100, L=27),
    "b_q2_ks_c4":     _c("k_convb<qb2,ks,chg4,nc1>", 250, 136, 1, bf=True, B=10, L=583),
    "b_q1_wpf":       _c("k_convb<qb1,ks,chg4,nc1,wpf>", 250, 136, 1, bf=True, B=3, L=45),
    "b_q1_wpf_3ch":   _c("k_convb<qb1,ks,chg4,nc1,wpf>", 70, 300, 1, bf=True, B=2, L=45),
    "b_q2_wpf":       _c("k_convb<qb2,ks,chg4,nc1,wpf>", 250, 136, 1, bf=True, B=4, L=499),
    # ---- k_convbT: >= 2048 blocks of one 32-column tile x 4 / 5 phases
    "bT4":            _c("k_convbT<4>", 40, 72, 8, S=4, bf=True, B=64, L=997),
    "bT4_s8":         _c("k_convbT<4>", 40, 72, 16, S=8, bf=True, B=64, L=485),
    "bT5":            _c("k_convbT<5>", 40, 72, 11, S=5, bf=True, B=64, L=997),
    # ---- the two forms the callers of make_conv select
    "c1":             _c("k_conv_c1", 1, 22, 7, B=3, L=300, c1=True),
    "gemv":           _c("k_gemv1", 70, 100, 1, B=5, L=1, gemv=True),
}

# forms of the table that no argument tuple of make_conv reaches: form -> the builder condition that excludes it
UNREACHABLE = {
    "k_conv<qb1,co,chg4,nc1>": "`chg = (S == 1 && K == 1 && Cin >= 128 && ks) ? 4 : 1`: the exact pipe stages 128-channel chunks only with ks "
                               "(the other `chg = ... 4` needs `bf`)",
    "k_conv<qb2,co,chg4,nc1>": "`chg = (S == 1 && K == 1 && Cin >= 128 && ks) ? 4 : 1`: the exact pipe stages 128-channel chunks only with ks "
                               "(the other `chg = ... 4` needs `bf`)",
}

# What the builder must NOT run as asked: name -> (sparkmi.bicodec.conv_case arguments, None = smi_conv_plan refuses the case, or the
# form it plans instead).  xw = (32 qb - 1) istr + 1 + (K - 1) dil as above.
REFUSED = {
    # a strided 1-tap layer at qb2 stages 127 columns in 128-channel chunks (chg 4 takes one 64-column pass)
    "chg4_wide":    (dict(Cout=250, Cin=136, K=1, istr=2, B=4, L=999), None),
    # istr 5, K 8 at qb2: 323 columns, over the 192 of the widest exact form
    "strided_wide": (dict(Cout=40, Cin=12, K=8, istr=5, B=16, L=4043), None),
    "c1_cout2":     (dict(Cout=2, Cin=22, K=7, B=3, L=300, c1=True), None),
    "c1_residual":  (dict(Cout=1, Cin=22, K=7, B=3, L=300, c1=True, has_R=True), None),
    "gemv_bf":      (dict(Cout=70, Cin=100, K=1, B=5, L=1, bf=True, gemv=True), None),
    # the shape of case bT4 with a residual: k_convbT has a bias / Snake epilogue only, the layer stays on k_convb
    "bT4_residual": (dict(Cout=40, Cin=72, K=8, S=4, bf=True, B=64, L=997, has_R=True), "k_convb<qb2,co,chg1,nc2>"),
}

# chunk of a form in input channels (k_conv: 8 rows x waves x chg; k_convb: 32 x chg)
def form_chunk(form: str) -> int:
    if form.startswith("k_convbT"):
        return 64
    if form in ("k_conv_c1", "k_gemv1"):
        return 4 if form == "k_conv_c1" else 32
    chg = int(form.split("chg")[1][0])
    return (24 if ",3w" in form else 32) * chg


def case_lens(name):
    """Ragged rows: row 0 full, the others shorter, every one ending inside a 32-column tile of the OUTPUT grid."""
    c = CONV_CASES[name]
    if c["lens"] is not None:
        return list(c["lens"])
    if c["gemv"]:
        return [1] * c["B"]
    B, L = c["B"], c["L"]
    lo = min(L, (c["K"] - 1) * c["dil"] + 1 + 3 * c["istr"]) if c["istr"] > 1 else 2     # a strided conv needs a few outputs
    lens = [L] + [max(lo, L - 3 - (7 * b) % max(1, min(L - lo, 40))) for b in range(1, B)]
    return [min(L, v) for v in lens]


def out_len(c, n):
    if c["S"] > 1:
        return n * c["S"]
    if c["istr"] > 1:
        return (n - (c["K"] - 1) * c["dil"] - 1) // c["istr"] + 1
    return n


def make_case(name):
    """sparkmi conv_case struct of a table entry"""
    from sparkmi.bicodec import conv_case
    c = CONV_CASES[name]
    return conv_case(c["Cout"], c["Cin"], c["K"], c["dil"], c["S"], c["istr"], c["act"], c["bf"], c["B"], c["L"], gemv=c["gemv"], c1=c["c1"])


def reduction_length(c):
    """n of the bound: input channels x taps of a phase"""
    taps = c["K"] if c["S"] == 1 else -(-c["K"] // c["S"])
    return c["Cin"] * taps


def case_data(name):
    """Plain normal draws with a fixed seed: w (Conv1d (Cout, Cin, K) / ConvTranspose1d (Cin, Cout, K)), x (B, Cin, L) with the
    positions beyond a row's length ZERO, bias (Cout), lens."""
    c = CONV_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    shape = (c["Cin"], c["Cout"], c["K"]) if c["S"] > 1 else (c["Cout"], c["Cin"], c["K"])
    w = rng.standard_normal(shape).astype(np.float32)
    x = rng.standard_normal((c["B"], c["Cin"], c["L"])).astype(np.float32)
    bias = rng.standard_normal(c["Cout"]).astype(np.float32)
    lens = case_lens(name)
    for b, n in enumerate(lens):
        x[b, :, n:] = 0.0
    return w, x, bias, lens


def conv_f64(c, w, x):
    """The float64 contraction of a case (no bias): torch conv1d / conv_transpose1d on the CPU; (B, Cout, L_out)."""
    w = torch.as_tensor(np.asarray(w), dtype=torch.float64)
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    if c["gemv"]:
        return (x.reshape(c["B"], c["Cin"]) @ w[:, :, 0].T)[:, :, None]
    if c["S"] > 1:
        return F.conv_transpose1d(x, w, stride=c["S"], padding=(c["K"] - c["S"]) // 2)
    if c["istr"] > 1:
        return F.conv1d(x, w, stride=c["istr"], dilation=c["dil"])
    return F.conv1d(x, w, dilation=c["dil"], padding=c["dil"] * (c["K"] - 1) // 2)


def reference(name):
    """(ref, mag, lens, olens): ref = conv + bias in float64, mag = |W| (*) |x| in float64, both (B, Cout, L_out)"""
    c = CONV_CASES[name]
    w, x, bias, lens = case_data(name)
    ref = conv_f64(c, w, x) + torch.as_tensor(bias, dtype=torch.float64)[None, :, None]
    mag = conv_f64(c, np.abs(w), np.abs(x))
    return ref, mag, lens, [out_len(c, n) for n in lens]


def bound(c, ref, mag):
    """The per-element bound.  Exact pipe: n fp32 products accumulated in fp32, each rounding at most
    2^-24 of the running magnitude, <= (n + 8) 2^-24 (|W| (*) |x|) with the epilogue's roundings in the 8.  Split pipe: both
    operands kept to 16 mantissa bits (2^-17 relative each) and the mid x mid product (2^-16) dropped: 2^-15 of the
    magnitude on top of the accumulation term, plus the rounding of the bias add on the result."""
    n = reduction_length(c)
    if c["bf"]:
        return (2.0 ** -15 + (n + 8) * 2.0 ** -24) * mag + 2.0 ** -24 * ref.abs()
    return (n + 8) * 2.0 ** -24 * mag


def accept(c, got, ref, mag, olens):
    """The acceptance test of the contraction: every valid output finite and within the bound.  Returns (ok, worst ratio)."""
    got = torch.as_tensor(np.asarray(got), dtype=torch.float64)
    bnd = bound(c, ref, mag)
    worst, ok = 0.0, True
    for b, n in enumerate(olens):
        g, r, t = got[b, :, :n], ref[b, :, :n], bnd[b, :, :n]
        if not bool(torch.isfinite(g).all()):
            return False, float("inf")
        ratio = ((g - r).abs() / t.clamp_min(1e-300)).max().item() if n else 0.0
        worst = max(worst, ratio)
        ok = ok and ratio <= 1.0
    return ok, worst


def corruptions(name):
    """Three wrong float64 results a subtly broken kernel would give: one tap dropped, one input channel of the last chunk
    dropped, the last tile's columns shifted by one."""
    c = CONV_CASES[name]
    w, x, bias, lens = case_data(name)
    b64 = torch.as_tensor(bias, dtype=torch.float64)[None, :, None]
    out = {}
    w1 = w.copy(); w1[:, :, c["K"] - 1] = 0.0
    out["tap dropped"] = conv_f64(c, w1, x) + b64
    w2 = w.copy()
    if c["S"] > 1:
        w2[c["Cin"] - 1] = 0.0
    else:
        w2[:, c["Cin"] - 1] = 0.0
    out["channel dropped"] = conv_f64(c, w2, x) + b64
    ref = conv_f64(c, w, x) + b64
    if not c["gemv"]:
        sh = ref.clone()
        for b, n in enumerate(lens):
            on = out_len(c, n)
            q0 = (on - 1) // 32 * 32 if c["S"] == 1 else ((n - 1) // 32 * 32) * c["S"]
            if on - q0 >= 2:
                sh[b, :, q0:on] = torch.roll(ref[b, :, q0:on], 1, dims=-1)
            else:
                sh[b, :, q0:on] = ref[b, :, q0 - 1:on - 1]
        out["last tile shifted"] = sh
    return out


# ---- block shapes (sparkmi.bicodec.run_block / plan_block): name -> (kind, cfg kwargs, B, L, what the plan must contain)
BLOCK_RESUNIT, BLOCK_DECBLOCK, BLOCK_CONVNEXT = 0, 1, 2
BLOCK_CASES = {
    "res96_fused":   (BLOCK_RESUNIT, dict(C_=96), 64, 449, {"res_nwv": 3}),
    "res96_two":     (BLOCK_RESUNIT, dict(C_=96), 2, 77, {"forms": ["k_convb<qb1,ks,chg2,nc2,wall>", "k_convb<qb1,ks,chg2,nc1>"]}),
    "res192_fused":  (BLOCK_RESUNIT, dict(C_=192), 32, 449, {"res_nwv": 6}),
    "res192_two":    (BLOCK_RESUNIT, dict(C_=192), 2, 77, {"forms": ["k_convb<qb1,ks,chg2,nc2,wall>", "k_convb<qb1,ks,chg4,nc1,wpf>"]}),
    "dec_T4":        (BLOCK_DECBLOCK, dict(C_=72, Cout=32, K=8, S=4), 64, 997, {"forms": ["k_convbT<4>"]}),
    "dec_T5":        (BLOCK_DECBLOCK, dict(C_=72, Cout=32, K=11, S=5), 64, 997, {"forms": ["k_convbT<5>"]}),
    "dec_chg4":      (BLOCK_DECBLOCK, dict(C_=136, Cout=32, K=16, S=8), 64, 27, {"forms": ["k_convb<qb1,co,chg4,nc1>"]}),
    "dec_chg2":      (BLOCK_DECBLOCK, dict(C_=136, Cout=32, K=4, S=2), 16, 1003, {"forms": ["k_convb<qb2,co,chg2,nc2>"]}),
    "cnx_d100":      (BLOCK_CONVNEXT, dict(C_=100, I=72), 2, 45, {"cpt": 4}),
    "cnx_d200":      (BLOCK_CONVNEXT, dict(C_=200, I=72), 2, 45, {"cpt": 12}),
    "cnx_d400":      (BLOCK_CONVNEXT, dict(C_=400, I=72), 2, 45, {"cpt": 16}),
}


def block_lens(name):
    _, _, B, L, _ = BLOCK_CASES[name]
    return [L] + [L - 5 - (3 * b) % 17 for b in range(1, B)]


def block_params(name, dil=1, cond_dim=0):
    """Seeded weights of a block under the oracle's naming ("L." + the layer's state_dict keys), scaled so that activations stay
    O(1): conv weights N(0, 1) / sqrt(fan-in) (half that inside a ResidualUnit), Snake alphas in [1, 3]."""
    kind, kw, B, L, _ = BLOCK_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()) + dil)
    nrm = lambda *s: rng.standard_normal(s).astype(np.float32)
    p = {}

    def unit(u, C):
        p[u + ".0.alpha"] = rng.uniform(1.0, 3.0, (1, C, 1)).astype(np.float32)
        p[u + ".1.weight"] = nrm(C, C, 7) / np.float32(2 * np.sqrt(7 * C))
        p[u + ".1.bias"] = 0.1 * nrm(C)
        p[u + ".2.alpha"] = rng.uniform(1.0, 3.0, (1, C, 1)).astype(np.float32)
        p[u + ".3.weight"] = nrm(C, C, 1) / np.float32(2 * np.sqrt(C))
        p[u + ".3.bias"] = 0.1 * nrm(C)
    C = kw["C_"]
    if kind == BLOCK_RESUNIT:
        unit("L.block", C)
    elif kind == BLOCK_DECBLOCK:
        Co, K, S = kw["Cout"], kw["K"], kw["S"]
        p["L.block.0.alpha"] = rng.uniform(1.0, 3.0, (1, C, 1)).astype(np.float32)
        p["L.block.1.weight"] = nrm(C, Co, K) / np.float32(np.sqrt(C * K / S))
        p["L.block.1.bias"] = 0.1 * nrm(Co)
        for r in range(3):
            unit(f"L.block.{r + 2}.block", Co)
    else:
        I = kw["I"]
        p["L.dwconv.weight"] = nrm(C, 1, 7) / np.float32(np.sqrt(7))
        p["L.dwconv.bias"] = 0.1 * nrm(C)
        if cond_dim:
            for n in ("scale", "shift"):
                p[f"L.norm.{n}.weight"] = nrm(C, cond_dim) / np.float32(np.sqrt(cond_dim))
                p[f"L.norm.{n}.bias"] = (1.0 if n == "scale" else 0.0) + 0.1 * nrm(C)
        else:
            p["L.norm.weight"] = 1.0 + 0.1 * nrm(C)
            p["L.norm.bias"] = 0.1 * nrm(C)
        p["L.pwconv1.weight"] = nrm(I, C) / np.float32(np.sqrt(C))
        p["L.pwconv1.bias"] = 0.1 * nrm(I)
        p["L.pwconv2.weight"] = nrm(C, I) / np.float32(np.sqrt(I))
        p["L.pwconv2.bias"] = 0.1 * nrm(C)
        p["L.gamma"] = rng.uniform(0.5, 1.0, C).astype(np.float32)
    x = nrm(B, C, L)
    cond = nrm(B, cond_dim) if cond_dim else None
    return p, x, cond
