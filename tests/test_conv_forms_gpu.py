"""Every conv kernel form the launch builder can pick, one layer at a time, against float64 (tests/conv_cases.py has the case
table, the reference and the derived bound; tests/test_conv_forms_cpu.py checks on the host that the table reaches every
form and that the bound rejects a subtly wrong result).  A failure names the form: the test id is the case, the assertion
message carries the kernel form that ran."""
import functools

import numpy as np
import pytest
import torch

import conv_cases as cc

pytestmark = pytest.mark.gpu

TOL_EXACT, TOL_SPLIT = 1e-5, 2e-4      # the project's bars for O(1) outputs (tests/test_ops_gpu.py)
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _reference(name):
    return cc.reference(name)


def _family(name):
    return cc.CONV_CASES[name]["form"].split("<")[0]


# ------------------------------------------------------------------ contraction + masking, every case
@pytest.mark.parametrize("name", list(cc.CONV_CASES))
def test_contraction_against_float64(name):
    """bias only.  Inputs beyond a row's length are NaN and the output is pre-filled: valid outputs are finite and within the
    derived bound, positions beyond a row's output length still hold the fill (conv_finish, k_convbT and k_conv_c1 store only
    q < olen; k_gemv1 has no time axis), and the form that ran is the one the host-side plan names."""
    from sparkmi.bicodec import form_name, run_conv
    c = cc.CONV_CASES[name]
    w, x, bias, lens = cc.case_data(name)
    ref, mag, _, olens = _reference(name)
    xn = torch.from_numpy(x)
    for b, n in enumerate(lens):
        xn[b, :, n:] = float("nan")
    xin = xn[:, :, 0] if c["gemv"] else xn
    y, _, plan = run_conv(cc.make_case(name), w, xin.cuda(), bias=bias, lens=None if c["gemv"] else lens, fill=SENTINEL)
    form = form_name(plan.form.key())
    assert form == c["form"]
    y = y.cpu().reshape(ref.shape)
    ok, worst = cc.accept(c, y.numpy(), ref, mag, olens)
    print(f"RATIO {_family(name)} {name} {form} n={cc.reduction_length(c)} worst error/bound {worst:.4f}")
    assert ok, f"{form}: worst |got - ref| / bound = {worst}"
    for b, n in enumerate(olens):
        assert bool((y[b, :, n:] == SENTINEL).all()), f"{form}: row {b} wrote beyond its {n} outputs"


# ------------------------------------------------------------------ epilogue
def _snake64(y, a):
    return y + (1.0 / (a + 1e-9)) * torch.sin(a * y) ** 2


def _epilogue64(acc, *, bias=None, bbias=None, act=0, gamma=None, beta=None, R=None, out_scale=1.0):
    """conv_finish's formula order in float64"""
    t = lambda v: torch.as_tensor(np.asarray(v), dtype=torch.float64)
    y = acc.clone()
    if bias is not None:
        y = y + t(bias)[None, :, None]
    if bbias is not None:
        y = y + t(bbias)[:, :, None]
    if act == cc.ACT_GELU:
        y = torch.nn.functional.gelu(y)
    if act == cc.ACT_RELU:
        y = torch.relu(y)
    if gamma is not None:
        y = t(gamma)[None, :, None] * y
    if beta is not None:
        y = y + t(beta)[None, :, None]
    if R is not None:
        y = t(R) + y
    if act == cc.ACT_TANH:
        y = torch.tanh(y)
    if act == cc.ACT_SIGMOID:
        y = torch.sigmoid(y)
    if out_scale != 1.0:
        y = (y + y) + y
    return y


EPI_SHAPES = ["x_q1_co", "x_q1_ks", "x_q1_wpf", "x_q2_ks_s2", "b_q1_co_c4", "b_q1_wall", "b_q1_wpf", "b_q2_ks"]
EPI_VARIANTS = ["bbias_gelu_gamma_beta_R_x3", "relu_gamma_beta_x2", "tanh_R_aliases_Y", "snake_only", "snake_and_raw"]


@pytest.mark.parametrize("variant", EPI_VARIANTS)
@pytest.mark.parametrize("name", EPI_SHAPES)
def test_epilogue_against_float64(name, variant):
    """conv_finish's operands and activations on both pipes and both reduction modes; weights scaled so that outputs are O(1);
    Snake runs the library sine on the exact pipe and the hardware sine on the split pipe"""
    from sparkmi.bicodec import conv_case, run_conv
    c = cc.CONV_CASES[name]
    w, x, bias, lens = cc.case_data(name)
    rng = np.random.default_rng(7)
    w = (w / np.sqrt(cc.reduction_length(c))).astype(np.float32)
    Bn, Co = c["B"], c["Cout"]
    Lout = cc.out_len(c, c["L"])
    kw, act, x2 = {}, cc.ACT_NONE, None
    nrm = lambda *s: rng.standard_normal(s).astype(np.float32)
    want_y, want_ys, alias = True, False, False
    if variant == "bbias_gelu_gamma_beta_R_x3":
        act = cc.ACT_GELU
        kw = dict(bbias=nrm(Bn, Co), gamma=nrm(Co), beta=nrm(Co), R=nrm(Bn, Co, Lout), out_scale=3.0)
    elif variant == "relu_gamma_beta_x2":
        act = cc.ACT_RELU
        kw = dict(gamma=nrm(Co), beta=nrm(Co))
        if not c["bf"]:          # the second input is added while staging: k_conv only (the encoder's Res2Net branches)
            x2 = nrm(*x.shape)
            for b, n in enumerate(lens):
                x2[b, :, n:] = 0.0
    elif variant == "tanh_R_aliases_Y":
        act, alias = cc.ACT_TANH, True
        kw = dict(R=nrm(Bn, Co, Lout))
    else:
        want_ys, want_y = True, variant == "snake_and_raw"
        kw = dict(alpha=rng.uniform(0.5, 1.5, Co).astype(np.float32))
    case = conv_case(Co, c["Cin"], c["K"], c["dil"], c["S"], c["istr"], act, c["bf"], Bn, c["L"], has_R="R" in kw)
    y, ys, plan = run_conv(case, w, torch.from_numpy(x).cuda(), bias=bias, lens=lens, x2=x2, want_y=want_y, want_ys=want_ys,
                           r_aliases_y=alias, **kw)
    from sparkmi.bicodec import form_name
    form = form_name(plan.form.key())
    assert form == c["form"]
    acc = cc.conv_f64(c, w, x.astype(np.float64) + (0 if x2 is None else x2.astype(np.float64)))
    alpha = kw.pop("alpha", None)
    want = _epilogue64(acc, bias=bias, act=act, **kw)
    tol = TOL_SPLIT if c["bf"] else TOL_EXACT
    olens = [cc.out_len(c, n) for n in lens]
    outs = []
    if want_y:
        outs.append(("Y", y, want))
    if want_ys:
        outs.append(("Ys", ys, _snake64(want, torch.as_tensor(alpha, dtype=torch.float64)[None, :, None])))
    for tag, got, ref in outs:
        got = got.cpu().double()
        err = max(float((got[b, :, :n] - ref[b, :, :n]).abs().max()) for b, n in enumerate(olens))
        print(f"EPI {form} {variant} {tag} max abs err {err:.3e} (bar {tol})")
        assert err <= tol, f"{form} {tag}: {err}"


@pytest.mark.parametrize("tph_case", ["bT4", "bT5"])
def test_multi_phase_transposed_conv_epilogue(tph_case):
    """k_convbT knows bias, the raw output and the Snake'd output; the run entry rejects everything else, as check_conv does"""
    from sparkmi import _lib
    from sparkmi.bicodec import conv_case, form_name, run_conv
    c = dict(cc.CONV_CASES[tph_case])
    w, x, bias, lens = cc.case_data(tph_case)
    w = (w / np.sqrt(cc.reduction_length(c))).astype(np.float32)
    rng = np.random.default_rng(9)
    alpha = rng.uniform(0.5, 1.5, c["Cout"]).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y, ys, plan = run_conv(cc.make_case(tph_case), w, xd, bias=bias, lens=lens, alpha=alpha, want_ys=True)
    assert form_name(plan.form.key()) == c["form"]
    want = _epilogue64(cc.conv_f64(c, w, x), bias=bias)
    wants = _snake64(want, torch.as_tensor(alpha, dtype=torch.float64)[None, :, None])
    for got, ref in ((y, want), (ys, wants)):
        got = got.cpu().double()
        err = max(float((got[b, :, :n * c["S"]] - ref[b, :, :n * c["S"]]).abs().max()) for b, n in enumerate(lens))
        assert err <= TOL_SPLIT, err
    nrm = lambda *s: rng.standard_normal(s).astype(np.float32)
    for bad in (dict(bbias=nrm(c["B"], c["Cout"])), dict(gamma=nrm(c["Cout"])), dict(beta=nrm(c["Cout"])), dict(out_scale=3.0)):
        with pytest.raises(_lib.SparkMIError):
            run_conv(cc.make_case(tph_case), w, xd, bias=bias, lens=lens, **bad)


@pytest.mark.parametrize("act", [cc.ACT_NONE, cc.ACT_RELU, cc.ACT_SIGMOID, cc.ACT_TANH])
def test_vector_and_one_channel_epilogues(act):
    """k_gemv1: bias + ReLU / sigmoid; k_conv_c1: bias + ReLU / tanh"""
    from sparkmi.bicodec import conv_case, run_conv
    for name in ("gemv", "c1"):
        if (name == "gemv" and act == cc.ACT_TANH) or (name == "c1" and act == cc.ACT_SIGMOID):
            continue
        c = cc.CONV_CASES[name]
        w, x, bias, lens = cc.case_data(name)
        w = (w / np.sqrt(cc.reduction_length(c))).astype(np.float32)
        case = conv_case(c["Cout"], c["Cin"], c["K"], act=act, B=c["B"], L=c["L"], gemv=c["gemv"], c1=c["c1"])
        xin = torch.from_numpy(x[:, :, 0] if c["gemv"] else x).cuda()
        y, _, _ = run_conv(case, w, xin, bias=bias, lens=None if c["gemv"] else lens)
        want = _epilogue64(cc.conv_f64(c, w, x), bias=bias, act=act)
        y = y.cpu().double().reshape(want.shape)
        err = max(float((y[b, :, :n] - want[b, :, :n]).abs().max()) for b, n in enumerate(lens))
        assert err <= TOL_EXACT, (name, err)


# ------------------------------------------------------------------ one-row plan shape
@pytest.mark.parametrize("name", ["x_q1_ks", "x_q1_wpf", "b_q1_wall", "b_q1_wpf", "b_q1_ks_T5"])
def test_rows_of_a_planned_batch_equal_their_solo_runs(name):
    """a ragged batch run with the plan shape of ONE row (PlanShape: smi_voc_forward_rows): every row whose own plan is that plan
    equals its solo run bit for bit"""
    from sparkmi.bicodec import conv_case, form_name, plan_conv, run_conv
    c = cc.CONV_CASES[name]
    w, x, bias, _ = cc.case_data(name)
    L = c["L"]
    lens = [L - 6, L, L - 11]
    x = np.ascontiguousarray(x[:3]) if c["B"] >= 3 else np.concatenate([x, x[:1] * 0.5], 0)
    mk = lambda Bn, Ln, pf=0: conv_case(c["Cout"], c["Cin"], c["K"], c["dil"], c["S"], c["istr"], 0, c["bf"], Bn, Ln, plan_frames=pf)
    batch, _, plan = run_conv(mk(3, L, lens[0]), w, torch.from_numpy(x).cuda(), bias=bias, lens=lens, fill=SENTINEL)
    for b, n in enumerate(lens):
        solo_plan = plan_conv(mk(1, n))
        assert solo_plan.form.key() == plan.form.key() and solo_plan.xw == plan.xw, (form_name(solo_plan.form.key()), form_name(plan.form.key()))
        solo, _, _ = run_conv(mk(1, n), w, torch.from_numpy(np.ascontiguousarray(x[b:b + 1, :, :n])).cuda(), bias=bias)
        on = n * c["S"]
        assert torch.equal(batch[b, :, :on], solo[0]), f"{form_name(plan.form.key())}: row {b}"
        assert bool((batch[b, :, on:] == SENTINEL).all())


# ------------------------------------------------------------------ blocks through run_block, against the float64 oracle
def _oracle(sd):
    from oracle.bicodec_ref import BiCodecDetokRef
    ref = BiCodecDetokRef.__new__(BiCodecDetokRef)
    ref.sd, ref.cfg = sd, None
    return ref


def _block_check(name, y, want, lens, scale, tol):
    y = y.cpu().double()
    err = max(float((y[b, :, :n * scale] - want[b, :, :n * scale]).abs().max()) for b, n in enumerate(lens))
    print(f"BLOCK {name} max abs err {err:.3e} (bar {tol})")
    assert err <= tol, f"{name}: {err}"


def _ragged_oracle(fn, x, lens, scale):
    """a ragged row equals the un-padded run of that row: rows of equal length go through the oracle together"""
    out = None
    for n in sorted(set(lens)):
        rows = [b for b, v in enumerate(lens) if v == n]
        yb = fn(x[rows][:, :, :n])
        if out is None:
            out = torch.zeros(x.shape[0], yb.shape[1], x.shape[2] * scale, dtype=torch.float64)
        out[rows, :, : n * scale] = yb
    return out


@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("name,exact", [("res96_fused", False), ("res96_two", False), ("res96_two", True),
                                        ("res192_fused", False), ("res192_two", False), ("res192_two", True)])
def test_residual_unit_forms(name, exact, dil):
    """k_resunit with three and six waves, and the two-launch unit at the same C in channel-split mode"""
    from oracle.bicodec_ref import precision, snake
    from sparkmi.bicodec import run_block
    kind, kw, Bn, L, _ = cc.BLOCK_CASES[name]
    p, x, _ = cc.block_params(name, dil)
    lens = cc.block_lens(name)
    xt = torch.from_numpy(x)
    xs = snake(xt, torch.from_numpy(p["L.block.0.alpha"]))
    y = run_block(kind, p, xt.cuda(), xs.cuda(), lens=lens, dil=dil, exact_fp32=exact)
    with precision(torch.float64):
        want = _ragged_oracle(lambda v: _oracle(p)._res_unit(v, "L.block", dil), xt.double(), lens, 1)
    _block_check(f"{name} dil {dil} exact {exact}", y, want, lens, 1, TOL_EXACT if exact else TOL_SPLIT)


@pytest.mark.parametrize("name,exact", [("dec_T4", False), ("dec_T5", False), ("dec_chg4", False), ("dec_chg4", True),
                                        ("dec_chg2", False), ("dec_chg2", True)])
def test_decoder_block_forms(name, exact):
    """k_convbT with 4 and 5 phases per block, and the 128- / 64-channel-chunk k_convb forms of a transposed conv"""
    from oracle.bicodec_ref import precision, snake
    from sparkmi.bicodec import run_block
    kind, kw, Bn, L, _ = cc.BLOCK_CASES[name]
    p, x, _ = cc.block_params(name)
    lens = cc.block_lens(name)
    xt = torch.from_numpy(x)
    xs = snake(xt, torch.from_numpy(p["L.block.0.alpha"]))
    y = run_block(kind, p, None, xs.cuda(), lens=lens, K=kw["K"], S=kw["S"], exact_fp32=exact)
    with precision(torch.float64):
        want = _ragged_oracle(lambda v: _oracle(p)._decoder_block(v, "L.block", kw["K"], kw["S"]), xt.double(), lens, kw["S"])
    _block_check(f"{name} exact {exact}", y, want, lens, kw["S"], 2 * TOL_EXACT if exact else TOL_SPLIT)


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("cond_dim", [0, 24])
@pytest.mark.parametrize("name", ["cnx_d100", "cnx_d200", "cnx_d400"])
def test_convnext_forms(name, cond_dim, exact):
    """k_dwln with 4, 12 and 16 channels per thread, LayerNorm and AdaLayerNorm"""
    from oracle.bicodec_ref import precision
    from sparkmi.bicodec import run_block
    kind, kw, Bn, L, _ = cc.BLOCK_CASES[name]
    p, x, cond = cc.block_params(name, cond_dim=cond_dim)
    lens = cc.block_lens(name)
    xt = torch.from_numpy(x)
    y = run_block(kind, p, xt.cuda(), None, None if cond is None else torch.from_numpy(cond).cuda(), lens=lens, exact_fp32=exact)
    with precision(torch.float64):
        rows = []
        for b, n in enumerate(lens):
            cb = None if cond is None else torch.from_numpy(cond[b:b + 1]).double()
            rows.append(torch.nn.functional.pad(_oracle(p)._convnext(xt[b:b + 1, :, :n].double(), "L", cb), (0, L - n)))
        want = torch.cat(rows, 0)
    _block_check(f"{name} cond {cond_dim} exact {exact}", y, want, lens, 1, TOL_EXACT if exact else TOL_SPLIT)
