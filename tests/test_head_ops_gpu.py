"""The head of a decode step on its own -- the final RMSNorm, the lm_head and the token pick: launch_one(KLM) then launch_one(KFIN)
-- through ``smi_llm_debug_head`` (libsparkmi_diag.so) against the float64 reference of tests/head_cases.py, form by form: the
hook reports the kernel form and grid each case launched, and the case asserts that it is the one it names.

One-layer configs (the layer is never run; its matrices are zero), intermediate_size 32, tied embedding, seeded bf16-exact
weights.  The inputs, the bound, the token rule and the corruptions they reject are shown on the CPU by
tests/test_head_ops_cpu.py."""
import numpy as np
import pytest

import head_cases as H
from sparkmi import config as C

pytestmark = pytest.mark.gpu

NEG_INF_BITS, NO_ID = 0xFF800000, 0x7FFFFFFF


class _Cfg(C.LLMConfig):
    """Hidden sizes that are no multiple of 64 (928 = 29 k tiles, 1056 = 33): the kernels take head_dim 64 and any hidden size
    that is a multiple of 32; LLMConfig derives head_dim from the hidden size, which these tests do not want."""
    head_dim = property(lambda self: 64)


_ENGINES = {}


def _engine(key, hidden, vocab, W, gamma, exact=False, slots=64, env=None):
    """One engine per (weights, mode, switches), kept for the module."""
    if key in _ENGINES:
        return _ENGINES[key]
    import warnings
    from sparkmi.llm import SparkLLM
    cfg = _Cfg(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=1, num_attention_heads=1, num_key_value_heads=1,
               intermediate_size=32, rms_norm_eps=1e-6)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    p = "model.layers.0."
    gamma0 = (1.0 + 0.1 * H.rng_of(f"gamma0/{hidden}").standard_normal(hidden)).astype(np.float32)
    w = {"model.embed_tokens.weight": W, "model.norm.weight": gamma, p + "input_layernorm.weight": gamma0,
         p + "post_attention_layernorm.weight": np.ones(hidden, np.float32),
         p + "self_attn.q_proj.weight": z(64, hidden), p + "self_attn.k_proj.weight": z(64, hidden),
         p + "self_attn.v_proj.weight": z(64, hidden), p + "self_attn.q_proj.bias": z(64), p + "self_attn.k_proj.bias": z(64),
         p + "self_attn.v_proj.bias": z(64), p + "self_attn.o_proj.weight": z(hidden, 64),
         p + "mlp.gate_proj.weight": z(32, hidden), p + "mlp.up_proj.weight": z(32, hidden), p + "mlp.down_proj.weight": z(hidden, 32)}
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (env or {}).items():
            mp.setenv(k, v)                     # the diagnostics build reads its switches when the handle is created
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*bf16-representable.*")   # a weight the bf16 arena would round is a mistake of the case
            llm = SparkLLM(cfg, w, "cuda:0", max_slots=slots, max_positions=8, kv_dtype="bf16", diag=True, weights_exact=exact)
    finally:
        mp.undo()
    _ENGINES[key] = (llm, gamma0)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for llm, _ in _ENGINES.values():
        llm.close()
    _ENGINES.clear()


_REFS = {}


def _group(name):
    """(W, gamma, x, ref, bound) of a shape at its largest row count, computed once: a case of M rows takes the first M."""
    if name not in _REFS:
        hidden, vocab, rows, exact, tag = H.GROUPS[name]
        W, gamma, x = H.make_inputs(hidden, vocab, exact, tag, rows=max(rows))
        ref, A, g, r = H.head_ref(W, gamma, x)
        _REFS[name] = (W, gamma, x, ref, H.head_bound(ref, A, hidden))
    return _REFS[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _check_form(out, want, tag):
    form, grid, block, launches, nblk = want
    got = (out["form"], out["grid"], out["block"], out["launches"], out["nblk"])
    assert got == (form, grid, block, launches, nblk), f"{tag}: launched {got}, the case names {(form, grid, block, launches, nblk)}"


def _check_partials(out, logits, V, tag, allow=None):
    """pval / pidx as the lm_head left them against the logits rows they were taken from."""
    pv, pi = out["pval"], out["pidx"]
    rows = H.masked(logits, allow)
    for m in range(pv.shape[0]):
        idle = _bits(pv[m]) == NEG_INF_BITS
        assert np.array_equal(pi[m][idle], np.full(int(idle.sum()), NO_ID, np.int32)), f"{tag} row {m}: a column at -inf names an id"
        live = pi[m][~idle]
        assert ((live >= 0) & (live < V)).all() and len(set(live.tolist())) == live.size, f"{tag} row {m}: pidx not distinct ids below V"
        assert _same(pv[m][~idle], rows[m][live]), f"{tag} row {m}: pval is not the stored logit at pidx"
        assert pv[m].max() == rows[m].max(), f"{tag} row {m}: max pval {pv[m].max()} is not the row maximum {rows[m].max()}"
        best = pi[m][pv[m] == pv[m].max()].min()
        assert best == H.lowest_argmax(rows[m]), f"{tag} row {m}: the partials' lowest-index maximum {best}, the row's {H.lowest_argmax(rows[m])}"


def _check_next_state(out, W, gamma0, tag):
    """After KFIN: the next step's residual row is the token's embedding row, its first-norm operand triples re-sum to
    fl32(gamma0 * h) exactly, the sums-of-squares partials re-sum to sum h^2 within 8 * 2^-24."""
    tok = out["tokens"]
    assert _same(out["h"], W[tok]), f"{tag}: the next residual rows are not the tokens' embedding rows"
    assert _same(out["g"], (gamma0[None, :] * W[tok]).astype(np.float32)), f"{tag}: the operand triples do not re-sum to fl32(gamma0 * h)"
    want = (H.f64(W[tok]) ** 2).sum(axis=1)
    got = H.f64(out["ss"]).sum(axis=1)
    rel = float((np.abs(got - want) / want).max())
    assert rel <= 8 * H.U, f"{tag}: sum of squares off by {rel / H.U:.2f} x 2^-24"


CASES = [(name, M) for name, g in H.GROUPS.items() for M in g[2]]


@pytest.mark.parametrize("name,M", CASES, ids=[f"{n}-{M}rows" for n, M in CASES])
def test_head_form_by_form(name, M):
    hidden, vocab, rows, exact, tag_ = H.GROUPS[name]
    W, gamma, x, ref, bnd = _group(name)
    llm, gamma0 = _engine(name, hidden, vocab, W, gamma, exact, slots=max(rows))
    tag = f"{name} {M} rows"
    want = H.expected_form(hidden, vocab, M, exact)
    out = llm.debug_head(x[:M], reads=[1] * M)
    _check_form(out, want, tag)
    ok, ratio = H.accept(out["logits_lm"], ref[:M], bnd[:M])
    print(f"HEAD_RATIO {out['form']} {name} rows={M} ratio={ratio:.4f}")
    assert ok, f"{tag}: logits at {ratio:.3f} of the bound"
    _check_partials(out, out["logits_lm"], vocab, tag)
    assert _same(out["logits_fin"], out["logits_lm"]), f"{tag}: KFIN changed the logits of unconstrained rows"
    ok, excluded, msg = H.token_rule(out["tokens"], ref[:M], bnd[:M], stored=out["logits_lm"], sampled=np.ones(M, bool))
    assert ok and excluded == 0.0, f"{tag}: {msg}"
    _check_next_state(out, W, gamma0, tag)
    # the same step with no row reading its logits: the lm_head stores none, the partials and the tokens are the same bits
    dry = llm.debug_head(x[:M])
    _check_form(dry, want, tag + " (no logits)")
    assert _same(dry["pval"], out["pval"]) and np.array_equal(dry["pidx"], out["pidx"]), f"{tag}: the partials depend on the logits store"
    unique = np.array([(out["logits_lm"][m] == out["logits_lm"][m].max()).sum() == 1 for m in range(M)])
    assert np.array_equal(dry["tokens"][unique], out["tokens"][unique]), f"{tag}: the tokens depend on the logits store"
    ok, excluded, msg = H.token_rule(dry["tokens"], ref[:M], bnd[:M], stored=out["logits_lm"])
    assert ok and excluded == 0.0, f"{tag} (no logits): {msg}"
    _check_next_state(dry, W, gamma0, tag + " (no logits)")


@pytest.mark.parametrize("M", [17, 33, 64])
def test_two_group_kernel_gives_the_bits_of_k_lm32(M):
    name = "h256_v1000"
    hidden, vocab, rows, exact, _ = H.GROUPS[name]
    W, gamma, x, ref, bnd = _group(name)
    llm, _ = _engine(name, hidden, vocab, W, gamma)
    two, gamma0 = _engine(name + "/tune2", hidden, vocab, W, gamma, env={"SPARKMI_TUNE2": "8192"})
    a = llm.debug_head(x[:M], reads=[1] * M)
    b = two.debug_head(x[:M], reads=[1] * M)
    _check_form(a, H.expected_form(hidden, vocab, M), f"k_lm32 {M} rows")
    _check_form(b, H.expected_form(hidden, vocab, M, two_group=True), f"k_lm<2> {M} rows")
    ok, ratio = H.accept(b["logits_lm"], ref[:M], bnd[:M])
    print(f"HEAD_RATIO {b['form']} {name} rows={M} ratio={ratio:.4f}")
    assert ok, f"k_lm<2> {M} rows: logits at {ratio:.3f} of the bound"
    for k in ("logits_lm", "pval", "pidx", "tokens", "h"):
        assert _same(a[k], b[k]), f"k_lm<2> {M} rows: {k} differs from k_lm32's"
    _check_partials(b, b["logits_lm"], vocab, f"k_lm<2> {M} rows")
    _check_next_state(b, W, gamma0, f"k_lm<2> {M} rows")


PLANTED = [("h256_v1000", 16), ("h256_v1000", 33), ("h928_v1000", 17), ("h64_v16400", 16), ("h64_v33003", 16), ("h64_v33003", 33),
           ("h1056_v1000", 16), ("h1056_v1000", 17), ("h1056_v1000", 33), ("x64_v1000", 33), ("x32_v262200", 2)]


@pytest.mark.parametrize("name,M", PLANTED, ids=[f"{n}-{M}rows" for n, M in PLANTED])
def test_planted_ties_take_the_lowest_id_and_identical_rows_give_identical_bits(name, M):
    hidden, vocab, rows, exact, tag_ = H.GROUPS[name]
    want = H.expected_form(hidden, vocab, M, exact)
    pairs, solos, neg = H.planted_plan(vocab, want[1][0], want[0], M)
    W, gamma, x, owner, solo_at = H.planted_inputs(hidden, vocab, pairs, exact, tag_, rows=M, solos=solos, negative_row=neg)
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, hidden)
    llm, gamma0 = _engine(f"{name}/planted/{M}", hidden, vocab, W, gamma, exact, slots=max(M, 2))
    tag = f"planted {name} {M} rows"
    out = llm.debug_head(x, reads=[1] * M)
    _check_form(out, want, tag)
    ok, ratio = H.accept(out["logits_lm"], ref, bnd)
    assert ok, f"{tag}: logits at {ratio:.3f} of the bound"
    for nm, (a, b) in pairs.items():
        assert _same(out["logits_lm"][:, a], out["logits_lm"][:, b]), f"{tag}: pair {nm} ({a}, {b}): identical weight rows, different logits bits"
    _check_partials(out, out["logits_lm"], vocab, tag)
    ok, _, msg = H.token_rule(out["tokens"], ref, bnd, stored=out["logits_lm"], sampled=np.ones(M, bool))
    assert ok, f"{tag}: {msg}"
    dry = llm.debug_head(x)                    # greedy rows: k_finalize's own pick
    assert _same(dry["pval"], out["pval"]) and np.array_equal(dry["pidx"], out["pidx"])
    ok, excluded, msg = H.token_rule(dry["tokens"], ref, bnd, stored=out["logits_lm"])
    assert ok and excluded == 0.0, f"{tag}: {msg}"
    names = list(pairs)
    for m, o in enumerate(owner):
        if o >= 0:
            assert dry["tokens"][m] == pairs[names[o]][0], f"{tag}: row {m}, pair {names[o]} {pairs[names[o]]}: token {dry['tokens'][m]}"
    # a maximum that stands ALONE in one partial column: k_finalize must read that column -- 4096 (its loop past the 16 x 256
    # register slots) at V = 262 200, 256 (thread 0's second slot) where the grid has more than 256 blocks, the last one elsewhere
    assert solo_at, f"{tag}: no row carries a solo maximum"
    for m, sid in solo_at.items():
        col = int(np.flatnonzero(out["pidx"][m] == sid)[0])
        assert dry["tokens"][m] == sid and int(np.argmax(out["logits_lm"][m])) == sid, f"{tag}: row {m}: token {dry['tokens'][m]}, the solo maximum is id {sid} (column {col})"
        assert (out["pval"][m] == out["pval"][m].max()).sum() == 1
        if name == "x32_v262200":
            assert col == 4096 and out["nblk"] == 4097
        if sid == 8200:
            assert col == 256 and out["nblk"] > 256
    if (owner == -2).any():
        m = int(np.flatnonzero(owner == -2)[0])
        assert out["logits_lm"][m].max() < 0 and dry["tokens"][m] == H.lowest_argmax(out["logits_lm"][m]) < vocab
    _check_next_state(dry, W, gamma0, tag)


RESTRICTED = [(h, m, "8192" if two else None) for h, m, two in H.RESTRICTED_CASES]


@pytest.mark.parametrize("hidden,M,tune2", RESTRICTED, ids=[f"h{h}-{M}rows" + ("-tune2" if t else "") for h, M, t in RESTRICTED])
def test_restricted_forms(hidden, M, tune2):
    vocab = 1000
    W, gamma, x, allow, tiles = H.restricted_inputs(hidden, vocab, M)
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, hidden)
    llm, gamma0 = _engine(f"restricted/{hidden}/{tune2}", hidden, vocab, W, gamma, env={"SPARKMI_TUNE2": tune2} if tune2 else None)
    tag = f"restricted h{hidden} {M} rows"
    full = llm.debug_head(x, reads=[1] * M)
    _check_form(full, H.expected_form(hidden, vocab, M, two_group=bool(tune2)), tag + " (full)")
    assert int(np.argmax(full["logits_lm"][0])) == 48, "the planted global maximum of row 0 sits one id past its range"
    # poisoned buffer, ONE sampling row, every row constrained: the restricted lm_head stores the union's tiles, masked per row
    reads = [1] + [0] * (M - 1)
    out = llm.debug_head(x, reads=reads, allow=allow, poison=True)
    _check_form(out, H.expected_form(hidden, vocab, M, restricted=True, two_group=bool(tune2)), tag)
    listed = np.zeros(vocab, bool)
    for t in tiles:
        listed[16 * t:16 * t + 16] = True
    want = H.masked(full["logits_lm"], allow)
    lm = out["logits_lm"]
    assert _same(lm[:, listed], want[:, listed]), f"{tag}: a listed tile does not hold the full kernel's logits, masked per row"
    assert np.isnan(lm[:, ~listed]).all(), f"{tag}: the restricted lm_head wrote outside the union's tiles"
    ok, ratio = H.accept(np.where(np.isfinite(want), lm, 0.0), np.where(np.isfinite(want), ref, 0.0), bnd)
    print(f"HEAD_RATIO {out['form']} h{hidden}_v{vocab} rows={M} ratio={ratio:.4f}")
    assert ok, f"{tag}: allowed logits at {ratio:.3f} of the bound"
    # the partials: taken from the masked rows; blocks without a group hold (-inf, no id)
    groups = (len(tiles) + 1) // 2
    assert (_bits(out["pval"][:, groups:]) == NEG_INF_BITS).all() and (out["pidx"][:, groups:] == NO_ID).all(), f"{tag}: idle blocks"
    _check_partials(out, np.where(listed[None, :], lm, -np.inf).astype(np.float32), vocab, tag)
    # after KFIN the sampling row is dense: -inf outside its set, no NaN left
    fin = out["logits_fin"]
    assert _same(fin[0], want[0]) and not np.isnan(fin[0]).any(), f"{tag}: the sampling row is not dense after KFIN"
    ok, excluded, msg = H.token_rule(out["tokens"], ref, bnd, stored=want, allow=allow, sampled=np.array(reads, bool))
    assert ok and excluded == 0.0, f"{tag}: {msg}"
    assert out["tokens"][0] != 48 and 16 <= out["tokens"][0] < 329
    _check_next_state(out, W, gamma0, tag)
    # every row greedy: same partials, the masked arg-max
    dry = llm.debug_head(x, allow=allow)
    assert _same(dry["pval"], out["pval"]) and np.array_equal(dry["pidx"], out["pidx"])
    assert np.array_equal(dry["tokens"], H.pick_tokens(full["logits_lm"], allow)), f"{tag}: the tokens are not the masked arg-max"


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampling"])
@pytest.mark.parametrize("M", [2, 17, 33])
def test_a_nan_row_gives_token_0_and_leaves_its_neighbours_alone(M, sampled):
    name = "h256_v1000"
    hidden, vocab, rows, exact, _ = H.GROUPS[name]
    W, gamma, x, ref, bnd = _group(name)
    llm, gamma0 = _engine(name, hidden, vocab, W, gamma)
    bad = M // 2
    xn = x[:M].copy()
    xn[bad] = np.nan
    reads = [1] * M if sampled else None       # sampling rows: k_sample finds no candidate and emits token 0 as well
    clean = llm.debug_head(x[:M], reads=reads)
    out = llm.debug_head(xn, reads=reads)
    assert out["tokens"][bad] == 0, "a row without a finite logit emits token 0 (k_finalize's guard; k_sample's empty candidate list)"
    keep = np.arange(M) != bad
    for k in ("pval", "pidx", "tokens", "h", "g", "ss"):
        assert _same(out[k][keep], clean[k][keep]), f"NaN row, {M} rows: {k} of the finite rows changed"
    assert (_bits(out["pval"][bad]) == NEG_INF_BITS).all() and (out["pidx"][bad] == NO_ID).all()
    assert _same(out["h"][bad], W[0])


@pytest.mark.parametrize("M", [1, 17])
def test_rows_whose_lo_terms_add_up_stay_inside_the_bound(M):
    """Positive lo terms of almost the largest size (head_cases.lo_inputs): a kernel that lost its lo chain would be at 2.3
    bounds here (shown on the CPU); hidden 32 is one k tile, three of the four waves idle."""
    hidden, vocab = H.LO_HIDDEN, H.LO_VOCAB
    W, gamma, x = H.lo_inputs(hidden, vocab, 17)
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, hidden)
    llm, gamma0 = _engine("lo", hidden, vocab, W, gamma)
    out = llm.debug_head(x[:M], reads=[1] * M)
    _check_form(out, H.expected_form(hidden, vocab, M), f"lo inputs {M} rows")
    ok, ratio = H.accept(out["logits_lm"], ref[:M], bnd[:M])
    print(f"HEAD_RATIO {out['form']}/lo h{hidden}_v{vocab} rows={M} ratio={ratio:.4f}")
    assert ok, f"lo inputs {M} rows: logits at {ratio:.3f} of the bound"
    _check_partials(out, out["logits_lm"], vocab, f"lo inputs {M} rows")


@pytest.mark.parametrize("M", [1, 17])
def test_the_exact_kernels_rebuilt_operand_keeps_its_lo_term(M):
    """The same inputs on an exact-weights engine: k_gemm_x rebuilds x = (hi + mid) + lo in one line that every epilogue shares; at
    hidden 32 a lost lo term stands 2.3 bounds out (shown on the CPU), from K = 128 on it could not be told from rounding."""
    hidden, vocab = H.LO_HIDDEN, H.LO_VOCAB
    W, gamma, x = H.lo_inputs(hidden, vocab, 17)
    ref, A, g, r = H.head_ref(W, gamma, x)
    bnd = H.head_bound(ref, A, hidden)
    llm, gamma0 = _engine("lo/exact", hidden, vocab, W, gamma, exact=True)
    out = llm.debug_head(x[:M], reads=[1] * M)
    _check_form(out, H.expected_form(hidden, vocab, M, exact=True), f"lo inputs, exact weights, {M} rows")
    ok, ratio = H.accept(out["logits_lm"], ref[:M], bnd[:M])
    print(f"HEAD_RATIO {out['form']}/lo h{hidden}_v{vocab} rows={M} ratio={ratio:.4f}")
    assert ok, f"lo inputs, exact weights, {M} rows: logits at {ratio:.3f} of the bound"
    _check_partials(out, out["logits_lm"], vocab, f"lo inputs, exact weights, {M} rows")
