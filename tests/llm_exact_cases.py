"""What test_llm_exact_ops_gpu.py and test_llm_exact_ops_cpu.py share: the exact-weights mode (``weights_exact = 1``, DESIGN.md
3.10; k_gemm_x in csrc/smi_llm.hip) at the 0.5B widths -- the model, the rows of every case, their inputs, the checks against
float64, a numpy-float32 model of k_gemm_x's arithmetic for each epilogue, and that model with known defects.

The model: ``llm_ctx_cases.model_cfg()`` (three layers of the 0.5B widths, vocab 320) with ``SyntheticLLM(cfg, bf16_exact=False)``:
fp32 matrices that the bf16 arena would round.  One fp32 arena (180 MB, max_positions 1024) serves every engine.

k_gemm_x's arithmetic, as the model restates it (every product and every sum rounded to fp32; the device fuses the two):
  * the operand: g = fl32(gamma * x) for the kernels behind an RMSNorm (PRO_NORM: QKV, gate_up, lm_head), the attention rows or
    the SwiGLU rows for the others -- rebuilt exactly as (hi + mid) + lo from the triples;
  * one chain over k per output, in the 4-wide steps of the fp32 matrix instruction;
  * PRO_NORM: times the row's norm factor.  From k_load_hidden / embed_row_x: ``head_cases.norm_factor32``; from an EPI_RESID
    producer: the ``ssout`` partials, one per four columns ((a^2 + b^2) + (c^2 + d^2)), added by ``smi_ss_lane_sum`` (lane l takes
    partials l, l + 64, ..) and the wave's butterfly (``norm_factor_parts``);
  * EPI_QKV: + bias; RoPE on q and k as four separately rounded products and two rounded sums per pair, with the arena's fp32
    (cos, sin) of the row's POSITION; k / v to the cache, a bf16 cache by round-to-nearest-even;
  * EPI_RESID: h + the chain; EPI_SWIGLU: (gate / (1 + expf(-gate))) * up in fp32.
The attention between QKV and o_proj is not k_gemm_x's (test_llm_long_ctx_gpu.py pins it): the model takes it in float64 over its
own fp32 q / k / v and rounds the result to fp32 once.
"""
import functools

import numpy as np

import head_cases as H
import llm_ctx_cases as X

F = np.float32
MAX_POS = 1024
SLOTS = 64
PAGE = 16
REL = X.REL                      # 1e-5 of each stage's max |value|: the bar of every sibling module (test_llm_ops_full_gpu.REL)
POSITIONS = [0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 460, 690, MAX_POS - 1]
ENGINES = {"f32": ("f32", 0), "bf16": ("bf16", 0), "f32-paged": ("f32", PAGE), "bf16-paged": ("bf16", PAGE)}   # name -> (cache, page)
STAGES = ("q", "k", "v", "attn", "h_mid", "act", "h_out")

# The whole-model bar (test 2b): the relative error (to max |logit|) of ``Model32.forward`` against ``forward_f64`` on
# ``whole_model_ids()``, measured by test_llm_exact_ops_cpu.py::test_whole_model_constant_is_the_measured_one (which fails when the
# two-digit value it measures is not this one).  Never taken from a GPU's output.  The GPU's logits are held to WHOLE_FACTOR times it.
WHOLE_MODEL_ERR = 4.5e-6         # measured 4.506e-06 (max |logit| 6.168)
WHOLE_FACTOR = 4.0               # the matrix instruction's internal order over its 4 k's; the device's expf / sqrtf
WHOLE_IDS = 70                   # 64 + 6: a full chunk and a short one


# ---------------------------------------------------------------------------------------------------------------- the model
def model_cfg():
    return X.model_cfg()


@functools.lru_cache(maxsize=1)
def model_weights():
    """name -> fp32 array of the fp32-saved synthetic checkpoint; asserts that its matrices are NOT bf16-representable (a silently
    rounded arena must not be able to pass)."""
    from sparkmi import weights as W
    cfg = model_cfg()
    syn = W.SyntheticLLM(cfg, bf16_exact=False)
    out = {n: syn[n] for n in syn.names()}
    for n, a in out.items():
        if a.ndim == 2:
            moved = float((H.round_bf16(a) != a).mean())
            assert moved > 0.9, f"{n}: {moved:.2f} of the elements change under bf16 rounding -- the checkpoint must not be bf16-exact"
    return out


def exact_arena(cfg, weights):
    """The fp32 arena on the device, packed once per module."""
    import torch
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    cs = llm_cfg_struct(cfg, 1, MAX_POS, "bf16", True, weights_exact=True)
    return torch.from_numpy(pack_llm_arena(cfg, weights, cs)).to("cuda:0")


def make_engine(cfg, arena, name):
    from sparkmi.llm import SparkLLM
    kv, page = ENGINES[name]
    kw = dict(kv_page_tokens=page, kv_pages=SLOTS * (MAX_POS // page) + 2) if page else {}
    return SparkLLM(cfg, None, "cuda:0", max_slots=SLOTS, max_positions=MAX_POS, arena=arena, kv_dtype=kv, diag=True,
                    weights_exact=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- the cases
DECODE_ROWS = (1, 2, 15, 16, 17, 32, 33, 49, 64)         # every m-tile edge of gy = ceil(M / 16)


def decode_layout(nrows, shuffled):
    """(slot, pos) rows as test_llm_ops_full_gpu._layout: row m in slot m or in a permuted slot, positions cycling through
    POSITIONS."""
    slots = np.random.default_rng(nrows).permutation(SLOTS)[:nrows] if shuffled else np.arange(nrows)
    pos = np.array([POSITIONS[(5 * m + nrows) % len(POSITIONS)] for m in range(nrows)])
    return np.stack([slots, pos], axis=1).astype(np.int32)


def chunk_layout(seqs):
    return np.array([(s, p0 + t) for s, p0, n in seqs for t in range(n)], dtype=np.int32).reshape(-1, 2)


# name -> rows.  The chunks are the shapes the mode's prompt path produces (chunks of at most 64 rows over one or more sequences);
# each chunk's cached context ends exactly at its first position.
CASES = {}
for _n in DECODE_ROWS:
    CASES[f"{_n}"] = decode_layout(_n, False)
    CASES[f"{_n}-perm"] = decode_layout(_n, True)
CASES["chunkA-64"] = chunk_layout([(5, 64, 64)])                       # one slot, positions 64 .. 127
CASES["chunkB-22"] = chunk_layout([(9, 128, 22)])                      # one slot, positions 128 .. 149
CASES["chunkC-40+20"] = chunk_layout([(2, 0, 40), (7, 300, 20)])       # two sequences in one call


def case_seed(name):
    return [23, list(CASES).index(name)]


def case_inputs(cfg, name, layer):
    """(rows, x, kc, vc): residual rows N(0, 1) and, per slot, a cached context of its own below the slot's first row."""
    rows = CASES[name]
    rng = np.random.default_rng(case_seed(name) + [layer])
    x = rng.standard_normal((len(rows), cfg.hidden_size)).astype(F)
    kc, vc = {}, {}
    for s in np.unique(rows[:, 0]):
        n = int(rows[rows[:, 0] == s, 1].min())
        kc[int(s)] = rng.standard_normal((n, cfg.num_key_value_heads, 64)).astype(F)
        vc[int(s)] = rng.standard_normal((n, cfg.num_key_value_heads, 64)).astype(F)
    return rows, x, kc, vc


def layers_under_test(cfg):
    return (0, cfg.num_hidden_layers - 1)


# ---------------------------------------------------------------------------------------------------------------- checks
def close(got, want, what, errs, key, rel=REL):
    scale = float(np.abs(want).max())
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    errs[key] = err / scale
    return err <= rel * scale, f"{what}: max |diff| {err:.3e} against scale {scale:.3f} ({err / scale:.2e}; bar {rel:g})"


def rounded(got, want, what, errs, key):
    """bf16 cache rows: each element within one rounding of the fp64 value, |got - want| <= 2^-8 |want| (+ the fp32 bar)"""
    scale = float(np.abs(want).max())
    diff = np.abs(np.asarray(got, np.float64) - want)
    excess = float((diff - 2.0 ** -8 * np.abs(want)).max())
    errs[key] = float(diff.max()) / scale
    return excess <= REL * scale, f"{what}: an element is {excess:.3e} beyond one bf16 rounding (scale {scale:.3f})"


def stored_cache(rows, kc, vc, k_own, v_own, bf16):
    """slot -> (K, V) of positions 0 .. the slot's last row, as a cache of the given type holds them after stage 0 (what
    ``debug_get_kv`` reads back on the device): the context, then the rows' own K / V at their positions."""
    rnd = H.round_bf16 if bf16 else (lambda a: np.asarray(a, F))
    K, V = {}, {}
    for s in kc:
        own = np.flatnonzero(rows[:, 0] == s)
        n = int(rows[own, 1].max()) + 1
        K[s] = np.zeros((n,) + kc[s].shape[1:], F)
        V[s] = np.zeros_like(K[s])
        K[s][: len(kc[s])], V[s][: len(vc[s])] = rnd(kc[s]), rnd(vc[s])
        K[s][rows[own, 1]], V[s][rows[own, 1]] = rnd(k_own[own]), rnd(v_own[own])
    return K, V


def judge(out, cfg, weights, layer, rows, x, kc, vc, bf16, stored, tag, errs, upto="h_out"):
    """The stage outputs ``out`` (q, k, v, attn, h_mid, act, h_out -- those present) against ``layer_stages_f64`` on the fp32
    weights.  f32 cache: every stage within REL.  bf16 cache: k / v within one bf16 rounding, and the reference attends over the
    cache AS STORED (``stored``: slot -> (K, V) read back after stage 0; ``own_kv=False``), so the later bars measure the kernels
    and not the cache's rounding.  Returns the first failure's message, or None."""
    from oracle.llm_ref import layer_stages_f64
    if bf16:
        ref = layer_stages_f64(cfg, weights, layer, rows, x, stored[0], stored[1], own_kv=False)
    else:
        ref = layer_stages_f64(cfg, weights, layer, rows, x, kc, vc, own_kv=True)
    for name in STAGES:
        if name not in out:
            continue
        if bf16 and name in ("k", "v"):
            ok, msg = rounded(out[name], ref[name], f"{tag}: {name} (bf16 cache row)", errs, name)
        else:
            ok, msg = close(out[name], ref[name], f"{tag}: {name}", errs, name)
        if not ok:
            return msg
        if name == upto:
            break
    return None


# ---------------------------------------------------------------------------------------------------------------- the fp32 model
CORRUPTIONS = ("drop_last_kstep", "weights_bf16", "mc_wide", "neighbour_norm", "rope_row_index", "swiglu_swapped",
               "no_resid_last_tile", "bf16_truncate", "ssout_group_missing")


def truncate_bf16(x):
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(F).reshape(np.shape(x))


def expf32(x):
    """exp of fp32 values rounded to fp32 (through float64: the same bits on every host)."""
    return np.exp(np.asarray(x, np.float64)).astype(F)


def chain(g, Wt, corrupt=None):
    """y[m][n] = sum_k g[m][k] W[n][k] as ONE fp32 chain over k (4 k per matrix instruction, 16 per loop trip of the kernel):
    g (M, K) fp32, Wt = W.T (K, N) fp32.  Each product and each sum is rounded (the device's fused chain rounds once per k)."""
    g = np.ascontiguousarray(g, F)
    K = g.shape[1]
    if corrupt == "drop_last_kstep":
        K -= 16
    if corrupt == "weights_bf16":
        Wt = H.round_bf16(Wt)
    acc = np.zeros((g.shape[0], Wt.shape[1]), F)
    tmp = np.empty_like(acc)
    for k in range(K):
        np.multiply(g[:, k, None], Wt[k][None, :], out=tmp)
        acc += tmp
    return acc


def operand(g, corrupt):
    """The rows a block row reads: ``mc = m < M ? m : M - 1`` clamps only the rows past M; "mc_wide": every row of the second
    m-tile (16 .. 31) takes row M - 1's operand."""
    if corrupt == "mc_wide" and g.shape[0] > 17:
        g = g.copy()
        g[16:32] = g[-1]
    return g


def norm_factor_parts(h, eps=H.EPS, drop_group=None):
    """The RMSNorm factor of rows h (M, N) from the ``ssout`` partials an EPI_RESID epilogue leaves: partial [nt * 4 + g] =
    (a^2 + b^2) + (c^2 + d^2) of columns 16 nt + 4 g .. + 3; lane l adds partials l, l + 64, ..; the wave's butterfly; then
    1 / sqrtf(ss / N + eps).  ``drop_group``: the partials of column group g of every tile are missing."""
    h = np.asarray(h, F)
    M, N = h.shape
    sq = (h * h).reshape(M, N // 4, 4)
    part = ((sq[:, :, 0] + sq[:, :, 1]) + (sq[:, :, 2] + sq[:, :, 3])).astype(F)
    if drop_group is not None:
        part[:, drop_group::4] = 0
    lanes = np.zeros((M, 64), F)
    for i0 in range(0, N // 4, 64):
        seg = part[:, i0:i0 + 64]
        lanes[:, : seg.shape[1]] += seg
    v = lanes
    while v.shape[1] > 1:
        half = v.shape[1] // 2
        v = v[:, :half] + v[:, half:]
    return (F(1.0) / np.sqrt(v[:, 0] / F(N) + F(eps))).astype(F)


def tile_roll(r):
    """every row takes its neighbour's value INSIDE its 16-row m-tile"""
    out = r.copy()
    for m0 in range(0, len(r), 16):
        out[m0:m0 + 16] = np.roll(r[m0:m0 + 16], 1)
    return out


class Model32:
    """The fp32 model of one layer (and of the head) on the fp32 weights; W.T of every matrix is made once."""

    def __init__(self, cfg, weights):
        self.cfg, self.w = cfg, weights
        self._wt = {}
        from sparkmi.arena import rope_table
        self.rope = rope_table(cfg, MAX_POS)                     # (pos, 32, 2) fp32 (cos, sin): the arena's table

    def wt(self, name):
        if name not in self._wt:
            self._wt[name] = np.ascontiguousarray(np.asarray(self.w[name], F).T)
        return self._wt[name]

    def _rope(self, t, idx):
        """t (M, heads, 64) in transformers' order (pairs d, d + 32)"""
        c, s = self.rope[idx, :, 0][:, None, :], self.rope[idx, :, 1][:, None, :]
        a, b = t[..., :32], t[..., 32:]
        return np.concatenate([(a * c) + ((-b) * s), (b * c) + (a * s)], axis=-1).astype(F)

    def layer(self, layer, rows, x, kc, vc, bf16=False, rn_in=None, corrupt=None, upto="h_out"):
        """Stage outputs of ``debug_layer`` for the rows (the dict of ``layer_stages_f64``), plus "rn_out": the next norm's factor
        from down_proj's partials.  ``rn_in``: the input norm's factor (default: as k_load_hidden leaves it)."""
        cfg, p = self.cfg, f"model.layers.{layer}."
        w = lambda n: np.asarray(self.w[p + n], F)  # noqa: E731
        nh, nkv = cfg.num_attention_heads, cfg.num_key_value_heads
        rows = np.asarray(rows, np.int64).reshape(-1, 2)
        x = np.asarray(x, F)
        M = len(rows)
        rn = H.norm_factor32(x) if rn_in is None else rn_in
        if corrupt == "neighbour_norm":
            rn = tile_roll(rn)
        g = operand(w("input_layernorm.weight")[None, :] * x, corrupt)
        qkv = []
        for nm in ("q", "k", "v"):
            y = chain(g, self.wt(p + f"self_attn.{nm}_proj.weight"), corrupt) * rn[:, None]
            qkv.append((y + w(f"self_attn.{nm}_proj.bias")[None, :]).astype(F))
        idx = np.arange(M) if corrupt == "rope_row_index" else rows[:, 1]
        q = self._rope(qkv[0].reshape(M, nh, 64), idx)
        k = self._rope(qkv[1].reshape(M, nkv, 64), idx)
        v = qkv[2].reshape(M, nkv, 64)
        out = {"q": q, "k": k, "v": v}
        if bf16:
            rnd = truncate_bf16 if corrupt == "bf16_truncate" else H.round_bf16
            out["k"], out["v"] = rnd(k), rnd(v)
        if upto in ("q", "k", "v"):
            return out
        K, V = stored_cache(rows, kc, vc, out["k"], out["v"], bf16)
        attn = np.zeros((M, nh * 64), F)
        for i, (s, pos) in enumerate(rows):
            attn[i] = X.attn_f64(q[i], K[int(s)][: pos + 1], V[int(s)][: pos + 1]).astype(F)
        out["attn"] = attn
        o = chain(operand(attn, corrupt), self.wt(p + "self_attn.o_proj.weight"), corrupt)
        h_mid = (x + o).astype(F)
        if corrupt == "no_resid_last_tile":
            m0 = (M - 1) // 16 * 16
            h_mid[m0:] = o[m0:]
        out["h_mid"] = h_mid
        if upto in ("attn", "h_mid"):
            return out
        rn2 = norm_factor_parts(h_mid)
        if corrupt == "neighbour_norm":
            rn2 = tile_roll(rn2)
        g2 = operand(w("post_attention_layernorm.weight")[None, :] * h_mid, corrupt)
        gate = chain(g2, self.wt(p + "mlp.gate_proj.weight"), corrupt) * rn2[:, None]
        up = chain(g2, self.wt(p + "mlp.up_proj.weight"), corrupt) * rn2[:, None]
        if corrupt == "swiglu_swapped":
            gate, up = up, gate
        act = ((gate / (F(1.0) + expf32(-gate))).astype(F) * up).astype(F)
        out["act"] = act
        if upto == "act":
            return out
        d = chain(operand(act, corrupt), self.wt(p + "mlp.down_proj.weight"), corrupt)
        h_out = (h_mid + d).astype(F)
        if corrupt == "no_resid_last_tile":
            m0 = (M - 1) // 16 * 16
            h_out[m0:] = d[m0:]
        out["h_out"] = h_out
        out["rn_out"] = norm_factor_parts(h_out, drop_group=3 if corrupt == "ssout_group_missing" else None)
        return out

    def forward(self, ids, corrupt=None):
        """Teacher-forced logits (S, V) of one sequence at positions 0 .. S - 1 in slot 0 as ``forward_logits`` runs them in this
        mode: chunks of 64 rows; embed_row_x's norm factor into layer 0, every later norm's factor from its producer's ``ssout``
        partials, the lm_head as one more PRO_NORM chain."""
        cfg = self.cfg
        E = np.asarray(self.w["model.embed_tokens.weight"], F)
        ids = np.asarray(ids)
        rows = np.stack([np.zeros(len(ids), np.int64), np.arange(len(ids))], axis=1)
        nkv = cfg.num_key_value_heads
        kc = [np.zeros((0, nkv, 64), F) for _ in range(cfg.num_hidden_layers)]
        vc = [np.zeros((0, nkv, 64), F) for _ in range(cfg.num_hidden_layers)]
        logits = []
        for c0 in range(0, len(ids), 64):
            r = rows[c0:c0 + 64]
            h = E[ids[c0:c0 + 64]]
            rn = H.norm_factor32(h)
            for layer in range(cfg.num_hidden_layers):
                out = self.layer(layer, r, h, {0: kc[layer]}, {0: vc[layer]}, rn_in=rn, corrupt=corrupt)
                kc[layer] = np.concatenate([kc[layer], out["k"]])
                vc[layer] = np.concatenate([vc[layer], out["v"]])
                h, rn = out["h_out"], out["rn_out"]
            g = np.asarray(self.w["model.norm.weight"], F)[None, :] * h
            logits.append(chain(g, self.wt("model.embed_tokens.weight"), corrupt) * rn[:, None])
        return np.concatenate(logits).astype(F)


def whole_model_ids(cfg):
    return np.random.default_rng(37).integers(0, cfg.vocab_size, size=WHOLE_IDS)


def forward_f64(cfg, weights, ids):
    """The float64 forward of one sequence: ``layer_stages_f64`` chained over the layers, then ``head_ref_textbook``."""
    from oracle.llm_ref import layer_stages_f64
    ids = np.asarray(ids)
    rows = np.stack([np.zeros(len(ids), np.int64), np.arange(len(ids))], axis=1)
    h = np.asarray(weights["model.embed_tokens.weight"], np.float64)[ids]
    for layer in range(cfg.num_hidden_layers):
        h = layer_stages_f64(cfg, weights, layer, rows, h, {}, {}, own_kv=True)["h_out"]
    return H.head_ref_textbook(weights["model.embed_tokens.weight"], weights["model.norm.weight"], h)


def whole_model_check(got, want, bar_rel):
    """(ok, relative error, message): every logit within bar_rel of max |logit|, and every row's arg-max the float64 one wherever
    the float64 gap between the two largest logits exceeds twice the bar."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max()) / scale
    if not np.isfinite(got).all() or err > bar_rel:
        return False, err, f"logits at {err:.3e} of max |logit| {scale:.3f} (bar {bar_rel:.3e})"
    top2 = np.sort(want, axis=1)[:, -2:]
    held = (top2[:, 1] - top2[:, 0]) > 2.0 * bar_rel * scale
    bad = np.flatnonzero(held & (got.argmax(1) != want.argmax(1)))
    if len(bad):
        return False, err, f"rows {bad.tolist()}: arg-max differs from the float64 one although its gap exceeds twice the bar"
    return True, err, f"{int(held.sum())} of {len(held)} rows have a clear float64 decision"


# ---------------------------------------------------------------------------------------------------------------- ragged prompts
def ragged_prompts(cfg, n=40):
    """n prompts of 3 .. 90 tokens: some take two chunks of the mode's prompt path; the first 20 are the smaller batch."""
    rng = np.random.default_rng(31)
    lens = rng.integers(3, 91, size=n)
    lens[[1, 7, 25]] = (90, 65, 3)
    return [rng.integers(0, cfg.vocab_size, size=int(k)).tolist() for k in lens]
