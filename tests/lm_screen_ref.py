"""A numpy model of the one-row greedy lm_head's int8 screen (csrc/smi_llm.hip: k_lm_pack8, k_lm_screen, k_lm_select; DESIGN.md
3.4.3) and the inputs its tests share.

The copy, per vocabulary row v:  s_v = max_k |w_vk| / 127,  q_vk = rint(w_vk / s_v) (int8),  Q_v = sum_k |q_vk|.
The operand (g = fl32(gamma * x), what the kernels' triples re-sum to):  a = max|g| / 127,  X1 = rint(g / a),  b = a / 254,
X2 = rint((g - a X1) / b), so g = a X1 + b X2 + r with |r_k| <= b / 2.
The screen:  S_v = s_v (a A1 + b A2) with A1 = sum q X1, A2 = sum q X2 exact integers, and

    |S_v - sum_k w_vk g_k|  <=  (s_v / 2) |g|_1  +  (s_v Q_v) b / 2      [+ slack_v = 2^-12 (s_v Q_v) max|g| for fp32 rounding]

because w = s q + e with |e| <= s / 2 and g = a X1 + b X2 + r.  A tile of 16 rows is listed when max (S_v + B_v) over its ids
reaches the largest S_v - B_v of all ids.  The RMSNorm factor is a positive factor common to the row and is left out.

The arithmetic is fp32 where the kernels' is; the sum |g|_1 is taken in float64 and rounded once (the kernels add it in another
order: covered by the slack)."""
import numpy as np

import head_cases as H

f32 = np.float32
TILE = 16


def pack8(W):
    """(s [V] f32, q [V][K] int32 in -127 .. 127, sQ [V] f32) of a bf16-exact W [V][K]."""
    W = np.asarray(W, f32)
    s = (np.abs(W).max(axis=1) / f32(127.0)).astype(f32)
    safe = np.where(s > 0, s, f32(1.0)).astype(f32)
    q = np.where(s[:, None] > 0, np.rint((W / safe[:, None]).astype(f32)), 0.0)
    q = np.clip(q, -127, 127).astype(np.int32)
    sq = (s * np.abs(q).sum(axis=1).astype(f32)).astype(f32)
    return s, q, sq


def operand(g):
    """The quantised operand of one row g [K] f32: dict(a, b, X1, X2, l1, mx, all) -- `all`: every tile is a candidate."""
    g = np.asarray(g, f32)
    mx = f32(np.abs(g).max()) if np.isfinite(g).all() else f32(np.nan)
    a = f32(mx / f32(127.0))
    b = f32(a / f32(254.0))
    if not (np.isfinite(g).all() and b > 0):
        z = np.zeros(g.shape, np.int32)
        return dict(a=a, b=b, X1=z, X2=z, l1=f32(0), mx=mx, all=True)
    X1 = np.clip(np.rint((g / a).astype(f32)), -127, 127)
    resid = (H.f64(g) - H.f64(a) * X1).astype(f32)          # fmaf(-a, X1, g): one rounding
    X2 = np.clip(np.rint((resid / b).astype(f32)), -127, 127)
    return dict(a=a, b=b, X1=X1.astype(np.int32), X2=X2.astype(np.int32), l1=f32(np.abs(H.f64(g)).sum()), mx=mx, all=False)


def screen(s, q, sq, op):
    """(S [V], B [V], slack [V]) in fp32 as k_lm_screen computes them; B includes the slack."""
    A1 = (q.astype(np.int64) @ op["X1"].astype(np.int64)).astype(f32)
    A2 = (q.astype(np.int64) @ op["X2"].astype(np.int64)).astype(f32)
    a, b = op["a"], op["b"]
    S = (s * ((a * A1).astype(f32) + (b * A2).astype(f32)).astype(f32)).astype(f32)
    hl1, hb, sl = f32(0.5) * op["l1"], f32(0.5) * b, f32(op["mx"] * f32(2.0 ** -12))
    slack = (sq * sl).astype(f32)
    B = (((s * hl1).astype(f32) + (sq * hb).astype(f32)).astype(f32) + slack).astype(f32)
    return S, B, slack


def n_tiles(V):
    return (V + TILE - 1) // TILE


def select(S, B, V, everything=False):
    """The ascending tile list: tiles whose largest S + B reaches the largest S - B."""
    nt = n_tiles(V)
    if everything:
        return np.arange(nt)
    up = np.full(nt * TILE, -np.inf, f32)
    up[:V] = (S + B).astype(f32)[:V]
    thr = (S - B).astype(f32)[:V].max()
    ub = up.reshape(nt, TILE).max(axis=1)
    return np.flatnonzero(~(ub < thr))


def model_list(W, g):
    """The tile list of row g against W, with (S, B, slack) for the checks."""
    s, q, sq = pack8(W)
    op = operand(g)
    S, B, slack = screen(s, q, sq, op)
    return select(S, B, W.shape[0], everything=op["all"]), S, B, slack


def tiles_of(ids):
    return np.unique(np.asarray(ids) // TILE)


def possible_winner_tiles(W, gamma, x):
    """Tiles holding a row that attains the float64 maximum within head_cases.head_bound: ref_v + bnd_v >= max_u (ref_u - bnd_u)."""
    ref, A, g, r = H.head_ref(W, gamma, x[None, :])
    bnd = H.head_bound(ref, A, W.shape[1])
    return tiles_of(np.flatnonzero(ref[0] + bnd[0] >= (ref[0] - bnd[0]).max()))


# ------------------------------------------------------------------------------------------ inputs
def gaussian(hidden, vocab, tag="a"):
    """(W bf16-exact [vocab][hidden], gamma [hidden]) of a shape."""
    r = H.rng_of(f"lm_screen/{hidden}/{vocab}/{tag}")
    W = H.round_bf16((0.05 * r.standard_normal((vocab, hidden))).astype(f32))
    gamma = (1.0 + 0.1 * r.standard_normal(hidden)).astype(f32)
    return W, gamma


def gaussian_rows(hidden, vocab, W, gamma, n, limit=0.10, tag="a"):
    """n seeded Gaussian rows x [n][hidden] (norms from 1e-2 to 1e2), each CHOSEN so that the model alone lists at most `limit` of
    the tiles: candidates are drawn in order and the first n that do are kept."""
    r = H.rng_of(f"lm_screen/rows/{hidden}/{vocab}/{tag}")
    s, q, sq = pack8(W)
    rows, drawn = [], 0
    while len(rows) < n:
        drawn += 1
        assert drawn <= 8 * n, f"hidden {hidden} vocab {vocab}: fewer than {n} of {drawn} Gaussian rows keep the list below {limit:.0%}"
        x = (r.standard_normal(hidden) * 10.0 ** r.uniform(-2.0, 2.0)).astype(f32)
        op = operand((gamma * x).astype(f32))
        S, B, _ = screen(s, q, sq, op)
        if len(select(S, B, vocab)) <= limit * n_tiles(vocab):
            rows.append(x)
    return np.stack(rows)


def cases():
    """name -> (W, gamma, x [hidden]) of the CPU cases; `identical` lists every tile by construction."""
    out = {}
    for name, hidden, vocab in (("gaussian", 256, 1008), ("v_not_multiple_of_16", 256, 1003), ("hidden928", 928, 1003), ("hidden1056", 1056, 1003)):
        W, gamma = gaussian(hidden, vocab)
        out[name] = (W, gamma, gaussian_rows(hidden, vocab, W, gamma, 1, limit=1.0)[0])
    W, gamma = gaussian(256, 1003, "o")
    r = H.rng_of("lm_screen/outlier")
    x = r.standard_normal(256).astype(f32)
    x[r.choice(256, 4, replace=False)] *= f32(20.0)          # four outlier channels
    out["outlier_channels"] = (W, gamma, x)
    W2 = W.copy()
    W2[517] = H.round_bf16((W2[517] * f32(64.0)).astype(f32))   # one huge row
    out["huge_row"] = (W2, gamma, r.standard_normal(256).astype(f32))
    W3 = W.copy()
    W3[40] = 0.0                                             # a zero row: s = 0, q = 0
    out["zero_row"] = (W3, gamma, r.standard_normal(256).astype(f32))
    W4 = np.repeat(W[:1], 1003, axis=0)                      # all rows identical: every tile ties
    out["identical"] = (W4, gamma, r.standard_normal(256).astype(f32))
    return out
