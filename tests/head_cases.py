"""Float64 restatement, derived acceptance bound, fp32 model, seeded inputs, planted ties and corruptions for the HEAD of a decode
step -- the final RMSNorm, the lm_head and the token pick: launch_one(KLM) then launch_one(KFIN) in csrc/smi_llm.hip (k_lm<1>,
k_lm32<7> / <8>, k_lm<2>, their RT = 1 restricted forms, k_gemm<.., EPI_LM>, k_gemm_x<.., EPI_LM>, k_finalize).  The table behind
tests/test_head_ops_cpu.py (no GPU: the reference against a second float64 statement, the fp32 model inside the bound, every
corruption rejected, no row excluded by the token rule) and tests/test_head_ops_gpu.py (smi_llm_debug_head against the
reference).  DESIGN.md 3.4.1 lists the forms, the bound and the worst measured ratios.

The operation.  x [M][K] are the residual rows leaving the last layer, gamma [K] the final norm's weight, W [V][K] the tied
embedding (bf16-exact; fp32 in the exact-weights mode).  The kernels round g = fl32(gamma * x) ONCE, split it exactly into three
bf16 terms (hi + mid + lo = g), and compute

    logit[m][n] = r[m] * sum_k W[n][k] g[m][k],      r[m] = 1 / sqrt(mean_k x[m][k]^2 + eps)

so the reference takes g in numpy float32 and everything after it in float64.

The bound ((n + 8) U M for a length-n fp32 dot product whose partial sums never exceed M).  With
A[m][n] = r sum_k |W| |g|:

    |got - ref| <= (K + 8) U (1 + 2^-7) A  +  8 U |ref|

  * every product W * (hi | mid | lo) is exact in fp32 (8 x 8 significant bits); the three accumulator chains of a wave add
    K / 4 of them each, the `(lo + mid) + hi` combine, the four-wave add: at most K + 8 rounded additions stand between a product
    and the sum, each rounding a partial sum that the magnitudes bound;
  * the magnitudes of the three chains: |hi| <= (1 + 2^-8) |g|, |mid| <= 2^-8 |g| (1 + 2^-8), |lo| <= 2^-16 |g|: together at
    most (1 + 2^-7) |g|;
  * 8 U |ref| for the norm factor (the sum of squares, the division by K, the add of eps, the root, the reciprocal -- the sum
    of squares is a sum of positive terms, so its relative error is that of its additions and enters r halved) and the final
    multiply by r.
  The exact-weights kernel (one fp32 FMA chain over k on x = hi + mid + lo rebuilt exactly) is inside the same expression.
c = 8 is the project's; a measured ratio above 1 is a finding to explain, not a reason to raise it.

The token rule (``token_rule``).  (1) Wherever the kernel stored its logits row, the token is the lowest-index arg-max of THAT
row (a sampling row with top_k = 1 keeps every id that ties with the maximum, as TopKLogitsWarper does: any of them).  (2) The
token is the float64 arg-max whenever the float64 gap from the maximum to every different-valued id exceeds twice the bound (the
larger of the two elements' bounds); at most 5 % of the rows may fail that premise, and the case seeds are chosen so that none
does (checked on the CPU).
"""
import zlib

import numpy as np

U = 2.0 ** -24
C_SUM = 8.0
C_NORM = 8.0
EPS = float(np.float32(1e-6))   # the config's rms_norm_eps as the kernels hold it
NW = 4                 # waves of an lm_head block: k tile j belongs to wave j % 4
ROW_EXCLUDED_MAX = 0.05
ALL_ROWS = (1, 2, 16, 17, 31, 32, 33, 48, 49, 64)
FEW_ROWS = (1, 17, 33, 64)


def rng_of(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def round_bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return (r.astype(np.uint32) << np.uint32(16)).view(np.float32).reshape(np.shape(x))


# ------------------------------------------------------------------------------------------ shapes
# name -> (hidden, vocab, row counts, exact-weights mode, seed tag).  DESIGN.md 3.4.1 says which form each (shape, rows) reaches.
GROUPS = {
    "h256_v1000": (256, 1000, ALL_ROWS, False, "a"),      # every row count; odd tile count (63), half-filled last tile
    "h256_v61": (256, 61, FEW_ROWS, False, "a"),          # V not a multiple of 4; one block
    "h64_v1000": (64, 1000, FEW_ROWS, False, "a"),        # 2 k tiles: fewer than the four waves
    "h896_v1000": (896, 1000, FEW_ROWS, False, "a"),      # 28 k tiles: UW = 7 full
    "h928_v1000": (928, 1000, FEW_ROWS, False, "a"),      # 29: UW = 8, three waves clamp their last tile
    "h1024_v1000": (1024, 1000, FEW_ROWS, False, "a"),    # 32: UW = 8 full
    "h1056_v1000": (1056, 1000, FEW_ROWS, False, "b"),    # 33: the EPI_LM GEMM
    "h64_v16400": (64, 16400, FEW_ROWS, False, "a"),      # 257 partial columns at <= 16 rows: k_finalize's second register slot
    "h64_v33003": (64, 33003, FEW_ROWS, False, "a"),      # 512 / 256 blocks with 2-3 / 4-5 groups
    "h1024_v33003": (1024, 33003, FEW_ROWS, False, "a"),
    "x64_v1000": (64, 1000, (1, 17, 33, 64), True, "a"),  # exact-weights mode: k_gemm_x, a block row per 16 rows
    "x32_v262200": (32, 262200, (1, 2), True, "a"),       # 4097 partial columns: k_finalize's loop past its 16 register slots
}
MAX_ROWS = 64


def ktiles(hidden):
    return hidden // 32


def lm_cap(vocab):
    return ((vocab + 15) // 16 + 3) // 4


def expected_form(hidden, vocab, rows, exact=False, restricted=False, two_group=False):
    """(kernel form, grid (x, y), block, launches, partial columns) as launch_one(KLM) chooses them -- restated from its
    conditions, for the tests to hold the hook's report against."""
    kt, cap = ktiles(hidden), lm_cap(vocab)
    if exact:
        return "k_gemm_x<EPI_LM>", (cap, (rows + 15) // 16), 256, 1, cap
    if kt > 32:                                     # one launch; beyond 32 rows a second block row of 32
        return ("k_gemm<1,EPI_LM>" if rows <= 16 else "k_gemm<2,EPI_LM>"), (cap, 1 if rows <= 16 else (rows + 31) // 32), 256, 1, cap
    blocks = min(cap, 512)
    rt = ",RT" if restricted else ""
    if rows <= 16:
        return f"k_lm<1{rt}>", (blocks, 1), 256, 1, blocks
    g = min(blocks, 256)
    if two_group:
        return f"k_lm<2{rt}>", (g, 1), 512, (rows + 31) // 32, g
    return f"k_lm32<{7 if kt <= 28 else 8}{rt}>", (g, 1), 256, (rows + 31) // 32, g


# ------------------------------------------------------------------------------------------ inputs
def make_inputs(hidden, vocab, exact=False, tag="a", rows=MAX_ROWS):
    """W [vocab][hidden] (bf16-exact, or any fp32 in the exact-weights mode), gamma [hidden], x [rows][hidden]: rows whose norms
    run from 1e-3 to 1e3 in a shuffled order, so that the first M rows of any case already differ by orders of magnitude and a
    wrong row's norm factor shows."""
    r = rng_of(f"head/{hidden}/{vocab}/{int(exact)}/{tag}")
    W = (0.05 * r.standard_normal((vocab, hidden))).astype(np.float32)
    if not exact:
        W = round_bf16(W)
    gamma = (1.0 + 0.1 * r.standard_normal(hidden)).astype(np.float32)
    ex = np.linspace(-3.0, 3.0, rows)[r.permutation(rows)]
    x = (r.standard_normal((rows, hidden)) * (10.0 ** ex)[:, None]).astype(np.float32)
    return W, gamma, x


# ------------------------------------------------------------------------------------------ reference and bound
def head_ref(W, gamma, x, eps=EPS):
    """(ref [M][V], A [M][V], g [M][K] fp32, r [M]) in float64 from the fp32 arrays the kernels read."""
    g = np.asarray(gamma, np.float32)[None, :] * np.asarray(x, np.float32)          # ONE fp32 rounding, as the kernels'
    r = 1.0 / np.sqrt((f64(x) ** 2).mean(axis=1) + eps)
    ref = r[:, None] * (f64(g) @ f64(W).T)
    A = r[:, None] * (np.abs(f64(g)) @ np.abs(f64(W)).T)
    return ref, A, g, r


def head_ref_textbook(W, gamma, x, eps=EPS):
    """The same head as transformers states it -- Qwen2RMSNorm (weight * (x * rsqrt(mean x^2 + eps))) then the linear layer --
    in float64 throughout: differs from head_ref by the fp32 rounding of gamma * x alone."""
    x = f64(x)
    h = f64(gamma)[None, :] * (x / np.sqrt((x ** 2).mean(axis=1, keepdims=True) + eps))
    return h @ f64(W).T


def head_bound(ref, A, K):
    return (K + C_SUM) * U * (1.0 + 2.0 ** -7) * f64(A) + C_NORM * U * np.abs(f64(ref))


def accept(got, ref, bnd):
    """Every element finite and within its bound.  (ok, worst ratio)."""
    got, ref, bnd = f64(got), f64(ref), f64(bnd)
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    if not np.isfinite(got).all():
        return False, float("inf")
    ratio = float((np.abs(got - ref) / np.maximum(bnd, 1e-300)).max()) if got.size else 0.0
    return ratio <= 1.0, ratio


# ------------------------------------------------------------------------------------------ fp32 model of the kernels' arithmetic
def split3(g):
    """hi + mid + lo == g exactly, each bf16 (csrc/smi_llm.hip: split3)."""
    g = np.asarray(g, np.float32)
    hi = round_bf16(g)
    r1 = (g - hi).astype(np.float32)
    mid = round_bf16(r1)
    lo = round_bf16((r1 - mid).astype(np.float32))
    return hi, mid, lo


def norm_factor32(x, eps=EPS):
    """r in fp32, the sum of squares added lane by lane as k_load_hidden / embed_row do (8 elements per piece, pieces
    lane, lane + 64, ..; then the butterfly over the 64 lanes)."""
    x = np.asarray(x, np.float32)
    M, K = x.shape
    sq = (x * x).astype(np.float32).reshape(M, K // 8, 8)
    lanes = np.zeros((M, 64), np.float32)
    for pc in range(K // 8):
        for e in range(8):
            lanes[:, pc % 64] = (lanes[:, pc % 64] + sq[:, pc, e]).astype(np.float32)
    v = lanes
    while v.shape[1] > 1:
        h = v.shape[1] // 2
        v = (v[:, :h] + v[:, h:]).astype(np.float32)
    ss = v[:, 0]
    return (np.float32(1.0) / np.sqrt((ss / np.float32(K) + np.float32(eps)).astype(np.float32))).astype(np.float32)


CORRUPT_LOGITS = ("drop_last_ktile", "drop_wave", "drop_mid", "neighbour_norm", "no_gamma")   # and "drop_lo", on lo_inputs


def head_model(W, gamma, x, eps=EPS, exact=False, corrupt=None):
    """The kernels' arithmetic in numpy float32: per wave (k tiles j = w, w + 4, ..) three accumulator chains over the hi, mid
    and lo terms, `(lo + mid) + hi`, the in-order add of the four waves, times r.  (A k tile's 32 products are summed by numpy's
    fp32 dot, not in the matrix unit's internal order: a faithful model of the roundings, not of the bits.)  exact: one chain
    over k in the 4-wide steps of the fp32 matrix instruction, on the operand rebuilt as (hi + mid) + lo -- one line shared by every
    epilogue of k_gemm_x ("drop_lo" there: g -> hi + mid).  ``corrupt``: one of CORRUPT_LOGITS."""
    W = np.asarray(W, np.float32)
    x = np.asarray(x, np.float32)
    gam = np.ones_like(gamma, dtype=np.float32) if corrupt == "no_gamma" else np.asarray(gamma, np.float32)
    g = (gam[None, :] * x).astype(np.float32)
    M, K = x.shape
    KT = K // 32
    rn = norm_factor32(x, eps)
    if corrupt == "neighbour_norm":
        rn = np.roll(rn, 1)
    skip = set()
    if corrupt == "drop_last_ktile":
        skip = {KT - 1}
    if corrupt == "drop_wave":
        skip = {j for j in range(KT) if j % NW == (KT - 1) % NW}
    if exact:
        if corrupt == "drop_lo":               # the rebuilt operand x = (hi + mid) + lo without its lo term
            hi, mid, _ = split3(g)
            g = (hi + mid).astype(np.float32)
        acc = np.zeros((M, W.shape[0]), np.float32)
        for k0 in range(0, K, 4):
            if k0 // 32 in skip:
                continue
            acc = (acc + g[:, k0:k0 + 4] @ W[:, k0:k0 + 4].T).astype(np.float32)
        return (acc * rn[:, None]).astype(np.float32)
    parts = split3(g)
    total = None
    for w in range(NW):
        acc = [np.zeros((M, W.shape[0]), np.float32) for _ in range(3)]
        for j in range(w, KT, NW):
            if j in skip:
                continue
            wt = W[:, 32 * j:32 * j + 32].T
            for s in range(3):
                if (corrupt == "drop_mid" and s == 1) or (corrupt == "drop_lo" and s == 2):
                    continue
                acc[s] = (acc[s] + parts[s][:, 32 * j:32 * j + 32] @ wt).astype(np.float32)
        t = ((acc[2] + acc[1]).astype(np.float32) + acc[0]).astype(np.float32)
        total = t if total is None else (total + t).astype(np.float32)
    return (total * rn[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------ token pick
def in_ranges(V, ranges):
    m = np.zeros(V, bool)
    for lo, hi in ranges:
        m[lo:hi] = True
    return m


def masked(logits, allow):
    """The rows with -inf outside each row's ranges (allow[m] None / empty: the row as it is)."""
    out = np.array(logits, np.float32, copy=True)
    if allow is not None:
        for m, ranges in enumerate(allow):
            if ranges:
                out[m, ~in_ranges(out.shape[1], ranges)] = -np.inf
    return out


def lowest_argmax(row):
    row = np.asarray(row)
    if np.isnan(row).any() or not (row > -np.inf).any():
        return 0                                   # k_finalize's guard: no finite maximum -> token 0
    return int(np.flatnonzero(row == row.max())[0])


CORRUPT_PICK = ("ignore_last_vtile", "tail_ids", "tie_high", "mask_after_best")


def pick_tokens(logits, allow=None, corrupt=None):
    """The pick the kernels make on logits rows [M][V] (fp32): lowest-index arg-max of the masked row.  ``corrupt``: one of
    CORRUPT_PICK -- the wrong picks the token rule must reject."""
    logits = np.asarray(logits, np.float32)
    M, V = logits.shape
    rows = logits if corrupt == "mask_after_best" else masked(logits, allow)
    out = np.zeros(M, np.int64)
    for m in range(M):
        row = rows[m]
        if corrupt == "ignore_last_vtile":
            row = row[: (V - 1) // 16 * 16]
        if corrupt == "tail_ids":                  # the zero rows that pad W to a whole tile give logit 0 at ids V .. 16 ceil(V / 16) - 1
            row = np.concatenate([row, np.zeros((-V) % 16, np.float32)])
        if corrupt == "tie_high" and not np.isnan(row).any():
            out[m] = int(np.flatnonzero(row == row.max())[-1])
        else:
            out[m] = lowest_argmax(row)
    return out


def decision(ref, bnd, allow=None):
    """(float64 arg-max id, held) per row: held = the gap from the maximum to every different-valued (allowed) id exceeds
    twice the larger of the two bounds, so every result inside the bound has its maximum there (or at an id of equal float64
    value: a planted duplicate, whose lowest index is the answer)."""
    ref, bnd = f64(ref), f64(bnd)
    M, V = ref.shape
    ids, held = np.zeros(M, np.int64), np.zeros(M, bool)
    for m in range(M):
        ok = in_ranges(V, allow[m]) if allow is not None and allow[m] else np.ones(V, bool)
        r = np.where(ok, ref[m], -np.inf)
        top = int(np.flatnonzero(r == r.max())[0])
        other = ok & (ref[m] != ref[m, top])
        ids[m] = top
        held[m] = bool(np.all(ref[m, top] - ref[m, other] > 2.0 * np.maximum(bnd[m, top], bnd[m, other]))) if other.any() else True
    return ids, held


def token_rule(tokens, ref, bnd, stored=None, allow=None, sampled=None):
    """(ok, excluded fraction, message).  tokens [M]; stored [M][V]: the kernel's own logits rows (None: not stored);
    sampled [M] bool: the row's token is the sampler's (any id that ties with the maximum) instead of k_finalize's."""
    tokens = np.asarray(tokens).reshape(-1)
    M, V = f64(ref).shape
    if ((tokens < 0) | (tokens >= V)).any():
        return False, 0.0, f"token outside [0, {V}): {tokens[(tokens < 0) | (tokens >= V)][:4]}"
    if stored is not None:
        rows = masked(stored, allow)
        for m in range(M):
            if sampled is not None and sampled[m]:
                if not rows[m, tokens[m]] == rows[m].max():
                    return False, 0.0, f"row {m}: sampled token {tokens[m]} is not a maximum of the stored row"
            elif tokens[m] != lowest_argmax(rows[m]):
                return False, 0.0, f"row {m}: token {tokens[m]}, lowest-index arg-max of the stored row {lowest_argmax(rows[m])}"
    ids, held = decision(ref, bnd, allow)
    excluded = 1.0 - float(held.mean())
    if excluded > ROW_EXCLUDED_MAX:
        return False, excluded, f"{excluded:.3f} of the rows have no clear float64 decision"
    for m in np.flatnonzero(held):
        same = f64(ref)[m, tokens[m]] == f64(ref)[m, ids[m]]
        if tokens[m] != ids[m] and not (sampled is not None and sampled[m] and same):
            return False, excluded, f"row {m}: token {tokens[m]}, float64 arg-max {ids[m]}"
    return True, excluded, ""


# ------------------------------------------------------------------------------------------ planted inputs
def tie_pairs(vocab, grid, form):
    """name -> (a, b), a < b: where two ids meet in the reduction.  k_lm / k_lm32: group q = tiles 2q, 2q + 1, block q % grid;
    the GEMM forms: block = tile // 4.  Only the pairs the shape has."""
    nt = (vocab + 15) // 16
    gemm = form.startswith("k_gemm")
    per_block = 4 if gemm else 2                    # tiles a block takes at a time
    first_tile = (lambda blk, trip=0: (blk + trip * grid) * 2) if not gemm else (lambda blk, trip=0: blk * 4)
    p = {}
    if vocab > 48:
        p["same_lane"] = (20, 21)
        p["two_lanes"] = (34, 41)
    if nt >= 8:
        p["tiles_2g_2g1"] = (16 * 6 + 3, 16 * 7 + 3)
    if not gemm and (nt + 1) // 2 > grid + 1:
        p["groups_g_gG"] = (16 * first_tile(1) + 5, 16 * first_tile(1, 1) + 5)
    if grid > 256:
        p["blocks_b_b256"] = (16 * first_tile(0) + 7, 16 * first_tile(256) + 7)
    if grid > 70:
        p["finalize_waves"] = (16 * first_tile(5) + 9, 16 * first_tile(70) + 9)
    p["last_id"] = (min(vocab - 2, 16 * per_block + 1), vocab - 1)
    return {k: (a, b) for k, (a, b) in p.items() if a < b < vocab}


def planted_plan(vocab, grid, form, rows):
    """(pairs, solos, negative_row) for a planted case of `rows` rows.  solos: ids that ALONE hold a row's maximum -- V - 3 (the
    last vocabulary tile; with the lm_cap-block forms at V = 262 200 that is partial column 4096, which only the loop of
    k_finalize past its 16 x 256 register slots reads) and, where a k_lm grid has more than 256 blocks, id 8200 (group 256 =
    column 256: the second register slot of k_finalize's thread 0).  The last rows carry them; at least one row keeps a pair."""
    pairs = tie_pairs(vocab, grid, form)
    solos = [vocab - 3] + ([8200] if not form.startswith("k_gemm") and grid > 256 else [])
    solos = solos[: max(0, rows - 1)]
    return pairs, solos, rows >= len(solos) + 2


def planted_inputs(hidden, vocab, pairs, exact=False, tag="a", rows=MAX_ROWS, solos=(), negative_row=False):
    """(W, gamma, x, owner, solo_at): row m's maximum is planted at pair owner[m] = m % len(pairs) -- both ids of the pair get the
    SAME weight row 0.25 sign(gamma d), d the +-(1 .. 2) direction row m lies along, so both logits are r sum 0.25 |gamma x|
    (about 0.3 K r |x|) against sqrt(K) 0.05-sized logits elsewhere.  solos[i] alone holds the maximum of row rows - 1 - i
    (owner -1; solo_at: row -> id).  negative_row: every weight row gets + 0.125 sign(gamma d) of one more direction and the row
    before the solo rows is -d (owner -2): all its valid logits are negative (the zero rows padding the last tile would win)."""
    r = rng_of(f"head/planted/{hidden}/{vocab}/{int(exact)}/{tag}")
    W, gamma, _ = make_inputs(hidden, vocab, exact, tag, rows)
    W = W.copy()
    names = list(pairs)
    dirs = [(r.choice([-1.0, 1.0], hidden) * r.uniform(1.0, 2.0, hidden)) for _ in range(len(names) + len(solos) + 1)]
    ex = np.linspace(-3.0, 3.0, rows)[r.permutation(rows)]
    x = np.zeros((rows, hidden), np.float32)
    owner = np.zeros(rows, np.int64)
    if negative_row:
        W = round_bf16(W + 0.125 * np.sign(gamma * dirs[-1])[None, :]) if not exact else (W + (0.125 * np.sign(gamma * dirs[-1]))[None, :]).astype(np.float32)
    off = (0.125 * np.sign(gamma * dirs[-1])).astype(np.float32) if negative_row else np.zeros(hidden, np.float32)
    for i, n in enumerate(names):
        a, b = pairs[n]
        W[a] = W[b] = (0.25 * np.sign(gamma * dirs[i])).astype(np.float32) + off      # (+-0.125, +-0.375: bf16-exact)
    solo_at = {}
    for i, sid in enumerate(solos):
        W[sid] = (0.25 * np.sign(gamma * dirs[len(names) + i])).astype(np.float32) + off
        solo_at[rows - 1 - i] = sid
    for m in range(rows):
        owner[m] = m % len(names)
        d = dirs[owner[m]]
        if m in solo_at:
            d, owner[m] = dirs[len(names) + (rows - 1 - m)], -1
        if negative_row and m == rows - 1 - len(solos):
            d, owner[m] = -dirs[-1], -2
        x[m] = (d * (1.0 + 0.01 * r.standard_normal(hidden)) * 10.0 ** ex[m]).astype(np.float32)
    return W, gamma, x, owner, solo_at


def lo_inputs(hidden, vocab, rows):
    """Inputs on which the LO chain shows: gamma = 1, positive bf16-exact weights, and x = (a 2^16 + b 2^8 + c) 2^-23 2^e with
    a in 128 .. 131, b in 64 .. 127, c in 48 .. 63 -- hi = a 2^16, mid = b 2^8 (its 8 significant bits end at 2^7 and c < 64
    rounds down), lo = c exactly: every lo term is positive and close to the largest a lo term can be (2^-17 of g), so the lo
    chain carries about 0.87 * 2^-17 of every logit.  Against (K + 8) U (1 + 2^-7) A + 8 U |ref| that is 2.3 bounds at K = 32 and
    1.4 at K = 64; from K = 128 on the WHOLE lo chain is below the bound, and its loss cannot be told from rounding."""
    r = rng_of(f"head/lo/{hidden}/{vocab}")
    W = round_bf16(np.abs(0.05 * r.standard_normal((vocab, hidden))).astype(np.float32) + np.float32(2.0 ** -10))
    a, b, c = r.integers(128, 132, (rows, hidden)), r.integers(64, 128, (rows, hidden)), r.integers(48, 64, (rows, hidden))
    e = r.integers(-8, 9, rows)
    x = ((a * 65536 + b * 256 + c).astype(np.float64) * 2.0 ** -23 * (2.0 ** e)[:, None]).astype(np.float32)
    return W, np.ones(hidden, np.float32), x


LO_HIDDEN, LO_VOCAB = 32, 1000


def restricted_allow(vocab, rows):
    """Per-row range sets for the restricted forms (vocab >= 1000): rows use different sets, the union has an odd number of
    tiles, one range ends inside a tile, one row's set lies wholly inside another's tile."""
    sets = [
        [(16, 48), (320, 329)],            # tiles 1, 2, 20: the second range ends inside tile 20
        [(322, 326)],                      # wholly inside tile 20 of the first set
        [(0, 5), (640, 672), (995, 1000)],  # tiles 0, 40, 41, 62 (62: the half-filled last tile at vocab 1000)
    ]
    allow = [sets[m % 3] for m in range(rows)]
    tiles = sorted({t for s in allow for lo, hi in s for t in range(lo // 16, (hi - 1) // 16 + 1)})
    return allow, tiles


RESTRICTED_TAGS = {256: "a", 1024: "b"}   # seed tags that give every restricted row a clear float64 decision (checked on the CPU)
RESTRICTED_CASES = [(256, 2, False), (256, 17, False), (256, 33, False), (1024, 17, False), (256, 17, True)]   # (hidden, rows, k_lm<2>)


def restricted_inputs(hidden, vocab, rows):
    """(W, gamma, x, allow, tiles) for the restricted forms: the seeded inputs of the shape, with the global maximum of row 0
    planted at id 48 -- one id past its range [16, 48), inside tile 3, which no row lists."""
    W, gamma, x = make_inputs(hidden, vocab, tag=RESTRICTED_TAGS[hidden])
    W = W.copy()
    W[48] = (0.25 * np.sign(gamma * x[0])).astype(np.float32)
    allow, tiles = restricted_allow(vocab, rows)
    return W, gamma, x[:rows], allow, tiles
