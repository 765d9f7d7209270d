"""Float64 restatements, derived acceptance bounds, seeded inputs and corruptions for the prompt encoder's own kernels
(csrc/smi_enc.hip: k_wavnorm, k_conv0, k_posconv, k_mha, k_tap, k_frames, k_mag, k_rowmean, k_se, k_geglu, k_rmsn, k_vq,
k_fsq_quant, k_copy2d, and k_dwln as the encoder uses it) -- the table behind tests/test_enc_ops_cpu.py (restatement against
the fp32 oracle, every corruption rejected: no GPU) and tests/test_enc_ops_gpu.py (one launch of a real launch list against
the restatement).  DESIGN.md 4.2.1 lists the bounds with the shapes tested and the worst measured ratios.

Conventions.  Every restatement takes the fp32 arrays the launch reads and returns float64.  U = 2^-24 is the unit roundoff
of fp32.  The library is built without fused multiply-adds, so a length-n dot product in fp32 is n rounded products and n
rounded additions of partial sums that never exceed M = sum |a| |b|: |got - ref| <= (n + 8) U M, the form of DESIGN.md 4.0.1
(the 8 covers the bias add and the reduction tree).  An elementwise kernel is held to 8 U of the magnitudes that enter the
element (a device math function good to a few ulp plus the roundings around it).  Data movement is bit-equal.  ``accept``
returns (ok, worst |got - ref| / bound); ``accept_ids`` holds ids to the float64 decision wherever its margin exceeds 1e-4.
"""
import math
import zlib

import numpy as np
import torch

U = 2.0 ** -24
C_ELEM = 8.0            # elementwise kernels: c of the issue; a measured ratio above 1 is a finding, not a reason to raise it
ID_MARGIN = 1e-4
ID_EXCLUDED_MAX = 0.05
GELU_LIP = 1.13         # max |d gelu / dx| = 1.1290 (at x = sqrt(2) * 1.0)


def rng_of(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def accept(got, ref, bnd):
    """Every element finite and within its bound.  (ok, worst ratio)."""
    got, ref, bnd = f64(got), f64(ref), f64(bnd)
    assert got.shape == ref.shape == bnd.shape, (got.shape, ref.shape, bnd.shape)
    if not np.isfinite(got).all():
        return False, float("inf")
    ratio = float((np.abs(got - ref) / np.maximum(bnd, 1e-300)).max()) if got.size else 0.0
    return ratio <= 1.0, ratio


def accept_equal(got, ref):
    """Data movement / selection: the same bits."""
    got = np.ascontiguousarray(got)
    ref = np.ascontiguousarray(ref, dtype=got.dtype)
    return bool(got.shape == ref.shape and np.array_equal(got.view(np.uint32), ref.view(np.uint32)))


def accept_ids(got, ref_ids, margin, planted=None):
    """Ids equal the float64 decision wherever its margin exceeds ID_MARGIN; at most ID_EXCLUDED_MAX of the decisions may be
    excluded that way; ``planted`` (bool mask) decisions -- a value placed exactly on a rounding boundary, whose answer is
    the rounding rule's -- are never excluded.  (k_vq's exact ties need no mask: vq_ref's margin is the gap to the best
    DIFFERENT row, so a duplicated winner is held whenever that gap is clear, and its expected id is the lowest index.)
    (ok, excluded fraction)."""
    got, ref_ids, margin = np.asarray(got).reshape(-1), np.asarray(ref_ids).reshape(-1), f64(margin).reshape(-1)
    assert got.shape == ref_ids.shape == margin.shape
    held = margin > ID_MARGIN
    if planted is not None:
        held = held | np.asarray(planted, dtype=bool).reshape(-1)
    excluded = 1.0 - float(held.mean()) if held.size else 0.0
    ok = excluded <= ID_EXCLUDED_MAX and bool(np.array_equal(got[held], ref_ids[held]))
    return ok, excluded


def gelu64(x):
    x = f64(x)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())


# ------------------------------------------------------------------------------------------ k_wavnorm
def wavnorm_ref(x, eps=1e-7, ddof=0):
    x = f64(x)
    return (x - x.mean()) / np.sqrt(x.var(ddof=ddof) + eps)


def wavnorm_bound(x):
    """The kernel accumulates the mean and the variance in double (error ~1e-16 n: nothing at fp32 scale), then works in fp32:
    fm = (float) mean moves every output by up to U |mean| rstd; rs = 1 / sqrtf((float) var + 1e-7f) carries four roundings
    (the conversion, the add, the root, the division) and (x - fm) * rs two more: 8 U |ref| covers them."""
    x = f64(x)
    rstd = 1.0 / np.sqrt(x.var() + 1e-7)
    return U * abs(x.mean()) * rstd + C_ELEM * U * np.abs(wavnorm_ref(x))


WAVNORM_CASES = {      # name -> (n, mean, spread)
    "n720": (720, 0.0, 0.1), "n1025": (1025, 0.01, 0.2), "n32123": (32123, -0.02, 0.1),
    "dc_offset": (32123, 0.5, 1e-3),            # |mean| / spread = 500: the fp32 mean subtraction term dominates
    "near_constant": (1025, 0.25, 1e-4),        # spread below sqrt(1e-7) = 3.2e-4: eps carries the result
}


def wavnorm_inputs(name):
    n, mean, spread = WAVNORM_CASES[name]
    return (mean + spread * rng_of("wavnorm." + name).standard_normal(n)).astype(np.float32)


def wavnorm_corruptions(name):
    x = wavnorm_inputs(name)
    out = {"sample variance": wavnorm_ref(x, ddof=1)}
    if name == "near_constant":
        out["eps omitted"] = wavnorm_ref(x, eps=0.0)
    return out


# ------------------------------------------------------------------------------------------ k_conv0
def conv0_ref(x, W, b, stride, T):
    """Conv1d(1 -> C, K, stride), no padding: W [C][K], x [n].  (ref [C][T], magnitude |W| (*) |x| + |b|)."""
    x, W, b = f64(x), f64(W), f64(b)
    K = W.shape[1]
    win = np.lib.stride_tricks.sliding_window_view(x, K)[::stride][:T]          # [T][K]
    return W @ win.T + b[:, None], np.abs(W) @ np.abs(win).T + np.abs(b)[:, None]


def conv0_bound(mag, K):
    return (K + 8) * U * mag


# ------------------------------------------------------------------------------------------ k_posconv
def posconv_pre(x, W, b, groups, shift=0, drop_tap=None, drop_ch=None, group_off=0):
    """b[c] + sum_{ci, k} W[c][ci][k] x[g Cg + ci][t + k - K/2 + shift] in float64: x [H][T], W [H][Cg][K].  The keyword
    arguments are the corruptions.  (pre-activation [H][T], magnitude)."""
    x, W, b = f64(x), f64(W).copy(), f64(b)
    H, T = x.shape
    Cg, K = W.shape[1], W.shape[2]
    if drop_tap is not None:
        W[:, :, drop_tap] = 0.0
    if drop_ch is not None:
        W[:, drop_ch, :] = 0.0
    lo = K // 2 - shift
    xp = np.zeros((H, T + 2 * K))
    xp[:, K:K + T] = x
    pre, mag = np.empty((H, T)), np.empty((H, T))
    for g in range(groups):
        gs = (g + group_off) % groups
        win = np.lib.stride_tricks.sliding_window_view(xp[gs * Cg:(gs + 1) * Cg, K - lo:K - lo + T + K - 1], K, axis=1)   # [Cg][T][K]
        Wg = W[g * Cg:(g + 1) * Cg]
        pre[g * Cg:(g + 1) * Cg] = np.einsum("ock,ctk->ot", Wg, win, optimize=True)
        mag[g * Cg:(g + 1) * Cg] = np.einsum("ock,ctk->ot", np.abs(Wg), np.abs(win), optimize=True)
    return pre + b[:, None], mag + np.abs(b)[:, None]


def posconv_ref(x, W, b, groups, **kw):
    pre, mag = posconv_pre(x, W, b, groups, **kw)
    return f64(x) + gelu64(pre), pre, mag


def posconv_bound(x, pre, mag, n):
    """n = Cg K fp32 products and sums: (n + 8) U M on the pre-activation, through GELU by its Lipschitz factor 1.13; erff, the
    GELU's own products and the residual add: 8 U (|x| + |pre|) (|gelu(z)| <= |z|)."""
    return GELU_LIP * (n + 8) * U * mag + C_ELEM * U * (np.abs(f64(x)) + np.abs(pre))


def posconv_corruptions(x, W, b, groups):
    Cg, K = W.shape[1], W.shape[2]
    last = min(K - 1, K // 2 + np.asarray(x).shape[1] - 1)          # the last tap that reaches a frame (T < K / 2: the others read padding)
    return {"window shifted by one frame (K/2 - 1 padding)": posconv_ref(x, W, b, groups, shift=1)[0],
            "last tap dropped": posconv_ref(x, W, b, groups, drop_tap=last)[0],
            "last channel of a group dropped": posconv_ref(x, W, b, groups, drop_ch=Cg - 1)[0],
            "wrong group": posconv_ref(x, W, b, groups, group_off=1)[0]}


# ------------------------------------------------------------------------------------------ k_mha
MHA_SCALE = 0.125
MHA_BOUNDARY_KEYS = (0, 63, 64, 255, 256)     # + Tk - 1


def mha_boundaries(Tk):
    return sorted({j for j in MHA_BOUNDARY_KEYS if j < Tk} | {Tk - 1})


def mha_inputs(name, heads, Tq, Tk):
    """q [heads*64][Tq], k, v [heads*64][Tk] fp32.  Plain normal draws; then, in every head, boundary key j (0, 63, 64, 255,
    256, Tk - 1) is pointed along one query row so that it takes most of that row's softmax mass -- the last valid row for key
    Tk - 1, rows spread over the 8-row blocks for the others -- and its value row is made large, so that a dropped or shifted
    boundary key moves the output far past the bound.  Returns (q, k, v, [(key, row)])."""
    rng = rng_of("mha." + name)
    q = rng.standard_normal((heads * 64, Tq)).astype(np.float32)
    k = rng.standard_normal((heads * 64, Tk)).astype(np.float32)
    v = rng.standard_normal((heads * 64, Tk)).astype(np.float32)
    bnd = mha_boundaries(Tk)
    rows = [Tq - 1 if j == Tk - 1 else (i * max(1, (Tq - 1) // max(1, len(bnd)))) % Tq for i, j in enumerate(bnd)]
    for h in range(heads):
        for i, (j, r) in enumerate(zip(bnd, rows)):
            # (two boundary keys that share a row -- fewer rows than boundaries -- get different scores, hence different masses)
            target = math.log(Tk) + 3.0 + 0.5 * (i % 3)
            qr = f64(q[h * 64:(h + 1) * 64, r])
            k[h * 64:(h + 1) * 64, j] = (qr * (target / (MHA_SCALE * float(qr @ qr)))).astype(np.float32)
            v[h * 64:(h + 1) * 64, j] = (3.0 * np.sign(v[h * 64:(h + 1) * 64, j]) + v[h * 64:(h + 1) * 64, j]).astype(np.float32)
    return q, k, v, list(zip(bnd, rows))


def mha_ref(q, k, v, heads, scale=MHA_SCALE, drop_key=None, shift_last_tile=False):
    """softmax_j(scale q.k) v per head in float64.  Returns (out [heads*64][Tq], probabilities [heads][Tq][Tk], bound)."""
    q, k, v = f64(q), f64(k), f64(v)
    Tq, Tk = q.shape[1], k.shape[1]
    out, probs, bnd = np.empty((heads * 64, Tq)), np.empty((heads, Tq, Tk)), np.empty((heads * 64, Tq))
    for h in range(heads):
        qh, kh, vh = q[h * 64:(h + 1) * 64], k[h * 64:(h + 1) * 64], v[h * 64:(h + 1) * 64]
        s = scale * (qh.T @ kh)                                     # [Tq][Tk]
        if drop_key is not None:
            s[:, drop_key] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        vv = vh
        if shift_last_tile:
            j0 = (Tk - 1) // 64 * 64
            vv = vh.copy()
            vv[:, j0:Tk] = np.roll(vh[:, j0:Tk], 1, axis=1) if Tk - j0 > 1 else vh[:, j0 - 1:Tk - 1]
        out[h * 64:(h + 1) * 64] = vv @ p.T
        probs[h] = p
        # the bound, in the issue's three steps: scores within (64 + 8) U scale sum |q| |k|, delta = the row's largest;
        # probabilities within the relative error 2 delta + (Tk + 8) U; the output within that plus (Tk + 8) U of sum p |v|
        delta = ((64 + 8) * U * abs(scale) * (np.abs(qh).T @ np.abs(kh))).max(axis=1)                # [Tq]
        rel = 2.0 * delta + 2.0 * (Tk + 8) * U
        bnd[h * 64:(h + 1) * 64] = (np.abs(vh) @ p.T) * rel[None, :]
    return out, probs, bnd


def mha_corruptions(q, k, v, heads):
    Tq, Tk = q.shape[1], k.shape[1]
    ref = mha_ref(q, k, v, heads)[0]
    out = {"scale omitted": mha_ref(q, k, v, heads, scale=1.0)[0]}
    if Tk > 1:
        out["last key dropped"] = mha_ref(q, k, v, heads, drop_key=Tk - 1)[0]
        out["last partial V tile shifted by one"] = mha_ref(q, k, v, heads, shift_last_tile=True)[0]
    if Tk > 256:
        out["key 256 dropped"] = mha_ref(q, k, v, heads, drop_key=256)[0]
    if Tq > 1:
        nb = ref.copy()
        nb[:, Tq - 1] = ref[:, Tq - 2]
        out["last query row given its neighbour's output"] = nb
    return out


# ------------------------------------------------------------------------------------------ k_tap
def tap_ref(h, acc, mode):
    h, acc = f64(h), f64(acc)
    return h if mode == 0 else (acc + h if mode == 1 else (acc + h) / 3.0)


def tap_bound(h, acc, mode):
    m = np.abs(f64(h)) + np.abs(f64(acc))
    return C_ELEM * U * (m if mode == 1 else m / 3.0)


def tap_corruptions(h, acc):
    return {"division by 3 applied to one operand (acc + h / 3)": f64(acc) + f64(h) / 3.0}


# ------------------------------------------------------------------------------------------ k_frames / k_mag
def frames_ref(x, n_fft, hop, lo=0, hi=0):
    """F[k][t] = reflect-padded x[t hop + k]; lo / hi: the reflection off by one on either side (corruptions)."""
    x = np.asarray(x)
    n, Tm = len(x), len(x) // hop + 1
    i = np.arange(Tm)[None, :] * hop + np.arange(n_fft)[:, None] - n_fft // 2
    i = np.where(i < 0, -i - lo, i)
    i = np.where(i >= n, 2 * (n - 1) - i + hi, i)
    return x[np.clip(i, 0, n - 1)]


def frames_corruptions(x, n_fft, hop):
    return {"left reflection repeats the edge sample": frames_ref(x, n_fft, hop, lo=1),
            "right reflection repeats the edge sample": frames_ref(x, n_fft, hop, hi=1)}


def mag_ref(D):
    D = f64(D)
    nf = D.shape[0] // 2
    return np.sqrt(D[:nf] ** 2 + D[nf:] ** 2)


def mag_bound(D):
    return C_ELEM * U * mag_ref(D)


def mag_corruptions(D):
    D = f64(D)
    nf = D.shape[0] // 2
    return {"imaginary rows one row early": np.sqrt(D[:nf] ** 2 + D[nf - 1:2 * nf - 1] ** 2)}


# ------------------------------------------------------------------------------------------ k_rowmean / k_se / k_copy2d
def rowmean_ref(X):
    return f64(X).mean(axis=1)


def rowmean_bound(X):
    """a length-T fp32 sum (64 lanes, then the wave reduction) and one division: (T + 8) U mean |x|"""
    X = f64(X)
    return (X.shape[1] + 8) * U * np.abs(X).mean(axis=1)


def rowmean_corruptions(X):
    X = f64(X)
    T = X.shape[1]
    out = {"sum divided by T + 1": X.sum(axis=1) / (T + 1)}
    if T % 64:
        out["last partial trip of 64 ignored"] = X[:, :T // 64 * 64].sum(axis=1) / T
    return out


def se_ref(xin, y, s):
    return f64(xin) + f64(y) * f64(s)[:, None]


def se_bound(xin, y, s):
    return C_ELEM * U * (np.abs(f64(xin)) + np.abs(f64(y) * f64(s)[:, None]))


def se_corruptions(xin, y, s):
    return {"scale of the neighbouring channel": f64(xin) + f64(y) * np.roll(f64(s), 1)[:, None]}


# ------------------------------------------------------------------------------------------ k_geglu / k_rmsn
def geglu_ref(X, inner):
    X = f64(X)
    return gelu64(X[inner:2 * inner]) * X[:inner]


def geglu_bound(X, inner):
    """8 U of the magnitudes entering the element, |gate| |value|: near gate = -3 the factor 1 + erf cancels to 3e-3, so the
    error is relative to the gate, not to the (much smaller) result"""
    X = f64(X)
    return C_ELEM * U * np.abs(X[inner:2 * inner]) * np.abs(X[:inner])


def geglu_corruptions(X, inner):
    X = f64(X)
    return {"gate and value swapped": gelu64(X[:inner]) * X[inner:2 * inner]}


def rmsn_ref(X, gamma, scale=None):
    X, gamma = f64(X), f64(gamma)
    C = X.shape[0]
    nrm = np.maximum(np.sqrt((X * X).sum(axis=0)), 1e-12)
    return X / nrm[None, :] * (math.sqrt(C) if scale is None else scale) * gamma[:, None]


def rmsn_bound(X, gamma):
    """the sum of C squares is within (C + 8) U of itself, its root within half of that; x / nrm * sqrt(C) * gamma adds the
    root, sqrtf(C), one division and two products: ((C + 8) / 2 + 8) U |ref|"""
    C = np.asarray(X).shape[0]
    return ((C + 8) / 2.0 + C_ELEM) * U * np.abs(rmsn_ref(X, gamma))


def rmsn_corruptions(X, gamma):
    return {"sqrt(C) omitted": rmsn_ref(X, gamma, scale=1.0)}


# ------------------------------------------------------------------------------------------ k_dwln as the encoder uses it
def ln_ref(X, w, b, eps, gelu=False, triple=False, ddof=0):
    """LayerNorm over the channels of X [C][T] (+ 3x, + GELU): (out, bound).  Bound: the mean is a length-C fp32 sum,
    e_m = (C + 8) U mean |x|; d = x - mean is off by e_m + U |d|; the variance by (C + 8) U var + 2 e_m mean |d|, so rstd by
    the relative r = half of that over (var + eps), plus 4 U for the division, the add, the root and the reciprocal;
    n = d rstd is then off by e_n = e_m rstd + |n| (r + 2 U); the affine adds 4 U (|n w| + |b|); 3x triples it (y + y + y: two
    more roundings); GELU multiplies by its Lipschitz factor 1.13 and adds 8 U |y|."""
    X, w, b = f64(X), f64(w), f64(b)
    C = X.shape[0]
    mean = X.mean(axis=0)
    d = X - mean[None, :]
    var = (d * d).sum(axis=0) / (C - ddof)
    rstd = 1.0 / np.sqrt(var + eps)
    n = d * rstd[None, :]
    y = n * w[:, None] + b[:, None]
    e_m = (C + 8) * U * np.abs(X).mean(axis=0)
    r = 0.5 * ((C + 8) * U * var + 2.0 * e_m * np.abs(d).mean(axis=0)) / (var + eps) + 4.0 * U
    e_n = e_m[None, :] * rstd[None, :] + np.abs(n) * (r[None, :] + 2.0 * U)
    e_y = np.abs(w)[:, None] * e_n + 4.0 * U * (np.abs(n * w[:, None]) + np.abs(b)[:, None])
    if triple:
        y, e_y = 3.0 * y, 3.0 * e_y + 6.0 * U * np.abs(y)
    if gelu:
        e_y = GELU_LIP * e_y + C_ELEM * U * np.abs(y)
        y = gelu64(y)
    return y, e_y


def ln_corruptions(X, w, b, eps, gelu, triple):
    out = {"sample variance": ln_ref(X, w, b, eps, gelu, triple, ddof=1)[0]}
    if triple:
        out["written once, not 3x"] = ln_ref(X, w, b, eps, gelu, False)[0]
    if gelu:
        y = ln_ref(X, w, b, eps, False, triple)[0]
        out["tanh-approximated GELU"] = 0.5 * y * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))
    return out


# ------------------------------------------------------------------------------------------ k_cbnorm + k_vq
def vq_ref(Ze, codebook, ncode_used=None, tie_high=False):
    """Ze [D][T] fp32, codebook [ncode][D] fp32 (un-normalised, as the arena holds it).  F.normalize both sides, arg-max of
    -(|e|^2 - 2 e.c + |c|^2) in float64, lowest index on exact ties.  margin = the gap to the best code whose ROW differs from
    the winner's (a duplicated row ties exactly in any arithmetic; the decision among the duplicates is the lowest-index rule,
    not a numerical one).  Returns (ids [T], margin [T], tie [T]: the winner's row is duplicated)."""
    Ze, cb = f64(Ze), f64(codebook)
    e = Ze / np.maximum(np.sqrt((Ze * Ze).sum(axis=0)), 1e-12)[None, :]
    cn = cb / np.maximum(np.sqrt((cb * cb).sum(axis=1)), 1e-12)[:, None]
    val = -((e * e).sum(axis=0)[:, None] - 2.0 * (e.T @ cn.T) + (cn * cn).sum(axis=1)[None, :])        # [T][ncode]
    if ncode_used is not None:
        val[:, ncode_used:] = -np.inf
    # group identical rows: first index of each distinct row
    _, first, inv = np.unique(np.asarray(codebook, dtype=np.float32), axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    group = first[inv]                                              # lowest index with the same row
    ids = val.argmax(axis=1)
    if tie_high:
        last = np.zeros_like(group)
        for i, g in enumerate(group):
            last[g] = i
        ids = last[group[ids]]
    else:
        ids = group[ids]
    masked = np.where(group[None, :] == group[ids][:, None], -np.inf, val)
    margin = val[np.arange(val.shape[0]), ids] - masked.max(axis=1)
    counts = np.bincount(group, minlength=len(group))
    return ids.astype(np.int64), margin, counts[group[ids]] > 1


def vq_codebook(name, ncode, D, dup_pairs):
    """normal rows; dup_pairs [(i, j)]: row j is made a copy of row i (an exact tie for every frame)"""
    cb = rng_of("vq.cb." + name).standard_normal((ncode, D)).astype(np.float32)
    for i, j in dup_pairs:
        cb[j] = cb[i]
    return cb


def vq_inputs(name, codebook, T, dup_pairs):
    """Ze [D][T]: normal frames; frame 0 all zero (the max(norm, 1e-12) path); frames 1.. point along the duplicated rows (so
    that the tie decides their id) and along the last rows of the code book (the ragged last trip of 256)."""
    ncode, D = codebook.shape
    Ze = rng_of("vq.ze." + name).standard_normal((D, T)).astype(np.float32)
    Ze[:, 0] = 0.0
    t = 1
    for i, _ in dup_pairs:
        Ze[:, t] = 2.5 * codebook[i]
        t += 1
    for i in (ncode - 1, ncode - 2, ncode - 3):
        if t < T:
            Ze[:, t] = 0.7 * codebook[i]
            t += 1
    return Ze


def vq_corruptions(Ze, codebook):
    ncode = codebook.shape[0]
    out = {"higher index returned on a tie": vq_ref(Ze, codebook, tie_high=True)[0]}
    if ncode % 256:
        out["last ragged trip of codes ignored"] = vq_ref(Ze, codebook, ncode_used=ncode // 256 * 256)[0]
    return out


# ------------------------------------------------------------------------------------------ k_fsq_quant
def fsq_consts(levels):
    lv = np.asarray(levels, dtype=np.int64)
    half_l = (lv - 1) * (1.0 + 1e-3) / 2.0
    offset = np.where(lv % 2 == 0, 0.5, 0.0)
    shift = np.arctanh(offset / half_l)
    return lv, half_l, offset, shift


def fsq_shift_f32(L):
    """the shift an fp32 kernel adds for an even level: atanhf(0.5f / half_l) with half_l = (L - 1) * 1.001f / 2"""
    half_l = np.float32(np.float32(np.float32(L - 1) * np.float32(1.0 + 1e-3)) / np.float32(2.0))
    return np.float32(np.arctanh(np.float32(np.float32(0.5) / half_l), dtype=np.float32))


def fsq_ref(X, W, b, levels, odd_as_even=False, rounding="even", reverse_basis=False, exact_half=None):
    """X [latent][Nt], W [nd][latent], b [nd].  z = W x + b; bounded = tanh(z + shift) half_l - offset; round half to even;
    index = sum (q + L // 2) basis.  ``exact_half`` (bool [Nt][nd]): entries where the fp32 kernel's z + shift is exactly 0, so
    that its bounded value is exactly -offset (the planted -0.5 of an even level).
    Returns (ids [Nt], bounded [Nt][nd], bound on bounded, margin [Nt]: the smallest distance of a digit from x.5)."""
    X, W, b = f64(X), f64(W), f64(b)
    lv, half_l, offset, shift = fsq_consts(levels)
    if odd_as_even:
        offset = np.full_like(offset, 0.5)
        shift = np.arctanh(offset / half_l)
    z = (W @ X).T + b[None, :]                                      # [Nt][nd]
    mag = (np.abs(W) @ np.abs(X)).T + np.abs(b)[None, :]
    arg = z + shift[None, :]
    bd = np.tanh(arg) * half_l[None, :] - offset[None, :]
    if exact_half is not None:
        bd = np.where(exact_half, -offset[None, :], bd)
    # (latent + 8) U M on z and U |z + shift| for the add, through tanh (Lipschitz 1) times half_l; tanhf, the product and the
    # subtraction: 8 U (half_l |tanh| + offset)
    bnd = half_l[None, :] * ((X.shape[0] + 8) * U * mag + U * np.abs(arg)) + C_ELEM * U * (half_l[None, :] * np.abs(np.tanh(arg)) + offset[None, :])
    if rounding == "even":
        q = np.rint(bd)
    else:                                                           # half away from zero (roundf)
        q = np.sign(bd) * np.floor(np.abs(bd) + 0.5)
    basis = np.cumprod(np.concatenate([[1], lv[:-1]]))
    if reverse_basis:
        basis = np.cumprod(np.concatenate([[1], lv[::-1][:-1]]))[::-1]
    ids = ((q + (lv // 2)[None, :]) * basis[None, :]).sum(axis=1).astype(np.int64)
    frac = np.abs(bd - np.floor(bd) - 0.5)
    if exact_half is not None:
        frac = np.where(exact_half, np.inf, frac)                   # planted: held, not excluded
    return ids.astype(np.int32), bd, bnd, frac.min(axis=1)


def fsq_weights(name, levels, latent):
    """project_in: normal rows / sqrt(latent), small bias; dimension 0 of a configuration whose first level is even reads
    x[0] alone (weight row e_0, zero bias), so that a test can place z + shift exactly on 0 there"""
    rng = rng_of("fsq.w." + name)
    nd = len(levels)
    W = (rng.standard_normal((nd, latent)) / math.sqrt(latent)).astype(np.float32)
    b = (0.02 * rng.standard_normal(nd)).astype(np.float32)
    if levels[0] % 2 == 0:
        W[0] = 0.0
        W[0, 0] = 1.0
        b[0] = 0.0
    return W, b


def fsq_inputs(name, levels, latent, Nt):
    """X [latent][Nt] (the perceiver's output: rows of norm sqrt(latent)).  With an even first level, tokens 0..2 carry
    x[0] = -(shift - 1 ulp), -shift, -(shift + 1 ulp): whichever of the three matches the device's atanhf lands z + shift on
    exactly 0, i.e. bounded on exactly -0.5 (tanh(0) = 0 in any implementation) -- the only x.5 that can be planted exactly.
    The two candidates that miss sit one ulp from the boundary: they are probes, not decisions -- the tests leave them out of
    the margin rule (and of its 5 % cap) and hold them, like every token, to the rounding of the kernel's own bounded value.
    Returns (X, candidates: the token indices)."""
    X = rng_of("fsq.x." + name).standard_normal((latent, Nt)).astype(np.float32)
    cand = []
    if levels[0] % 2 == 0 and Nt >= 3:
        s = fsq_shift_f32(levels[0])
        for t, v in enumerate((np.nextafter(s, np.float32(0)), s, np.nextafter(s, np.float32(10)))):
            X[0, t] = -v
            cand.append(t)
    return X, cand


def fsq_corruptions(X, W, b, levels, exact_half=None):
    out = {}
    if list(levels) != list(levels)[::-1]:
        out["basis order reversed"] = fsq_ref(X, W, b, levels, reverse_basis=True, exact_half=exact_half)[0]
    if any(L % 2 for L in levels):
        out["an odd level treated as even"] = fsq_ref(X, W, b, levels, odd_as_even=True, exact_half=exact_half)[0]
    if exact_half is not None and exact_half.any():
        # floor(x + 1/2) agrees with half-to-even at -0.5 (both give 0), so the rounding slip that the one exactly plantable
        # boundary can expose is roundf -- half away from zero -- which gives -1 there
        out["round half away from zero on the planted -0.5"] = fsq_ref(X, W, b, levels, rounding="away", exact_half=exact_half)[0]
    return out


# ------------------------------------------------------------------------------------------ configurations
def samples_for(T):
    """samples that give T wav2vec2 frames (conv kernels 10, 3, 3, 3, 3, 2, 2; strides 5, 2, 2, 2, 2, 2, 2)"""
    return 400 + 320 * (T - 1)


def tiny_cfgs(**tok_kw):
    from sparkmi import config as C, config_tok as T
    import dataclasses
    return T.tiny_wav2vec2(), dataclasses.replace(T.tiny_tok(), **tok_kw), C.tiny_bicodec()


def wide_cfgs():
    """the product's positional-conv group shape (64 channels x 128 taps) and its LayerNorm widths (512, 1024, 384) at two layers"""
    from sparkmi import config as C, config_tok as T
    import dataclasses
    w = T.Wav2Vec2Cfg(conv_dim=[512] * 7, hidden_size=1024, num_attention_heads=16, num_hidden_layers=2, taps=(0, 1, 2),
                      intermediate_size=256, num_conv_pos_embeddings=128, num_conv_pos_embedding_groups=16)
    t = dataclasses.replace(T.tiny_tok(), enc_input_channels=1024, enc_vocos_dim=384)
    return w, t, C.tiny_bicodec()


FSQ_LEVEL_SETS = ([4] * 6, [5, 4, 3, 8, 2], [5, 4, 3, 8, 2, 7, 4, 6], [3])
SPK_TOKEN_NUMS = (5, 8, 70)
VQ_SHAPES = ((256, 8), (300, 5), (300, 16))


def vq_dup_pairs(ncode):
    """(kept row, copy): the same thread's stride (5 and 261: both thread 5 of the 256), different threads (5 and ncode - 1),
    adjacent rows"""
    pairs = [(40, 41), (5, ncode - 1)]
    if ncode > 262:
        pairs.append((5, 261))
    return pairs


# ------------------------------------------------------------------------------------------ the shapes both test modules use
MHA_SELF_T = (2, 9, 65, 257, 1499, 2040)      # 1499 = the default 30 s limit (66,656 B of LDS), 2040 = the kernel's limit (83,968 B)
# cross-attention: (spk_token_num, perceiver_heads, n_ref) -> Tk = Nt + n_ref // 80 + 1: Nt + 3, a value in 65..127, a value > 256
MHA_CROSS = ((5, 2, 200), (8, 3, 200), (70, 2, 200), (5, 3, 7200), (8, 2, 8007), (8, 2, 20800), (70, 3, 16000), (5, 2, 20163))
POSCONV_TINY_T = (2, 64, 65, 1499)
POSCONV_WIDE_T = (65, 130)
ROWMEAN_TM = (3, 64, 65, 201)
REF_HOP, REF_NFFT = 80, 256                    # tiny_tok's mel parameters


def normal(name, shape, scale=1.0, mean=0.0):
    return (mean + scale * rng_of(name).standard_normal(shape)).astype(np.float32)


def mha_lds(Tk):
    return (512 + 8 * Tk + 64 * 65) * 4


def posconv_lds(Cg, K):
    return Cg * (64 + K - 1) * 4
