"""The device sampler's draw, restated token by token (csrc/smi_llm.hip: philox_u32, k_sample_scan, k_sample): the counter-based
stream as Python integers, the chain temperature -> top-k with ties -> nucleus -> inverse-CDF pick in float64 with every
threshold comparison widened by ``delta`` (``accepted``), the same chain in numpy float32 in the kernel's own order of operations
(``device_order_f32``), and the cases that tests/test_sample_draws_cpu.py and tests/test_sample_draws_gpu.py share.

The stream.  ``philox_u32(seed, c0, c1)`` is Philox4x32-10 with key = (seed low word, seed high word) and counter =
(c0, c1, 0x5eed5eed, 0), of which output word 0 is used; c0 = the number of tokens the sequence has emitted before this one,
c1 = the sequence's admission number, or 0xFFFFFFFF for a record with a seed of its own (key = that seed).  The draw is
``U = (r >> 8) * 2^-24`` in [0, 1), compared against the CDF over the kept ranks.

The chain.  -inf never survives; the survivors are the finite logits >= the k-th largest (all of them when fewer than top_k are
finite), ordered by (value descending, id ascending), at most the 256 first ranks; p_i = exp((z_i - z_0) * s) / sum with
s = fl32(1 / fl32(T)) (the launch computes ``1.0f / temperature`` from the float the caller passed); rank i >= 1 stays iff
sum_{j >= i} p_j > 1 - fl32(top_p); the pick is the first kept rank whose prefix mass over the kept mass exceeds U, the last kept
rank when none does.  No finite logit: token 0.

``delta`` (``delta_for``): a bound on the distance between the kernel's fp32 and this module's float64 NORMALISED quantities
(suffix mass against 1 - top_p; prefix mass over kept mass against U).  With u = 2^-24 (half an fp32 ulp, relative):
  * exponent argument fl(fl(z_i s) - fl(z_0 s)) against (z_i - z_0) s: two product roundings and one difference,
    <= (|z_i| + |z_0| + |z_i - z_0|) s u <= 4 Z s u = Z s 2^-22 absolute with Z = max |z| over the survivors, which is the
    same relative error of the exponential;
  * expf: no document on this tree states the device library's bound.  ASSUMED: <= EXPF_ULP = 4 ulp, i.e. 4 * 2^-23 relative
    (OpenCL's full profile demands <= 3 ulp of exp and the device library is built to that profile; HIP's published table says 1);
  so every numerator carries a relative error eta <= Z s 2^-22 + 4 * 2^-23;
  * the sum of <= 256 positive numerators is a tree 8 additions deep (two in the lane, six across lanes): <= 8 u relative, and it
    carries eta as well; the division adds u: p_i has relative error <= 2 eta + 9 u;
  * a suffix mass is <= 3 + 6 + 1 = 10 more additions of values <= 1 (<= 10 u absolute), and ``1.0f - top_p`` rounds once (u):
    |suffix_f32 - suffix_f64| <= 2 eta + 20 u;
  * the draw compares fl(fl(U) ksum) with a prefix mass: the prefix (<= 10 additions) has relative error <= eta + 10 u, ksum
    <= eta + 9 u, the product u: on the normalised CDF again <= 2 eta + 20 u.
  delta = 2 (Z s 2^-22 + EXPF_ULP 2^-23) + 20 * 2^-24: 2.6e-6 at Z s = 1, 1.2e-5 at Z s = 20.
Observed (tests/test_sample_draws_cpu.py measures and prints them): the largest |f32 - f64| of a normalised suffix or prefix mass
that ``device_order_f32`` shows over every case of the CPU test is 2.2e-7 (the 166 000-id row at T 0.6, k 256, p 0.999), 3 % of
that case's derived delta 7.7e-6 (numpy's float32 ``exp`` stands where ``expf`` stands, so this is the summation order and the
roundings, not the device library).  The GPU test uses the derived delta.  What the kernels needed of it on an MI355X
(``needed_delta``: the smallest window at which the drawn token is accepted): 0 -- every one of the 5055 draws of the sampler
alone, on both paths, and of the 806 draws inside real steps named the token the float64 chain names at delta = 0.  With delta
0.08 % of the alone draws have more than one accepted token (per case: ties_300_at_kth 0.52 %, big_rows64 0.17 %, tiny 0.10 %,
every other case 0).
"""
import math
import os

import numpy as np

M32 = 0xFFFFFFFF
SEEDED_WORD = 0xFFFFFFFF     # csrc/smi_llm.hip: kSeededStream
SAMPLE_CAP = 256             # kSampleCap: ranks the kernel sorts
EXPF_ULP = 4.0               # assumed bound of the device's expf, in ulp (module docstring)
U24 = 2.0 ** -24


# ------------------------------------------------------------------ the stream
def philox_u32(seed: int, c0: int, c1: int) -> int:
    """csrc/smi_llm.hip's philox_u32, word for word, on Python integers."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    x0, x1, x2, x3 = c0 & M32, c1 & M32, 0x5EED5EED, 0
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x0, 0xCD9E8D57 * x2
        y0, y1 = (p1 >> 32) ^ x1 ^ k0, p1 & M32
        y2, y3 = (p0 >> 32) ^ x3 ^ k1, p0 & M32
        x0, x1, x2, x3 = y0, y1, y2, y3
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return x0


def philox4x32_10(counter, key):
    """The published Philox4x32-10 (Salmon et al., SC'11; Random123's philox.h) written from its definition, not from the
    device function: S-box (hi, lo) = mulhilo(M, x), one permutation per round, key bumped by the Weyl constants BETWEEN rounds.
    The second statement ``philox_u32`` is held to; returns all four output words."""
    ctr, k = [int(c) & M32 for c in counter], [int(x) & M32 for x in key]
    mults, weyl = (0xD2511F53, 0xCD9E8D57), (0x9E3779B9, 0xBB67AE85)

    def mulhilo(a, b):
        p = a * b
        return p >> 32, p & M32

    for rnd in range(10):
        if rnd:
            k = [(k[0] + weyl[0]) & M32, (k[1] + weyl[1]) & M32]
        hi0, lo0 = mulhilo(mults[0], ctr[0])
        hi1, lo1 = mulhilo(mults[1], ctr[2])
        ctr = [hi1 ^ ctr[1] ^ k[0], lo1, hi0 ^ ctr[3] ^ k[1], lo0]
    return ctr


def stream_word(seeded: bool, admission: int) -> int:
    return SEEDED_WORD if seeded else admission & M32


def uniform24(r: int) -> float:
    """U = (r >> 8) * 2^-24: exact in float32 and float64."""
    return (r >> 8) * U24


# ------------------------------------------------------------------ the chain, shared front end
def inv_temp32(T) -> np.float32:
    return np.float32(1.0) / np.float32(T)


def survivors(row: np.ndarray, top_k: int):
    """(ids, values) of the ranks the kernel sorts: finite logits >= the k-th largest, (value desc, id asc), <= 256 of them."""
    row = np.asarray(row, dtype=np.float32)
    fin = np.nonzero(row > -np.inf)[0]
    if len(fin) == 0:
        return fin, row[fin]
    v = row[fin].astype(np.float64)
    k = min(int(top_k), len(fin))
    kth = np.partition(v, len(v) - k)[len(v) - k]
    keep = v >= kth                                 # (-0.0 >= +0.0: both zeros stay, as `scores < kth` removes neither)
    ids, v = fin[keep], v[keep] + 0.0               # (+ 0.0: one zero, so that the sort sees the tie it is)
    order = np.lexsort((ids, -v))[:SAMPLE_CAP]
    return ids[order], row[ids[order]]


def delta_for(row: np.ndarray, T: float, top_k: int) -> float:
    """The derived bound of the module docstring for one row and temperature."""
    _, z = survivors(row, top_k)
    if len(z) == 0:
        return 0.0
    zs = float(np.abs(z.astype(np.float64)).max()) * float(inv_temp32(T))
    return 2.0 * (zs * 2.0 ** -22 + EXPF_ULP * 2.0 ** -23) + 20.0 * U24


def _probs64(z: np.ndarray, T: float) -> np.ndarray:
    z = z.astype(np.float64)
    e = np.exp((z - z[0]) * float(inv_temp32(T)))
    return e / math.fsum(e)


def _suffix64(p: np.ndarray) -> np.ndarray:
    return np.cumsum(p[::-1])[::-1]


def keep_range(p: np.ndarray, top_p: float, delta: float):
    """(fewest, most) ranks the nucleus may keep when its comparison is evaluated at -+delta; rank 0 always stays."""
    thr = 1.0 - float(np.float32(top_p))
    s = _suffix64(p)[1:]
    return 1 + int((s > thr + delta).sum()), 1 + int((s > thr - delta).sum())


def accepted(row, T: float, top_k: int, top_p: float, u: float, delta: float) -> set:
    """Every token the chain may give for the uniform ``u`` = ``uniform24(r)`` when each threshold comparison (nucleus cut,
    inverse-CDF pick) is evaluated at +delta and at -delta: the union of the outcomes."""
    ids, z = survivors(row, top_k)
    if len(ids) == 0:
        return {0}
    p = _probs64(z, T)
    lo, hi = keep_range(p, top_p, delta)
    out = set()
    for keep in range(lo, hi + 1):
        cdf = np.cumsum(p[:keep])
        cdf = cdf / cdf[-1]
        first = int(np.searchsorted(cdf, u - delta, side="right"))       # first rank with cdf > u - delta
        last = int(np.searchsorted(cdf, u + delta, side="right"))        # first rank with cdf > u + delta
        first, last = min(first, keep - 1), min(last, keep - 1)          # no such rank: the last kept one
        out.update(int(t) for t in ids[first: last + 1])
    return out


def needed_delta(row, T: float, top_k: int, top_p: float, u: float, token: int, delta: float) -> float:
    """The smallest window (to 1 / 1024 of ``delta``) at which ``accepted`` holds ``token``, 0.0 when the exact chain names it:
    how far a kernel's draw actually sat from the float64 one.  ``token`` must be accepted at ``delta``."""
    if token in accepted(row, T, top_k, top_p, u, 0.0):
        return 0.0
    lo, hi = 0.0, delta
    for _ in range(10):
        mid = 0.5 * (lo + hi)
        if token in accepted(row, T, top_k, top_p, u, mid):
            hi = mid
        else:
            lo = mid
    return hi


def kept_ids(row, T: float, top_k: int, top_p: float, delta: float):
    """The survivor sets (sorted id arrays) for the fewest and the most ranks the nucleus may keep at -+delta."""
    ids, z = survivors(row, top_k)
    lo, hi = keep_range(_probs64(z, T), top_p, delta)
    return [np.sort(ids[:k]) for k in range(lo, hi + 1)]


# ------------------------------------------------------------------ the kernel's own order, float32
def _tree64(v: np.ndarray) -> np.float32:
    """smi_wave_sum: pairwise over lanes (xor 1, xor 2, half-mirror, mirror inside 16 -- additions commute, so a balanced pairwise
    tree), then (g0 + g1) + (g2 + g3)."""
    v = v.astype(np.float32)
    while len(v) > 1:
        v = v[0::2] + v[1::2]
    return v[0]


VARIANTS = ("no_ties", "keep_minus", "keep_plus", "u_topk_mass", "shift9", "temp_after_cut")


def device_order_f32(row, T: float, top_k: int, top_p: float, r: int, variant=None, probe=None) -> int:
    """k_sample's chain in numpy float32 in the kernel's order (four ranks per lane, wave sum, c / sum suffix sums with the
    shuffle-down tree, prefix tree, u * ksum, backward scan), on the Philox word ``r``; the one token that order gives.
    ``variant``: one of VARIANTS -- a deliberately wrong kernel for the CPU test.  ``probe``: a dict that receives the
    normalised float32 suffix and prefix masses (for measuring their distance from float64)."""
    f32 = np.float32
    row = np.asarray(row, dtype=np.float32)
    ids, z = survivors(row, top_k)
    if len(ids) == 0:
        return 0
    if variant == "no_ties":
        ids, z = ids[: min(top_k, len(ids))], z[: min(top_k, len(ids))]
    k = len(ids)
    s = inv_temp32(T)

    def numerators(scale):
        c = np.zeros(SAMPLE_CAP, dtype=np.float32)
        c[:k] = np.exp((z * scale).astype(np.float32) - f32(z[0] * scale), dtype=np.float32)
        return c.reshape(64, 4)

    c = numerators(f32(1.0) if variant == "temp_after_cut" else s)
    tot = _tree64((c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3]))
    sfx = np.zeros((64, 4), dtype=np.float32)
    sfx[:, 3] = c[:, 3] / tot
    for e in (2, 1, 0):
        sfx[:, e] = c[:, e] / tot + sfx[:, e + 1]
    t = sfx[:, 0].copy()
    d = 1
    while d < 64:
        nxt = t.copy()
        nxt[: 64 - d] = t[: 64 - d] + t[d:]
        t, d = nxt, d * 2
    above = np.append(t[1:], f32(0.0)).astype(np.float32)
    rank = np.arange(SAMPLE_CAP).reshape(64, 4)
    mass = sfx + above[:, None]
    ok = (rank >= 1) & (rank < k) & (mass > f32(1.0) - f32(top_p))
    keep = int(rank[ok].max()) + 1 if ok.any() else 1
    if variant == "keep_minus":
        keep = max(1, keep - 1)
    if variant == "keep_plus":
        keep = min(k, keep + 1)
    if variant == "temp_after_cut":
        c = numerators(s)
        tot = _tree64((c[:, 0] + c[:, 1]) + (c[:, 2] + c[:, 3]))
    ck = np.where(rank < keep, c, f32(0.0)).astype(np.float32)
    pre = np.zeros((64, 4), dtype=np.float32)
    pre[:, 0] = ck[:, 0]
    for e in (1, 2, 3):
        pre[:, e] = pre[:, e - 1] + ck[:, e]
    q = pre[:, 3].copy()
    d = 1
    while d < 64:
        nxt = q.copy()
        nxt[d:] = q[d:] + q[: 64 - d]
        q, d = nxt, d * 2
    ksum = q[63]
    before = np.append(f32(0.0), q[:-1]).astype(np.float32)
    bits = (r >> 9) if variant == "shift9" else (r >> 8)
    u = f32(f32(bits) * f32(U24)) * (tot if variant == "u_topk_mass" else ksum)
    cdf = before[:, None] + pre
    hit = (rank < keep) & (u < cdf)
    pick = int(rank[hit].min()) if hit.any() else keep - 1
    if probe is not None:
        probe["suffix"] = mass.reshape(-1)[:k].astype(np.float64)
        probe["prefix"] = (cdf.reshape(-1)[:keep] / ksum).astype(np.float64)
        probe["keep"] = keep
    return int(ids[pick])


def f32_discrepancy(row, T, top_k, top_p, r) -> float:
    """max |float32 - float64| of the normalised suffix masses and (when both keep the same ranks) prefix masses."""
    probe = {}
    device_order_f32(row, T, top_k, top_p, r, probe=probe)
    if not probe:
        return 0.0
    _, z = survivors(row, top_k)
    p = _probs64(z, T)
    d = float(np.abs(probe["suffix"] - _suffix64(p)).max())
    lo, hi = keep_range(p, top_p, 0.0)
    if probe["keep"] == lo == hi:
        cdf = np.cumsum(p[:lo])
        d = max(d, float(np.abs(probe["prefix"] - cdf / cdf[-1]).max()))
    return d


# ------------------------------------------------------------------ the cases both tests run
ALONE_SEEDS = (1234, (7 << 32) | 5, 0xDEADBEEFCAFE)   # one debug_sample call of n rows per seed: u_m = philox_u32(seed, 0, m)
BIG_V = 166000


def fixture_row(g, name):
    if name != "big":
        return g[f"{name}.logits"]
    seed, v = (int(x) for x in g["big.seed"])
    return (np.random.Generator(np.random.PCG64(seed)).standard_normal(v) * float(g["big.std"])).astype(np.float32)


def _noise(seed, n, lo, hi):
    """n DISTINCT float32 values in [lo, hi), shuffled"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.permutation(np.linspace(lo, hi, n, endpoint=False)).astype(np.float32)


def built_rows():
    """name -> (row, [(T, top_k, top_p)], n_rows): the rows made from seeds.  With a 1000-id vocabulary the lm_head leaves 16
    block maxima, so top_k <= 16 takes the bound path (k_sample_scan) and anything above it the radix path; use_bound = False
    takes the radix path everywhere."""
    out = {}
    base = _noise(11, 1003, -4.0, 4.0)
    out["v1003_scalar_scan"] = (base, [(0.9, 8, 0.9), (1.1, 16, 0.97), (0.8, 40, 0.95)], 64)
    # V % 4 == 0: the float4 loop; 250 float4 over 16 blocks of 16: the last block holds 10, and the top values sit in it
    r = _noise(12, 1000, -4.0, 3.0)
    r[[999, 997, 962, 961, 960, 3]] = [5.0, 4.5, 4.25, 4.0, 3.75, 3.5]
    out["v1000_float4_tail"] = (r, [(1.0, 6, 0.93), (0.7, 12, 0.99)], 16)
    out["all_negative"] = (_noise(13, 1003, -60.0, -50.0), [(1.0, 10, 0.9), (2.0, 50, 0.95)], 64)
    r = np.full(1003, -np.inf, dtype=np.float32)
    r[[5, 17, 400, 401, 999, 1002]] = [1.0, 0.5, 0.25, 0.0, -0.5, -1.0]
    out["six_finite"] = (r, [(1.0, 10, 0.98), (0.8, 50, 1.0)], 16)      # fewer than top_k finite logits
    r = np.full(1003, -np.inf, dtype=np.float32)
    r[777] = -3.0
    out["one_finite"] = (r, [(1.0, 10, 0.9), (1.0, 50, 0.95)], 1)
    # the two zeros tie at the k-th value: 4 positive logits, then +0.0 (id 700) and -0.0 (ids 20, 900); transformers keeps all
    r = _noise(14, 1003, -6.0, -1.0)
    r[[100, 300, 500, 800]] = [2.0, 1.5, 1.0, 0.5]
    r[700] = 0.0
    r[[20, 900]] = -0.0
    out["zeros_tie_at_kth"] = (r, [(1.0, 5, 1.0), (1.0, 6, 0.995), (1.0, 20, 1.0)], 64)
    # 300 ids tie at the k-th value: the 256 first ranks in (value, id) order are what the kernel promises (include/sparkmi.h)
    r = _noise(15, 1003, -8.0, -2.0)
    r[np.arange(300) * 3 + 50] = 1.0
    r[[0, 1, 2, 1001, 1002, 6, 7]] = [3.0, 2.5, 2.25, 2.0, 1.75, 1.5, 1.25]
    out["ties_300_at_kth"] = (r, [(1.0, 8, 1.0), (1.5, 60, 0.999)], 64)
    # more than 1024 ids at or above the bound, a clean top-16 above them: 16 values at ids 0 .. 15, 2984 ids in [1, 2) behind
    # them (fewer than 16 of the 512 / 256 blocks), the rest in [0, 0.1): the 16th largest block maximum is a low one
    r = _noise(16, BIG_V, 0.0, 0.1)
    r[16:3000] = _noise(17, 2984, 1.0, 2.0)
    r[:16] = np.linspace(6.0, 4.5, 16, dtype=np.float32)
    out["bound_overflow"] = (r, [(1.0, 16, 0.98)], 64)
    return out


def alone_cases(golden_dir, big=True):
    """[(name, row, params, n_rows)] for the sampler alone: the fixture rows at all their parameter sets and ``built_rows``.
    n_rows 1 / 16 / 64: with the 166 000-id rows the lm_head leaves 512 maxima at <= 16 rows and 256 above."""
    g = np.load(os.path.join(golden_dir, "sampling.npz"))
    cases = []
    for name, n_rows in (("tiny", 64), ("tie", 16), ("edge", 64), ("big", 0)):
        if name == "big" and not big:
            continue
        params = [(float(t), int(k), float(p)) for t, k, p in g[f"{name}.params"]]
        if name == "big":
            row = fixture_row(g, name)
            for n in (1, 16, 64):
                cases.append((f"big_rows{n}", row, params, n))
        else:
            cases.append((name, fixture_row(g, name), params, n_rows))
    for name, (row, params, n_rows) in built_rows().items():
        if len(row) == BIG_V and not big:
            continue
        cases.append((name, row, params, n_rows))
    return cases


ALONE_NAMES = ("tiny", "tie", "edge", "big_rows1", "big_rows16", "big_rows64", "v1003_scalar_scan", "v1000_float4_tail",
               "all_negative", "six_finite", "one_finite", "zeros_tie_at_kth", "ties_300_at_kth", "bound_overflow")


def alone_draws(n_rows):
    """[(seed, row m, r)] of a case's debug_sample calls: key = seed, token index 0, admission number m."""
    return [(seed, m, philox_u32(seed, 0, m)) for seed in ALONE_SEEDS for m in range(n_rows)]


# ------------------------------------------------------------------ the in-step cases (counter words)
STEP_HANDLE = dict(do_sample=True, temperature=0.9, top_k=40, top_p=0.95, seed=(3 << 32) | 77)
STEP_RECORDS = (
    {"do_sample": False},                                                                        # greedy under a sampling handle
    None,                                                                                        # inherit
    {"do_sample": True, "temperature": 1.0, "top_k": 60, "top_p": 0.9},                          # own T / k / p, the handle's stream
    {"do_sample": True, "temperature": 0.7, "top_k": 12, "top_p": 0.97, "seed": (9 << 32) | 1001},   # seeded
    {"do_sample": True, "temperature": 1.2, "top_k": 30, "top_p": 0.9, "repetition_penalty": 1.3,
     "presence_penalty": 0.4},                                                                   # penalised: k_penalize's logits
)
STEP_LIVE = (1, 5, 33)
STEP_STEPS = 12
STEP_FIRST_ADMISSION = 1     # one throwaway sequence is admitted and retired first, so that admission number != slot


def step_record(j, n_live):
    """Row j's record in an admission of ``n_live`` rows: the kinds in turn; a one-row session runs the seeded record."""
    return STEP_RECORDS[3] if n_live == 1 else STEP_RECORDS[j % len(STEP_RECORDS)]


def step_selection(rec):
    """(samples, T, top_k, top_p, key, seeded) a record resolves to under STEP_HANDLE (csrc/smi_llm.hip: row_sel)."""
    h = STEP_HANDLE
    if rec is None or "do_sample" not in rec:
        return True, h["temperature"], h["top_k"], h["top_p"], h["seed"], False
    if not rec["do_sample"]:
        return False, 1.0, 1, 1.0, h["seed"], False
    seeded = rec.get("seed") is not None
    return True, rec["temperature"], rec["top_k"], rec["top_p"], rec["seed"] if seeded else h["seed"], seeded


def step_word(rec, token_index, admission, variant=None) -> int:
    """The Philox word of a sampling row's draw in a step; ``variant``: 'swapped' / 'seeded_on_admission' -- wrong streams."""
    _, _, _, _, key, seeded = step_selection(rec)
    c1 = stream_word(seeded and variant != "seeded_on_admission", admission)
    return philox_u32(key, c1, token_index) if variant == "swapped" else philox_u32(key, token_index, c1)
