"""What test_llm_long_ctx_gpu.py, test_llm_paged_ops_gpu.py and test_llm_long_ctx_cpu.py share: the three-layer model of the
0.5B widths, the rows of every case, the inputs of a row (a function of layer and position alone, so that one row has the same
residual row and the same cached context in whichever slot, row count or engine it turns up), the cache bookkeeping with the
leak sentinel, the checks against float64, and the attention of one row restated in fp32 in the kernels' summation order and in
float64 with known defects.

The kernels' order (smi_llm.hip: attn_body, attn_merge, k_attn_merge): keys in segments of 1024 (one block each), a segment in
chunks of 256 (bf16 cache) or 128 (f32 cache) keys; inside a chunk wave w, lane group g takes key w * TPW + g of each of four
passes; every wave keeps a running maximum and rescales its sums chunk by chunk; the groups of a wave add up in order, the eight
waves are rescaled to the block's maximum and added in order, the segments to the row's maximum and added in order."""
import contextlib
import os

import numpy as np

SEG = 1024                      # kAttnSeg
MAX_POS = 4096
REL = 1e-5                      # bar of every fp32 stage output, relative to the stage's max |value|
SENTINEL_V = 1.0e4              # leak sentinel: K = 0 (an ordinary score), V = 1e4 (finite; bf16 holds 9984)
LONG_POSITIONS = [1022, 1023, 1024, 1025, 1279, 1280, 2047, 2048, 2049, 3071, 3072, 4094, 4095]


def model_cfg():
    from sparkmi import config as C
    return C.LLMConfig(vocab_size=320, hidden_size=896, num_hidden_layers=3, num_attention_heads=14, num_key_value_heads=2,
                       intermediate_size=4864, rope_theta=1000000.0, rms_norm_eps=1e-6)


def model_weights(cfg):
    """The synthetic weights as a dict (SyntheticLLM builds a tensor on every lookup)."""
    from sparkmi import weights as W
    syn = W.SyntheticLLM(cfg)
    return {n: syn[n] for n in syn.names()}


def device_arena(cfg, weights):
    import torch
    from sparkmi.arena import llm_cfg_struct, pack_llm_arena
    return torch.from_numpy(pack_llm_arena(cfg, weights, llm_cfg_struct(cfg, 1, MAX_POS, "bf16", True))).to("cuda:0")


@contextlib.contextmanager
def env(**kw):
    """SPARKMI_* switches in the environment for the duration (an engine reads them when it is created, debug_layer when it reads
    the fused row back)."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make_engine(cfg, arena, kv, slots, switches=None, **kw):
    from sparkmi.llm import SparkLLM
    with env(**(switches or {})):
        llm = SparkLLM(cfg, None, "cuda:0", max_slots=slots, max_positions=MAX_POS, arena=arena, kv_dtype=kv, diag=True, **kw)
    llm.switches = dict(switches or {})
    return llm


# ---------------------------------------------------------------------------------------------------------------- inputs
def row_x(cfg, layer, pos, salt=0):
    """The residual row entering `layer` for the row at position `pos`."""
    return np.random.default_rng([11, layer, pos, salt]).standard_normal(cfg.hidden_size).astype(np.float32)


def row_ctx(cfg, layer, pos, salt=0):
    """The cached K / V of positions 0 .. pos - 1 behind the row at position `pos`: (pos, kv heads, 64) each, N(0, 1)."""
    rng = np.random.default_rng([13, layer, pos, salt])
    shape = (pos, cfg.num_key_value_heads, 64)
    return rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32)


def decode_inputs(cfg, layer, rows, salts=None):
    """x (M, hidden) and, per slot, the context below the slot's first row (a slot's later rows are the next positions).
    ``salts``: one number per row that sets rows of the same position apart (default: a row's inputs depend on its position alone)."""
    rows = np.asarray(rows, dtype=np.int32).reshape(-1, 2)
    salts = [0] * len(rows) if salts is None else list(salts)
    x = np.stack([row_x(cfg, layer, int(p), salts[m]) for m, (_, p) in enumerate(rows)])
    kc, vc = {}, {}
    for s in np.unique(rows[:, 0]):
        own = np.flatnonzero(rows[:, 0] == s)
        first = own[np.argmin(rows[own, 1])]
        kc[int(s)], vc[int(s)] = row_ctx(cfg, layer, int(rows[first, 1]), salts[first])
    return rows, x, kc, vc


def short_pos(m):
    """Position of short row m: 0 .. 63, all different over 64 rows."""
    return (7 * m + 3) % 64


def layout(n, long_rows, perm=False):
    """n rows, row m in slot m (or in slot perm[m]): position long_rows[m] where given, else a short one."""
    slots = np.random.default_rng(n).permutation(max(n, 9))[:n] if perm else np.arange(n)
    return [(int(slots[m]), int(long_rows.get(m, short_pos(m)))) for m in range(n)]


# name -> rows; in this order a call with 2 segments comes before one with 3 and one with 4 (the partial buffer grows twice)
DECODE_CASES = {f"1row-slot0-{p}": [(0, p)] for p in LONG_POSITIONS}
DECODE_CASES.update({f"1row-slot3-{p}": [(3, p)] for p in (1023, 1024, 2048, 4095)})
DECODE_CASES.update({
    "2rows-short-long": [(0, 17), (1, 1024)],
    "2rows-long-short": [(0, 1025), (1, 40)],
    "9rows": layout(9, {2: 2047, 5: 1279, 7: 3072}),
    "9rows-perm": layout(9, {2: 2047, 5: 1279, 7: 3072}, perm=True),
    # slot 4 holds two consecutive rows on either side of the segment boundary; short rows before, between and after
    "9rows-straddle": [(6, 5), (4, 1023), (4, 1024), (1, 33), (0, 2049), (8, 12), (2, 1280), (7, 61), (3, 0)],
    "17rows": layout(17, {0: 4094, 9: 1280, 16: 2048}),
    "64rows": layout(64, {2: 2047, 31: 1025, 63: 3071}),
    "64rows-last": layout(64, {3: 4095, 40: 1022, 41: 3072}),
})

# prompt pass: name -> ((first position, rows) per sequence, family); sequence b sits in slot PF_SLOTS[b]
PF_GROUPED, PF_PGEMM = 1, 2
PF_SLOTS = [3, 0, 6]
PREFILL_CASES = {
    "0:1025": ([(0, 1025)], PF_PGEMM),
    "1000:70": ([(1000, 70)], PF_PGEMM),
    "2040:65+0:300": ([(2040, 65), (0, 300)], PF_PGEMM),
    "4031:65-cache-end": ([(4031, 65)], PF_PGEMM),
    "1010:40-grouped": ([(1010, 40)], PF_GROUPED),
}


def paged_positions(P):
    """Positions of the paged module's one-row cases: page edges, position 0, one above 1024, the slot's last position."""
    return [0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 1100, MAX_POS - 1]


def prefill_inputs(cfg, layer, plan, seed):
    seqs = [(PF_SLOTS[b], p0, n) for b, (p0, n) in enumerate(plan)]
    rows = np.array([(s, p0 + t) for s, p0, n in seqs for t in range(n)], dtype=np.int32).reshape(-1, 2)
    rng = np.random.default_rng([17, layer, seed])
    x = rng.standard_normal((len(rows), cfg.hidden_size)).astype(np.float32)
    shape = lambda p0: (p0, cfg.num_key_value_heads, 64)  # noqa: E731
    kc = {s: rng.standard_normal(shape(p0)).astype(np.float32) for s, p0, _ in seqs}
    vc = {s: rng.standard_normal(shape(p0)).astype(np.float32) for s, p0, _ in seqs}
    return seqs, rows, x, kc, vc


# ---------------------------------------------------------------------------------------------------------------- the cache
class Cache:
    """One engine's KV cache as the tests leave it.  Every position of a slot above the rows of the case in hand holds the leak
    sentinel (K = 0, V = 1e4), up to ``cap[slot]`` positions (default: the slot's end): ``load`` writes the contexts and renews the
    sentinel where an earlier case's rows or contexts stood.  ``page`` > 0: every write goes page by page, round-robin over the
    slots, so the first writes hand the slots interleaved pages of a paged cache's pool."""

    def __init__(self, llm, page=0, cap=None, sentinel=True):
        self.llm, self.page, self.cap, self.sentinel = llm, page, cap or {}, sentinel
        self.top = {}                      # (layer, slot) -> positions >= top hold the sentinel (absent: nothing written yet)

    def _cap(self, slot):
        return self.cap.get(slot, MAX_POS)

    def _write(self, layer, pieces):
        """pieces: slot -> (pos0, k, v); contiguous: one call each; paged: one page of each slot in turn"""
        if not self.page:
            for s, (p0, k, v) in pieces.items():
                if len(k):
                    self.llm.debug_set_kv(layer, s, k, v, pos0=p0)
            return
        P = self.page
        todo = {s: [p0, p0 + len(k), p0, k, v] for s, (p0, k, v) in pieces.items() if len(k)}
        while todo:
            for s in sorted(todo):
                at, end, p0, k, v = todo[s]
                nxt = min(end, (at // P + 1) * P)
                self.llm.debug_set_kv(layer, s, k[at - p0: nxt - p0], v[at - p0: nxt - p0], pos0=at)
                todo[s][0] = nxt
            todo = {s: t for s, t in todo.items() if t[0] < t[1]}

    def load(self, layer, kc, vc, last):
        """kc / vc: slot -> context from position 0; last: slot -> the position of the slot's last row in the coming call"""
        if self.sentinel:
            tail = {}
            for s, lp in last.items():
                top = self.top.get((layer, s), self._cap(s))
                if (layer, s) not in self.top or lp + 1 < top:
                    n = top - (lp + 1)
                    nkv = next(iter(kc.values())).shape[1]
                    tail[s] = (lp + 1, np.zeros((n, nkv, 64), np.float32), np.full((n, nkv, 64), SENTINEL_V, np.float32))
                self.top[(layer, s)] = lp + 1
            self._write(layer, tail)
        self._write(layer, {s: (0, kc[s], vc[s]) for s in kc})

    def fill(self, layer, slot, pos0, n, k, v):
        """positions pos0 .. pos0 + n - 1 of a slot set to constants (outside the bookkeeping: the caller restores them)"""
        nkv = self.llm.cfg.num_key_value_heads
        self._write(layer, {slot: (pos0, np.full((n, nkv, 64), k, np.float32), np.full((n, nkv, 64), v, np.float32))})

    def sentinel_intact(self, layer, slot, pos0, n):
        """positions pos0 .. pos0 + n - 1 still hold exactly the sentinel (as the cache's type stores it)"""
        if n <= 0:
            return True
        k, v = self.llm.debug_get_kv(layer, slot, pos0, n)
        want = np.float32(SENTINEL_V)
        if self.llm._cs.kv_dtype == 0:
            import torch
            want = torch.tensor(SENTINEL_V).to(torch.bfloat16).float().numpy()
        return bool((k == 0).all() and (v == want).all())


# ---------------------------------------------------------------------------------------------------------------- checks
def close(got, want, what, errs, key, rel=REL):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max())
    errs[key] = err / scale
    print(f"{what}: {err / scale:.3e} of scale")
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} against scale {scale:.3f} ({err / scale:.2e}; bar {rel:g})"


def rounded(got, want, what, errs, key):
    """bf16 cache rows: each element within one rounding of the fp64 value, |got - want| <= 2^-8 |want| (+ the fp32 bar)"""
    scale = float(np.abs(want).max())
    excess = np.abs(got.astype(np.float64) - want) - 2.0 ** -8 * np.abs(want)
    errs[key] = float(np.abs(got.astype(np.float64) - want).max()) / scale
    print(f"{what}: {errs[key]:.3e} of scale (bf16 rows)")
    assert excess.max() <= REL * scale, f"{what}: an element is {excess.max():.3e} beyond one bf16 rounding (scale {scale:.3f})"


def check_qkv(out, ref, f32, tag, errs):
    close(out["q"], ref["q"], f"{tag} stage 0 q", errs, "q")
    for name in ("k", "v"):
        if f32:
            close(out[name], ref[name], f"{tag} stage 0 {name}", errs, name)
        else:
            rounded(out[name], ref[name], f"{tag} stage 0 {name} (bf16 cache row)", errs, name + " (bf16 rows)")


def report(title, measured):
    for key, errs in sorted(measured.items(), key=str):
        print(f"[{title}] {key}: " + ", ".join(f"{s} {e:.2e}" for s, e in errs.items()))
    stages = sorted({s for errs in measured.values() for s in errs if not s.endswith("(bf16 rows)")})
    for s in stages:
        v = [errs[s] for errs in measured.values() if s in errs]
        print(f"[{title}] {s}: {min(v):.2e} .. {max(v):.2e} over {len(v)} outputs")


# ---------------------------------------------------------------------------------------------------------------- one row's attention
def attn_f64(q, K, V, defect=None, page=16, chunk=256):
    """softmax(q K^T / 8) V of one row in float64: q (heads, 64), K / V (T, kv heads, 64) = positions 0 .. T - 1 -> (heads * 64,).
    ``defect``: a known-wrong variant --
      "drop-seg-first"   the first key of the second segment (position 1024) is skipped
      "no-rescale"       the segments' sums are added without bringing them to the common maximum
      "page-off-by-one"  the first key of the row's last page is looked up one page early (position - page)
      "drop-chunk-last"  the last key, when it leaves its chunk partially filled, is skipped"""
    T, nkv, hd = K.shape
    rep = q.shape[0] // nkv
    K = np.repeat(np.asarray(K, np.float64), rep, axis=1)
    V = np.repeat(np.asarray(V, np.float64), rep, axis=1)
    keep = np.ones(T, bool)
    if defect == "drop-seg-first":
        assert T > SEG
        keep[SEG] = False
    if defect == "drop-chunk-last":
        assert T % chunk
        keep[T - 1] = False
    if defect == "page-off-by-one":
        t = (T - 1) // page * page
        assert t >= page
        K, V = K.copy(), V.copy()
        K[t], V[t] = K[t - page], V[t - page]
    sc = np.einsum("hd,thd->ht", np.asarray(q, np.float64), K) * hd ** -0.5
    sc[:, ~keep] = -np.inf
    if defect != "no-rescale":
        pr = np.exp(sc - sc.max(-1, keepdims=True))
        return (np.einsum("ht,thd->hd", pr, V) / pr.sum(-1, keepdims=True)).reshape(-1)
    assert T > SEG
    O, Ls = 0.0, 0.0
    for s0 in range(0, T, SEG):
        pr = np.exp(sc[:, s0: s0 + SEG] - sc[:, s0: s0 + SEG].max(-1, keepdims=True))
        O = O + np.einsum("ht,thd->hd", pr, V[s0: s0 + SEG])
        Ls = Ls + pr.sum(-1, keepdims=True)
    return (O / Ls).reshape(-1)


def attn_f32_restated(q, K, V, f32_cache):
    """The same row in fp32 in the kernels' summation order (the module docstring): every product and sum an fp32 operation, the
    keys of one lane group's stream added strictly one after the other.  q (heads, 64) f32, K / V (T, kv heads, 64) f32."""
    f = np.float32
    T, nkv, hd = K.shape
    nh = q.shape[0]
    rep = nh // nkv
    tpw = 4 if f32_cache else 8               # lane groups per wave; NGRP = 8 * tpw keys per pass, 4 passes per chunk
    ngrp, chunk = 8 * tpw, 32 * tpw
    log2e, neg = f(1.4426950408889634), f(-1e30)
    qv = (q * f(0.125)).astype(f)
    out = np.zeros((nh, hd), f)
    for h in range(nh):
        Kh, Vh = K[:, h // rep].astype(f), V[:, h // rep].astype(f)
        s_all = np.zeros(T, f)
        for d in range(hd):                    # (the lanes' partial dot products meet in a tree; sequential here)
            s_all = (s_all + qv[h, d] * Kh[:, d]).astype(f)
        parts = []
        for s0 in range(0, T, SEG):
            s1 = min(T, s0 + SEG)
            m_run = np.full(8, neg, f)
            lrun = np.zeros((8, tpw), f)
            o = np.zeros((8, tpw, hd), f)
            for c0 in range(s0, s1, chunk):
                t = c0 + np.arange(chunk).reshape(4, 8, tpw)               # [pass][wave][group]
                ok = t < s1
                sc = np.where(ok, s_all[np.minimum(t, s1 - 1)], neg).astype(f)
                mn = np.maximum(m_run, sc.max(axis=(0, 2)))
                a = np.exp2(((m_run - mn) * log2e).astype(f)).astype(f)
                lrun = (lrun * a[:, None]).astype(f)
                o = (o * a[:, None, None]).astype(f)
                for u in range(4):
                    e = np.where(ok[u], np.exp2(((sc[u] - mn[:, None]) * log2e).astype(f)), f(0)).astype(f)
                    lrun = (lrun + e).astype(f)
                    o = (o + e[:, :, None] * Vh[np.minimum(t[u], s1 - 1)]).astype(f)
                m_run = mn
            O, Ls = np.zeros((8, hd), f), np.zeros(8, f)
            for g in range(tpw):                                           # step 1: the groups of a wave, in order
                O, Ls = (O + o[:, g]).astype(f), (Ls + lrun[:, g]).astype(f)
            bm = m_run.max()
            Ob, Lb = np.zeros(hd, f), f(0)
            for w in range(8):                                             # step 2: the waves, rescaled, in order
                scw = np.exp2(f((m_run[w] - bm) * log2e)).astype(f)
                Ob, Lb = (Ob + O[w] * scw).astype(f), f(Lb + Ls[w] * scw)
            parts.append((bm, Lb, Ob))
        if len(parts) == 1:
            out[h] = parts[0][2] / parts[0][1]
            continue
        bm = max(p[0] for p in parts)
        Om, Lm = np.zeros(hd, f), f(0)
        for m_s, l_s, o_s in parts:                                        # k_attn_merge: the segments, rescaled, in order
            scs = np.exp2(f((m_s - bm) * log2e)).astype(f)
            Om, Lm = (Om + o_s * scs).astype(f), f(Lm + l_s * scs)
        out[h] = Om / Lm
    return out.reshape(-1)
