"""The paged KV cache (``kv_page_tokens`` > 0) under every kernel form that reads or appends through ``kv_row()`` with a page table,
stage by stage: against float64, and bit for bit against a contiguous engine of the same model loaded with the same K / V and
given the same rows -- DESIGN.md's claim that contiguous and paged caches take the same code, checked where it could be false.

Model: three layers of the 0.5B widths, 4096 positions per slot (llm_ctx_cases).  Page sizes 16 and 64, f32 and bf16 cache.
Scrambled table: when an engine is built, every slot's positions are written through ``debug_set_kv`` one page at a time,
round-robin over the slots, so a slot's pages interleave with its neighbours' and no two of them are consecutive
(``debug_page_table``; slots 0 and 1 are equally long so that neither is ever alone in the round).

Forms (named in every assertion message): one row in slot 0 at positions 0, P-1, P, P+1, 2P-1, 2P -- the fused ``k_attn<KV,1,1,1>``
(stage 1 is inside the kernel: stages 0, 2, 3, 4) and, with SPARKMI_NO_FUSE_O=1, ``k_attn<KV,1,0,1>``; 2, 8, 17 and 64 identity rows --
``k_attn<KV,2,0,1>``; 8 permuted rows -- the general ``k_attn<KV,0>``; one row at 1100 and at the slot's last position 4095, and 8 rows
with two long ones -- the general kernel with segments + ``k_attn_merge``, reading through pages; 2 and 8 rows with
SPARKMI_FUSE2_ROWS=8 -- the diagnostics-only ``k_attn<KV,2,2,1>``; the prompt pass (``k_attn_pf<f32>``, ``k_attn_pf2``, ``k_attn_pf<bf16>``
with SPARKMI_ATTN_PF2=0, and the KV-append epilogue of ``k_pgemm``) on 70 + 65 + 96 rows and on 38 rows from 651 beside 300.

Assertions: (a) the float64 bars of test_llm_long_ctx_gpu.py (1e-5 of each stage's max |value|; bf16 K / V rows within one
rounding); (b) every stage output, the appended K / V rows read back by ``debug_get_kv`` included, equals the contiguous engine's
bit for bit; (c) every position above a slot's last row -- the unused tail of its last page and the pages behind it -- and every
page of an idle slot holds K = 0 / V = 1e4 in both engines: a leaked key would break (a), and after stage 0 the pages still hold
exactly the sentinel, so the append wrote its own (page, offset) only.
Measured on MI355X over every (page size, engine, case, layer): attention 0 (one key) .. 1.7e-6, q 9.5e-8 .. 7.0e-7, f32 K / V rows
8.1e-8 .. 7.4e-7, o_proj + residual 4.9e-8 .. 6.1e-7, SwiGLU 1.3e-7 .. 1.5e-6, down_proj + residual 1.9e-7 .. 1.3e-6; bf16 K / V rows
1.2e-3 .. 3.7e-3 of the rows' scale.  Printed per stage and at teardown (pytest -s), with each engine's first table rows."""
import numpy as np
import pytest

import llm_ctx_cases as X

pytestmark = pytest.mark.gpu

MEASURED = {}
CAPS = {0: 4096, 1: 4096, 3: 768, 5: 1152, 6: 320}      # positions a slot may hold in these tests (others: 256)
CAP = 256
SWITCHES = {"default": {}, "nofuse": {"SPARKMI_NO_FUSE_O": "1"}, "fuse2": {"SPARKMI_FUSE2_ROWS": "8"}, "pf0": {"SPARKMI_ATTN_PF2": "0"}}


def _caps(slots):
    return {s: CAPS.get(s, CAP) for s in range(slots)}


class Engines:
    """(page size, cache type, switches) -> (paged engine, contiguous twin), built on first use, closed with the module"""

    def __init__(self, cfg, arena):
        self.cfg, self.arena, self.paged, self.twins = cfg, arena, {}, {}

    def get(self, P, kv, variant):
        slots = 64 if variant == "default" else 8
        caps = _caps(slots)
        if (kv, variant) not in self.twins:
            e = X.make_engine(self.cfg, self.arena, kv, slots, SWITCHES[variant])
            e.cache = X.Cache(e, cap=caps)
            self.twins[(kv, variant)] = e
        if (P, kv, variant) not in self.paged:
            pages = sum(-(-c // P) for c in caps.values())
            e = X.make_engine(self.cfg, self.arena, kv, slots, SWITCHES[variant], kv_page_tokens=P, kv_pages=pages + 2)
            e.cache = X.Cache(e, page=P, cap=caps)
            # the scramble: the sentinel into every position of every slot, a page at a time, round-robin over the slots (the first
            # layer's writes draw the pages; the other layer under test gets the same contents)
            none = {s: np.zeros((0, 2, 64), np.float32) for s in caps}
            for layer in (0, 2):
                e.cache.load(layer, none, none, {s: -1 for s in caps})
            tables = [e.debug_page_table(s) for s in range(slots)]
            for s, pt in enumerate(tables):
                assert len(pt) == -(-caps[s] // P), f"slot {s}: {len(pt)} pages for {caps[s]} positions of {P}"
                assert (np.abs(np.diff(pt)) > 1).all(), f"page {P}: slot {s} holds consecutive pages: {pt[:12]} ..."
            assert len(np.unique(np.concatenate(tables))) == pages, "a page sits in two slots"
            print(f"[paged layer stages] page {P}, {kv}, {variant}: slot 0 holds pages {tables[0][:6]} ..., slot 1 {tables[1][:6]} ..., "
                  f"slot 5 {tables[5][:6]} ... of {pages + 2}")
            self.paged[(P, kv, variant)] = e
        return self.paged[(P, kv, variant)], self.twins[(kv, variant)]

    def close(self):
        for e in list(self.paged.values()) + list(self.twins.values()):
            e.close()


@pytest.fixture(scope="module")
def model():
    cfg = X.model_cfg()
    weights = X.model_weights(cfg)
    return cfg, weights, X.device_arena(cfg, weights)


@pytest.fixture(scope="module")
def engines(model):
    out = Engines(model[0], model[2])
    yield out
    out.close()
    X.report("paged layer stages", MEASURED)


def _edge(P, m):
    return [0, P - 1, P, P + 1, 2 * P - 1, 2 * P, 3 * P + 5][m % 7]


def _identity(P, n, long_rows=None):
    return [(m, (long_rows or {}).get(m, _edge(P, m + n))) for m in range(n)]


# case -> (switches, rows per call as a function of the page size, the attention form the calls take)
DECODE = {
    "1row-page-edges": ("default", lambda P: [[(0, p)] for p in X.paged_positions(P) if p < X.SEG], "k_attn<KV,1,1,1> (fused one-row, PG)"),
    "1row-page-edges-nofuse": ("nofuse", lambda P: [[(0, p)] for p in X.paged_positions(P) if p < X.SEG], "k_attn<KV,1,0,1> (one row, PG)"),
    "1row-1100": ("default", lambda P: [[(0, 1100)]], "k_attn<KV,0> with 2 segments + k_attn_merge, through pages"),
    "1row-4095-slot-end": ("default", lambda P: [[(0, 4095)]], "k_attn<KV,0> with 4 segments + k_attn_merge, through pages"),
    "2rows": ("default", lambda P: [_identity(P, 2)], "k_attn<KV,2,0,1> (slot == row, PG)"),
    "8rows": ("default", lambda P: [_identity(P, 8)], "k_attn<KV,2,0,1> (slot == row, PG)"),
    "17rows": ("default", lambda P: [_identity(P, 17)], "k_attn<KV,2,0,1> (slot == row, PG)"),
    "8rows-perm": ("default", lambda P: [[(int(s), _edge(P, m + 3)) for m, s in enumerate([5, 2, 7, 0, 3, 6, 1, 4])]], "k_attn<KV,0> (row descriptors)"),
    "8rows-long": ("default", lambda P: [_identity(P, 8, {1: 2050, 5: 1100})], "k_attn<KV,0> with 3 segments + k_attn_merge, through pages"),
    # (last of the 64-slot engines' cases: until here the slots from 17 on have never held a row)
    "64rows": ("default", lambda P: [_identity(P, 64)], "k_attn<KV,2,0,1> (slot == row, PG)"),
    "2rows-fuse2": ("fuse2", lambda P: [_identity(P, 2)], "k_attn<KV,2,2,1> (fused o_proj at 2 .. 8 rows, PG)"),
    "8rows-fuse2": ("fuse2", lambda P: [_identity(P, 8)], "k_attn<KV,2,2,1> (fused o_proj at 2 .. 8 rows, PG)"),
}


def _last(rows):
    return {int(s): int(rows[rows[:, 0] == s, 1].max()) for s in np.unique(rows[:, 0])}


def _tails_intact(llm, P, layer, last, tag):
    """(c) above each slot's last row: the rest of its last page and the page behind it; an idle slot: all its pages"""
    caps = llm.cache.cap
    for s, lp in last.items():
        n = min(caps[s], (lp // P + 2) * P) - (lp + 1)
        assert llm.cache.sentinel_intact(layer, s, lp + 1, n), f"{tag} slot {s}: positions above {lp} no longer hold the sentinel"
    idle = [s for s in caps if s not in last]
    for s in idle[-2:]:    # (above what an earlier case's rows left in the slot; never used: from position 0)
        top = llm.cache.top[(layer, s)]
        assert llm.cache.sentinel_intact(layer, s, top, caps[s] - top), f"{tag} idle slot {s}: its pages no longer hold the sentinel"


def _equal(a, b, tag, stage):
    for name in a:
        assert np.array_equal(a[name], b[name]), f"{tag} stage {stage} {name}: the paged engine's bits differ from the contiguous engine's"


@pytest.mark.parametrize("kv", ["f32", "bf16"])
@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("case", list(DECODE))
def test_paged_decode_stages_against_float64_and_the_contiguous_engine(model, engines, case, P, kv):
    from oracle.llm_ref import layer_stages_f64
    cfg, weights, _ = model
    variant, calls, form = DECODE[case]
    paged, twin = engines.get(P, kv, variant)
    for case_rows in calls(P):
        for layer in (0, 2):
            rows, x, kc, vc = X.decode_inputs(cfg, layer, case_rows, salts=range(len(case_rows)))
            last = _last(rows)
            for e in (paged, twin):
                e.cache.load(layer, kc, vc, last)
            tag = f"page {P}, {kv} KV, {form}, rows {case_rows if len(rows) <= 2 else case}, layer {layer}:"
            errs = MEASURED.setdefault((P, kv, case, str(case_rows[0]), layer), {})
            fused = (variant == "default" and len(rows) == 1 and rows[0, 0] == 0 and rows[0, 1] < X.SEG) or variant == "fuse2"
            with X.env(**SWITCHES[variant]):
                out0, ref0 = paged.debug_layer(layer, rows, x, 0), twin.debug_layer(layer, rows, x, 0)
                _equal(out0, ref0, tag, 0)
                _tails_intact(paged, P, layer, last, tag)
                if kv == "bf16":   # the reference attends over the cache as stored
                    for s, lp in last.items():
                        kc[s], vc[s] = paged.debug_get_kv(layer, s, 0, lp + 1)
                        kt, vt = twin.debug_get_kv(layer, s, 0, lp + 1)
                        assert np.array_equal(kc[s], kt) and np.array_equal(vc[s], vt), f"{tag} slot {s}: the two caches differ"
                ref = layer_stages_f64(cfg, weights, layer, rows, x, kc, vc, own_kv=kv == "f32")
                X.check_qkv(out0, ref, kv == "f32", tag, errs)
                for stage, name, want in ((1, "attn", "attn"), (2, "h", "h_mid"), (3, "act", "act"), (4, "h", "h_out")):
                    if stage == 1 and fused:    # stage 1 happens inside the fused kernel (no buffer to read)
                        continue
                    out = paged.debug_layer(layer, rows, x, stage)
                    _equal(out, twin.debug_layer(layer, rows, x, stage), tag, stage)
                    X.close(out[name], ref[want], f"{tag} stage {stage} {want}", errs, want)


PF_ENGINES = {"f32": ("f32", "default", "k_attn_pf<f32>"), "bf16": ("bf16", "default", "k_attn_pf2"), "bf16-pf0": ("bf16", "pf0", "k_attn_pf<bf16>")}
PF_PLANS = {"70+65+96": [(0, 70), (0, 65), (0, 96)], "651:38+300": [(651, 38), (0, 300)]}


@pytest.mark.parametrize("eng", list(PF_ENGINES))
@pytest.mark.parametrize("P", [16, 64])
@pytest.mark.parametrize("plan", list(PF_PLANS))
def test_paged_prompt_pass_stages_against_float64_and_the_contiguous_engine(model, engines, plan, P, eng):
    from oracle.llm_ref import layer_stages_f64
    cfg, weights, _ = model
    kv, variant, form = PF_ENGINES[eng]
    f32 = kv == "f32"
    paged, twin = engines.get(P, kv, variant)
    seqs, rows, x, kc, vc = X.prefill_inputs(cfg, 0, PF_PLANS[plan], 1000 + sum(n for _, n in PF_PLANS[plan]))
    last = {s: p0 + n - 1 for s, p0, n in seqs}
    for e in (paged, twin):
        e.cache.load(0, kc, vc, last)
    tag = f"page {P}, prompt pass {plan}, {form} + k_pgemm's KV append, layer 0:"
    errs = MEASURED.setdefault((P, eng, "pf " + plan, 0), {})
    out0, ref0 = paged.debug_prefill_layer(0, seqs, x, 0), twin.debug_prefill_layer(0, seqs, x, 0)
    _equal(out0, ref0, tag, 0)
    _tails_intact(paged, P, 0, last, tag)
    if not f32:
        for s, p0, n in seqs:
            kc[s], vc[s] = paged.debug_get_kv(0, s, 0, p0 + n)
    ref = layer_stages_f64(cfg, weights, 0, rows, x, kc, vc, own_kv=f32)
    X.check_qkv(out0, ref, f32, tag, errs)
    for stage, name, want in ((1, "attn", "attn"), (2, "h", "h_mid"), (3, "act", "act"), (4, "h", "h_out")):
        out = paged.debug_prefill_layer(0, seqs, x, stage)
        _equal(out, twin.debug_prefill_layer(0, seqs, x, stage), tag, stage)
        X.close(out[name], ref[want], f"{tag} stage {stage} {want}", errs, want)


def test_debug_entry_points_on_a_paged_handle(model, engines):
    """set_kv / get_kv round-trip across page edges; a pool too small is an error that leaves the engine usable; a contiguous
    engine has no page table."""
    from sparkmi._lib import SparkMIError
    cfg, _, arena = model
    paged, twin = engines.get(16, "f32", "nofuse")
    assert len(twin.debug_page_table(0)) == 0
    rng = np.random.default_rng(5)
    k, v = rng.standard_normal((2, 50, 2, 64)).astype(np.float32)
    paged.debug_set_kv(1, 2, k, v, pos0=7)                  # positions 7 .. 56: four pages, the first and the last partly
    k2, v2 = paged.debug_get_kv(1, 2, 7, 50)
    assert np.array_equal(k, k2) and np.array_equal(v, v2)
    assert np.array_equal(paged.debug_get_kv(1, 2, 16, 16)[0], k[9: 25])
    small = X.make_engine(cfg, arena, "f32", 2, kv_page_tokens=16, kv_pages=3)
    try:
        x = X.row_x(cfg, 0, 70)[None]
        with pytest.raises(SparkMIError):
            small.debug_layer(0, [(1, 70)], x, 0)            # 5 pages needed
        with pytest.raises(SparkMIError):
            small.debug_set_kv(0, 0, k, v, pos0=7)           # 4 pages needed
        assert small.debug_layer(0, [(1, 40)], x, 2)["h"].shape == (1, cfg.hidden_size)
        assert len(small.debug_page_table(1)) == 3 and len(small.debug_page_table(0)) == 0
    finally:
        small.close()
