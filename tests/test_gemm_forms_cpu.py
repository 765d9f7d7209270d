"""Which kernel form every layer GEMM and the lm_head start with (``smi_llm_gemm_forms`` of libsparkmi_diag.so: host only, the pick
functions the launch sites call) against tests/golden/gemm_forms.json -- the kernel trace of the commit before the picks existed,
reduced by tools/gemm_forms_trace.py: per case the launches in order as [kernel, grid x, y, z, threads, LDS bytes as the trace
reports them (static only), dynamic LDS bytes].  Name, grid, block, dynamic LDS and the number of launches must be the trace's.
Cases: ``<shape>/<cache>/decode[/<switch>]/M=<rows>`` -- three decode steps of M rows in identity slots -- and
``<shape>/<cache>/prefill/tokens=<n>`` -- a prompt pass over n - 1 rows, then the one-row step of the last token."""
import ctypes as C
import dataclasses
import json
import os
import re

import pytest

from sparkmi import _lib, config as cfgs
from sparkmi.arena import llm_cfg_struct

GEMM_KERNELS = ("k_gemm", "k_down", "k_resid_comb", "k_pgemm", "k_lm")     # (k_gemm: also k_gemm_hot, k_gemm_x)
LAYERS = (_lib.SMI_LAYER_FIRST, _lib.SMI_LAYER_MIDDLE, _lib.SMI_LAYER_LAST)
PF_PGEMM = 2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "gemm_forms.json")))


def _shape(name):
    # the trace's shapes: tiny_llm() (TPC 2, 4 heads) and the 0.5B widths with three layers (TPC 10, 14 heads)
    return cfgs.tiny_llm() if name == "tiny" else dataclasses.replace(cfgs.spark_0p5b_llm(), num_hidden_layers=3)


def _forms(shape, kv, M, layer, **flags):
    cs = llm_cfg_struct(_shape(shape), 64, 576, kv, False)
    out = (_lib.GemmFormInfo * 5)()
    d = _lib.diag()
    d.check(d.smi_llm_gemm_forms(C.byref(cs), M, layer, C.byref(_lib.GemmFlags(**flags)), out), "smi_llm_gemm_forms")
    return list(out)


def _launches(info):
    """the trace entries [kernel, grid x, y, threads, dynamic LDS] of one picked launch"""
    if info.launches == 0:
        return []
    names = info.kernel.decode().split("+")
    first = [names[0], info.grid[0], info.grid[1], info.block, info.lds_bytes]
    if len(names) == 2:
        assert info.launches == 2
        return [first, [names[1], info.grid2, 1, 64, 0]]
    return [first] * info.launches


def _step(shape, kv, M, **flags):
    """the GEMM launches of one decode step over three layers: per layer QKV, o_proj, gate_up, down_proj; then lm_head"""
    out = []
    for layer in LAYERS:
        forms = _forms(shape, kv, M, layer, **flags)
        for f in forms[:4]:
            out += _launches(f)
    return out + _launches(forms[4])


def _expected(case):
    shape, kv, kind, *rest = case.split("/")
    if kind == "prefill":
        rows = int(rest[0].split("=")[1]) - 1
        out = []
        for layer in LAYERS:      # the last layer of a prompt pass ends after its K/V append
            forms = _forms(shape, kv, rows, layer, pass_=PF_PGEMM)
            for f in forms[:1] if layer == _lib.SMI_LAYER_LAST else forms[:4]:
                out += _launches(f)
        return out + _step(shape, kv, 1)
    flags = {}
    if rest[0] == "no_fuse_o":
        flags["fused"] = 0
    elif rest[0].startswith("tune2="):
        flags["tune2"] = int(rest[0].split("=")[1])
    M = int(rest[-1].split("=")[1])
    return 3 * _step(shape, kv, M, **flags)


def _traced(entries):
    return [[e[0], e[1], e[2], e[4], e[6]] for e in entries if e[0].startswith(GEMM_KERNELS)]


def test_every_traced_case(golden):
    assert len(golden) == 46
    for case, entries in golden.items():
        assert all(e[3] == 1 for e in entries), case           # no grid z anywhere
        assert _expected(case) == _traced(entries), case


def test_names_between_traced_row_counts(golden):
    """For every M in 1 .. 64 the kernel names are those of the nearest traced row count at or below M."""
    for shape in ("tiny", "half"):
        traced = sorted(int(m.group(1)) for c in golden if (m := re.fullmatch(rf"{shape}/bf16/decode/M=(\d+)", c)))
        assert traced[0] == 1
        for M in range(1, 65):
            below = max(t for t in traced if t <= M)
            for layer in LAYERS:
                got = [f.kernel for f in _forms(shape, "bf16", M, layer)]
                want = [f.kernel for f in _forms(shape, "bf16", below, layer)]
                assert got == want, (shape, M, below, layer)


def test_exact_weights_mode_picks_k_gemm_x_everywhere():
    """exact = 1 (smi_llm_cfg.weights_exact): at every M in 1 .. 64, either cache type and the first / middle / last
    layer all five GEMMs are k_gemm_x<PRO,EPI,kv> -- never a bf16 form -- on grid ((NT + 3) / 4, ceil(M / 16)) with 256 threads, one
    launch and no dynamic LDS; the o_proj is there even at one row in slot 0 (the mode has no fused attention + o_proj).  The golden
    trace has no exact case and stays as it is."""
    PRO_PLAIN, PRO_NORM, EPI_RESID, EPI_SWIGLU, EPI_QKV, EPI_LM = 0, 1, 0, 1, 2, 3
    for shape in ("tiny", "half"):
        c = _shape(shape)
        Q, KV = c.num_attention_heads * c.head_dim, c.num_key_value_heads * c.head_dim
        nts = [(Q + 2 * KV) // 16, c.hidden_size // 16, 2 * c.intermediate_size // 16, c.hidden_size // 16, (c.vocab_size + 15) // 16]
        for kv in ("bf16", "f32"):
            kvf = int(kv == "f32")
            names = [f"k_gemm_x<{PRO_NORM},{EPI_QKV},{kvf}>", f"k_gemm_x<{PRO_PLAIN},{EPI_RESID},0>", f"k_gemm_x<{PRO_NORM},{EPI_SWIGLU},0>",
                     f"k_gemm_x<{PRO_PLAIN},{EPI_RESID},0>", f"k_gemm_x<{PRO_NORM},{EPI_LM},0>"]
            for M in range(1, 65):
                for layer in LAYERS:
                    forms = _forms(shape, kv, M, layer, exact=1)
                    for i, f in enumerate(forms):
                        got = (f.kernel.decode(), f.grid[0], f.grid[1], f.block, f.launches, f.lds_bytes)
                        want = (names[i], (nts[i] + 3) // 4, (M + 15) // 16, 256, 1, 0)
                        assert got == want, (shape, kv, M, layer, i, got, want)
                    assert [f.kernel for f in _forms(shape, kv, M, layer, exact=1, fused=1)] == [f.kernel for f in forms], "fused o_proj in the exact mode"
        # the config's own field gives the same picks as the flag
        cs = llm_cfg_struct(c, 64, 576, "bf16", False, weights_exact=True)
        out = (_lib.GemmFormInfo * 5)()
        d = _lib.diag()
        d.check(d.smi_llm_gemm_forms(C.byref(cs), 1, _lib.SMI_LAYER_FIRST, C.byref(_lib.GemmFlags()), out), "smi_llm_gemm_forms")
        assert [f.kernel for f in out] == [f.kernel for f in _forms(shape, "bf16", 1, _lib.SMI_LAYER_FIRST, exact=1)]
        assert out[1].launches == 1 and _forms(shape, "bf16", 1, _lib.SMI_LAYER_FIRST)[1].launches == 0, "one row: only the bf16 path fuses the o_proj away"
