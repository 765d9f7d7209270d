"""The hot entries of the one-row decode kernels rely on the build: -amdgpu-kernarg-preload-count (csrc/Makefile) makes the
command processor put their leading scalar parameters into SGPRs before a wave starts, and the kernel descriptor says how many
dwords (.amdhsa_user_sgpr_kernarg_preload_length).  A build without the flag, or a hot entry whose parameter list no longer
starts with its hot values, would still compute the same results -- only slower -- so the descriptors of the built library are
read here: every hot entry preloads exactly its hot dwords, and a kernel whose first parameter is a struct (k_lm32) preloads
none.  No GPU and no compilation: the gfx950 code objects are taken out of libsparkmi.so and their descriptors disassembled."""
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "spark-tts_amd", "sparkmi", "libsparkmi.so")
OBJDUMP = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")) if p and os.path.exists(p)), None)

# mangled-name fragment of each hot entry -> its hot dwords (pointers count two)
HOT = {
    "k_gemm_hot": 13,      # W, three operand pointers, KT, NT, work_blocks, one count, ldsb       (QKV and gate_up at one row)
    "k_down1_hot": 12,     # W, XS, residual source, gamma_next, KT, NT, work_blocks, wperm
    "k_attn_hot": 14,      # q, K, V, rows, W_o, work_blocks, max_pos, NTo, heads | group << 16
}


@pytest.fixture(scope="module")
def preload(tmp_path_factory):
    """{mangled kernel name: preload length} of every gfx950 kernel in the product library"""
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    if OBJDUMP is None:
        pytest.skip("llvm-objdump of the ROCm tree not found")
    d = tmp_path_factory.mktemp("kd")
    lib = shutil.copy(LIB, d)                                   # the bundles are written beside the file they come from
    subprocess.run([OBJDUMP, "--offloading", lib], check=True, capture_output=True, timeout=120)
    out = {}
    for co in glob.glob(os.path.join(d, "*gfx950*")):
        txt = subprocess.run([OBJDUMP, "-D", "-j", ".rodata", co], check=True, capture_output=True, text=True, timeout=120).stdout
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", txt, re.S):
            pl = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", m.group(2))
            out[m.group(1)] = int(pl.group(1)) if pl else 0    # (the directive is only printed when it is not zero)
    assert out, "no gfx950 kernel descriptor read from the library: the extraction or the disassembly's format has changed"
    return out


@pytest.mark.parametrize("frag", list(HOT))
def test_hot_entries_preload_their_hot_dwords(preload, frag):
    got = {k: v for k, v in preload.items() if frag in k}
    assert got, f"no {frag} kernel in the library"
    bad = {k: v for k, v in got.items() if v != HOT[frag] or v <= 0}
    assert not bad, f"{frag}: preload length {HOT[frag]} expected: {bad}"


def test_struct_first_kernels_preload_nothing(preload):
    got = {k: v for k, v in preload.items() if "k_lm32" in k}
    assert got, "no k_lm32 kernel in the library"
    assert all(v == 0 for v in got.values()), got
    # ... and so does every struct-only entry the hot kernels share their bodies with (k_down1 has none: its one entry is the
    # hot one), and the lm_head and finalize kernels (their hot entries gave no measurable gain and were not adopted)
    for frag in ("6k_gemmI", "6k_attnI", "4k_lmI", "10k_finalizeE"):
        sel = {k: v for k, v in preload.items() if frag in k}
        assert sel and all(v == 0 for v in sel.values()), (frag, {k: v for k, v in sel.items() if v})
