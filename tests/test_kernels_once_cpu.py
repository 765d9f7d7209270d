"""A kernel is compiled once.  Two ways it has been compiled twice without any test noticing, since both copies compute the same
results: a header full of kernels included by two translation units (every kernel of it then sits in two code objects under one
name), and a template parameter that a launch site switches on although the kernel never reads it (two symbols, one instruction
stream).  Both cost build time and module size only, so the built library is read here: no kernel symbol occurs in more than one
of libsparkmi.so's gfx950 code objects, and no two kernels have the same instruction text.  No GPU and no compilation: the code
objects are taken out of the library and disassembled."""
import collections
import glob
import hashlib
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "spark-tts_amd", "sparkmi", "libsparkmi.so")
OBJDUMP = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump", shutil.which("llvm-objdump")) if p and os.path.exists(p)), None)

_PADDING = re.compile(r"s_nop\b.*|s_code_end|\.\.\.")   # ('...': zero bytes that the disassembler elides)


def code_objects(lib, workdir):
    """the gfx950 code objects of a library, extracted into workdir (the bundles are written beside the file they come from)"""
    lib = shutil.copy(lib, workdir)
    subprocess.run([OBJDUMP, "--offloading", lib], check=True, capture_output=True, timeout=120)
    return sorted(glob.glob(os.path.join(workdir, "*gfx950*")))


def kernel_texts(co):
    """{kernel symbol: its instruction text} of one code object: addresses, <symbol+offset> operands, // comments and the
    s_nop / s_code_end / zero padding behind the last instruction stripped"""
    syms = subprocess.run([OBJDUMP, "-t", co], check=True, capture_output=True, text=True, timeout=120).stdout
    kernels = set(re.findall(r"\s(\S+)\.kd$", syms, flags=re.M))     # a kernel is a function with a descriptor
    dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True, timeout=300).stdout
    out, name, lines = {}, None, []

    def close():
        if name in kernels:
            while lines and _PADDING.fullmatch(lines[-1]):
                lines.pop()
            out[name] = "\n".join(lines)

    for ln in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", ln)
        if m:
            close()
            name, lines = m.group(1), []
            continue
        ln = re.sub(r"<[^>]*>", "", ln.split("//")[0]).strip()
        if ln and name is not None:
            lines.append(ln)
    close()
    assert set(out) == kernels, f"{co}: kernels without a disassembly: {sorted(kernels ^ set(out))[:5]}"
    return out


def duplicates(lib, workdir):
    """(kernel count, {symbol: the code objects holding it} for symbols in more than one, groups of symbols with one instruction text)"""
    where, same = collections.defaultdict(list), collections.defaultdict(list)
    for co in code_objects(lib, workdir):
        for sym, text in kernel_texts(co).items():
            where[sym].append(os.path.basename(co))
            same[hashlib.sha256(text.encode()).digest()].append(sym)
    shared = {s: c for s, c in where.items() if len(c) > 1}
    # (a symbol that sits in two code objects is reported once, as shared, not again as its own twin)
    twins = sorted(sorted(set(g)) for g in same.values() if len(set(g)) > 1)
    return sum(len(c) for c in where.values()), shared, twins


@pytest.fixture(scope="module")
def found(tmp_path_factory):
    if not os.path.exists(LIB):
        pytest.skip(f"{LIB} is not built")
    if OBJDUMP is None:
        pytest.skip("llvm-objdump of the ROCm tree not found")
    count, shared, twins = duplicates(LIB, str(tmp_path_factory.mktemp("co")))
    assert count, "no gfx950 kernel read from the library: the extraction or the disassembly's format has changed"
    return shared, twins


def test_no_kernel_symbol_in_two_code_objects(found):
    shared, _ = found
    report = "\n".join(f"  {s}: {', '.join(c)}" for s, c in sorted(shared.items()))
    assert not shared, f"{len(shared)} kernel symbols are compiled into more than one code object (a header of kernels included twice?):\n{report}"


def test_no_two_kernels_with_the_same_instructions(found):
    _, twins = found
    extra = sum(len(g) - 1 for g in twins)
    report = "\n".join("  " + "  ==  ".join(g) for g in twins)
    assert not twins, f"{extra} kernels repeat another kernel's instructions (a template parameter the kernel never reads?):\n{report}"
