"""DevBuf (spark-tts_amd/csrc/smi_common.h), the one owner of every device allocation, on a machine without a GPU: there every
hipMalloc / hipHostMalloc fails at once, which is exactly the path the handles' create functions unwind through.
tests/host/dev_owner_host.hip is a stand-alone program (its own main, the library's header only); its host half is built under
AddressSanitizer and UBSan (the runtime linked statically into the executable) and run as its own process with nothing preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "dev_owner_host.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _gpu_visible():
    if os.path.exists("/dev/kfd"):
        return True
    import torch
    return torch.cuda.is_available()


def test_owner_unwinds_cleanly_when_every_allocation_fails(tmp_path):
    if _gpu_visible():
        pytest.skip("a GPU is visible: the sanitizer-instrumented program runs on machines without one only")
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not in this image")
    exe = str(tmp_path / "dev_owner_host")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "spark-tts_amd", "csrc"), SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0:exitcode=23"
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "dev_owner_host ok" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
