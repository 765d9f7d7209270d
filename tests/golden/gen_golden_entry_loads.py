#!/usr/bin/env python3
"""Records ``tests/golden/entry_loads_parent.npz`` on the GPU: token ids and the last step's residual row of the one-row greedy
decodes of tests/test_entry_loads_gpu.py (its shapes, prompts and step count are imported, not restated), as the library in the
tree computes them.  Run ONCE, on the build of the commit whose bits are the reference -- the parent of the change that
reworked the address arithmetic of the one-row kernels' first loads -- and never on the code under test:

    python tests/golden/gen_golden_entry_loads.py <commit> [out.npz]

``parent_commit`` and ``parent_smi_llm_sha256`` (of spark-tts_amd/csrc/smi_llm.hip as it stands when this runs) name that
build in the file.  Data only."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "spark-tts_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_entry_loads_gpu as T   # noqa: E402

if __name__ == "__main__":
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else T.FIXTURE
    src = os.path.join(ROOT, "spark-tts_amd", "csrc", "smi_llm.hip")
    rec = {"parent_commit": np.array(commit), "parent_smi_llm_sha256": np.array(hashlib.sha256(open(src, "rb").read()).hexdigest())}
    for name in T.SHAPES:
        for ctx, (toks, hid) in T.decode_all(name).items():
            rec[f"{name}_{ctx}_tokens"], rec[f"{name}_{ctx}_hidden"] = toks, hid
            print(name, ctx, toks.tolist(), hex(int(hid[0])))
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")
