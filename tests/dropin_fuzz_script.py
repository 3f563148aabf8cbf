"""Runs in a subprocess (it claims the module name `minidiff`). Runs the random forward+backward
programs of tests/fuzz_tape.py through the tape on the plug-in backend class
(minidiff_amd.plugin.hip_backend) bound to the CPU test double, and pickles outputs, gradients
(second order every fourth case) or the exception type of each case — the form
tests/golden/make_dropin_golden.py records for the reference's NumPy backend.
    dropin_fuzz_script.py N_CASES SEED OUT_PATH      (MDHIP_LAZY=1: fused chains)"""
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

n_cases, seed, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
from minidiff_amd import _capi  # noqa: E402

_capi.use_library(os.path.join(ROOT, "oracle", "_build", "libmdhip_host.so"))

import numpy as np  # noqa: E402
import golden_util as gu  # noqa: E402

md = gu.plugin_engine()[0]

# fuzz_tape builds engines lazily; only its program generator is used here
import fuzz_tape  # noqa: E402

results = []
for i in range(n_cases):
    second = (i % 4 == 0)
    try:
        with np.errstate(all="ignore"):
            o, l, g1, g2, dt = fuzz_tape.run(md, seed, i, second)
        results.append(("ok", o, l, g1, g2, np.dtype(dt).name))
    except Exception as e:  # the two backends must fail alike
        results.append(("raise", type(e).__name__))
with open(out_path, "wb") as f:
    pickle.dump(results, f)
print(f"DROPIN-FUZZ {len(results)} cases, {sum(r[0] == 'raise' for r in results)} raised")
