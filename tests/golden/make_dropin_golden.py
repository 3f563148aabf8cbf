"""GENERATOR (not a test): runs the random forward+backward programs of tests/fuzz_tape.py
(seed 7, cases 0..299, second order every fourth case) through the UNMODIFIED reference on
its own NumPy backend and records outputs, losses, gradients and raised exception types as
data: dropin_fuzz.npz + dropin_fuzz.json. tests/test_dropin_reference.py compares the
plug-in backend against this record, so the suite needs no reference checkout.

    MINIDIFF_REFERENCE=<checkout of ahoynodnarb/minidiff> python tests/golden/make_dropin_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SEED, N_CASES = 7, 300


def main():
    ref = os.environ.get("MINIDIFF_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "minidiff")):
        raise SystemExit("set MINIDIFF_REFERENCE to a checkout of the reference (the directory holding minidiff/)")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, ref)
    sys.argv = [sys.argv[0], "--backend", "minidiff.backend.numpy"]     # minidiff parses sys.argv at import
    import minidiff as md
    assert md.__file__.startswith(ref), md.__file__
    import fuzz_tape   # only its program generator is used here

    arrays, meta = {}, []
    for i in range(N_CASES):
        second = (i % 4 == 0)
        try:
            with np.errstate(all="ignore"):
                o, loss, g1, g2, dt = fuzz_tape.run(md, SEED, i, second)
        except Exception as e:   # the plug-in must fail alike
            meta.append({"status": "raise", "raise": type(e).__name__})
            continue
        arrays[f"{i}/out"] = o
        arrays[f"{i}/loss"] = np.float64(loss)
        for tag, grads in (("g1", g1), ("g2", g2)):
            for k, g in enumerate(grads or []):
                if g is not None:
                    arrays[f"{i}/{tag}/{k}"] = g
        meta.append({"status": "ok", "dtype": np.dtype(dt).name,
                     "g1": [g is not None for g in g1], "g2": None if g2 is None else [g is not None for g in g2]})
    np.savez_compressed(os.path.join(HERE, "dropin_fuzz.npz"), **arrays)
    info = {"generator": "tests/golden/make_dropin_golden.py", "program_generator": "tests/fuzz_tape.py", "seed": SEED,
            "numpy": np.__version__, "python": sys.version.split()[0], "reference": "ahoynodnarb/minidiff, NumPy backend",
            "cases": meta}
    with open(os.path.join(HERE, "dropin_fuzz.json"), "w") as f:
        json.dump(info, f, indent=0)
    print(f"{N_CASES} cases, {sum(m['status'] == 'raise' for m in meta)} raised -> tests/golden/dropin_fuzz.npz")


if __name__ == "__main__":
    main()
