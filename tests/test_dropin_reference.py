"""Drop-in proof (CPU test double): the plug-in backend class minidiff_amd.plugin.hip_backend
reproduces the reference's own results — its golden cases, and its NumPy backend on 300 random
forward+backward programs — recorded as data under tests/golden/ (make_golden.py,
make_dropin_golden.py), so no reference checkout is needed."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_reference_runs_on_plugin_backend(lib, on_gpu):
    if on_gpu:
        pytest.skip("runs against the CPU test double")
    p = subprocess.run([sys.executable, os.path.join(HERE, "dropin_reference_script.py")], capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DROPIN-OK" in p.stdout


def test_reference_fuzz_numpy_backend_vs_plugin(lib, on_gpu, tmp_path):
    """300 random forward+backward programs (tests/fuzz_tape.py): the reference on its NumPy backend (recorded in
    tests/golden/dropin_fuzz.*) and the plug-in must agree on every output, gradient and raised exception type."""
    if on_gpu:
        pytest.skip("runs against the CPU test double")
    import pickle

    import numpy as np
    sys.path.insert(0, HERE)
    import fuzz_tape
    outs = {"numpy": _recorded_numpy_run(np)}
    for which, env in (("plugin", {"MDHIP_LAZY": "0"}), ("plugin-lazy", {"MDHIP_LAZY": "1"})):
        path = tmp_path / f"{which}.pkl"
        p = subprocess.run([sys.executable, os.path.join(HERE, "dropin_fuzz_script.py"), "300", "7", str(path)],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, **env))
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
        outs[which] = pickle.loads(path.read_bytes())
    assert len(outs["numpy"]) == len(outs["plugin"]) == len(outs["plugin-lazy"]) == 300
    for mode in ("plugin", "plugin-lazy"):   # the fused-chain layer sits under the same unmodified tape
        _compare(outs["numpy"], outs[mode], fuzz_tape, np)


def _recorded_numpy_run(np):
    """tests/golden/dropin_fuzz.* in the form dropin_fuzz_script.py pickles: one tuple per case."""
    with open(os.path.join(HERE, "golden", "dropin_fuzz.json")) as f:
        info = json.load(f)
    assert info["seed"] == 7 and len(info["cases"]) == 300
    arrs = np.load(os.path.join(HERE, "golden", "dropin_fuzz.npz"))
    out = []
    for i, c in enumerate(info["cases"]):
        if c["status"] == "raise":
            out.append(("raise", c["raise"]))
            continue
        grads = {tag: None if c[tag] is None else [arrs[f"{i}/{tag}/{k}"] if present else None for k, present in enumerate(c[tag])]
                 for tag in ("g1", "g2")}
        out.append(("ok", arrs[f"{i}/out"], float(arrs[f"{i}/loss"]), grads["g1"], grads["g2"], c["dtype"]))
    return out


def _compare(ref, got, fuzz_tape, np):
    n_ok = 0
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a[0] == b[0], (i, a[:2], b[:2])
        if a[0] == "raise":
            assert a[1] == b[1], (i, a, b)
            continue
        n_ok += 1
        dt = np.dtype(a[5]).type
        fuzz_tape.close(b[1], a[1], dt, f"case {i} output")
        for k, (ga, gb) in enumerate(zip(a[3], b[3])):
            fuzz_tape.close(gb, ga, dt, f"case {i} grad[{k}]")
        if a[4] is not None:
            for k, (ga, gb) in enumerate(zip(a[4], b[4])):
                fuzz_tape.close(gb, ga, dt, f"case {i} second-order grad[{k}]")
    assert n_ok > 150
