"""Runs in a subprocess (it claims the module name `minidiff`): the plug-in backend class
(minidiff_amd.plugin.hip_backend), bound to the CPU test double, must be a complete backend —
every public function of the table, DeviceArray as its tensor class — and reproduce the
reference's golden results (tests/golden/: README example and every golden case) through the tape."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from minidiff_amd import _capi  # noqa: E402

_capi.use_library(os.path.join(ROOT, "oracle", "_build", "libmdhip_host.so"))

import numpy as np  # noqa: E402
import golden_util as gu  # noqa: E402
from minidiff_amd.hip_backend import HipBackendTable  # noqa: E402
from minidiff_amd.ndarray import DeviceArray  # noqa: E402

md, plugin, Backend = gu.plugin_engine()
assert issubclass(plugin.hip_backend, Backend) and plugin.hip_backend.tensor_class is DeviceArray
missing = [k for k in vars(HipBackendTable) if not k.startswith("_") and getattr(plugin.hip_backend, k, None) is not getattr(HipBackendTable, k)]
assert not missing, missing
assert isinstance(md.Tensor([1.0, 2.0])._data, DeviceArray)

# README (reference README.md:13-36)
x = md.Tensor([[0, 2, -2, 1], [-1, -1, -2, -2]], allow_grad=True)
y = md.Tensor([[2, 3, 4, 5], [0, -1, -3, 2]], allow_grad=True)
f = 2 * y * md.sin(x) - x ** 2
f.backward(allow_higher_order=True)
g = gu.golden()["cfg"]
assert np.allclose(x.grad.as_numpy(), g["cfg1/dx"], rtol=1e-13) and np.allclose(y.grad.as_numpy(), g["cfg1/dy"], rtol=1e-13)
x.grad.backward()
assert np.allclose(x.grad.as_numpy(), g["cfg1/d2x"], rtol=1e-13) and np.allclose(y.grad.as_numpy(), g["cfg1/d2xy"], rtol=1e-13)

n = 0
with np.errstate(all="ignore"):
    for key in gu.case_keys():
        gu.run_case_on(md, key, exact=False)
        n += 1
print(f"DROPIN-OK {n} golden cases through the tape on the plug-in backend")
