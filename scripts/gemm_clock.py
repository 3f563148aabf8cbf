#!/usr/bin/env python3
"""In-kernel clock and main-loop time of the float32 GEMM under SUSTAINED load: MDHIP_GEMM_STAMP=1 makes libmdhip launch the
stamped (diagnostic) instantiation of the kernel, which writes s_memtime / s_memrealtime differences around every block's main loop
into a persistent buffer of their own (no sync behind the launches); the last launch's figures are printed at exit.

  usage: gemm_clock.py N LAYOUT [launches [ROUTE]]
  ROUTE  auto (default: the library's choice) | fp32 (the fma chain: gemm_bf16x3 = 0) | bf16x3[:LOOP] (the six bf16 products on
         every shape the kernel takes, k loop LOOP: option gemm_bf16x3_loop; for these the exit line also gives the shader cycles
         per k-tile and CU, to set against the 3072 the matrix pipe needs: 2 waves per SIMD x 48 MFMAs x 32 cycles, or under
         bf16x3:3 x 96 MFMAs x 16 cycles)
Take >= 2 s of launches (a 4096^3 bf16x3 product is ~0.6 ms: 4000) so that the clock has settled where the chip holds it."""
import os, sys
os.environ["MDHIP_EXPERIMENTS"] = "1"   # the library reads experiment variables only behind this gate
os.environ["MDHIP_GEMM_STAMP"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ctypes as C
import numpy as np
from minidiff_amd import _capi, ndarray as nd
lib = _capi.load()
n, layout = int(sys.argv[1]), sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2500
route = sys.argv[4] if len(sys.argv) > 4 else "auto"
if route == "fp32":
    lib.debug_set_option(b"gemm_bf16x3", 0)
elif route.startswith("bf16x3"):
    lib.debug_set_option(b"gemm_bf16x3", 2)
    if ":" in route:
        lib.debug_set_option(b"gemm_bf16x3_loop", int(route.split(":")[1]))
elif route != "auto":
    raise SystemExit(__doc__)
rng = np.random.default_rng(0)
A = nd.asarray(rng.standard_normal((n, n), dtype=np.float32)); B = nd.asarray(rng.standard_normal((n, n), dtype=np.float32))
a, b = {"NN": lambda: (A, B), "NT": lambda: (A, nd.asarray(np.ascontiguousarray(np.asarray(B).T)).T),
        "TN": lambda: (nd.asarray(np.ascontiguousarray(np.asarray(A).T)).T, B)}[layout]()
e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_float()
lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
for _ in range(reps - 50):
    nd.matmul(a, b)
lib.event_record(e0)
for _ in range(50):
    nd.matmul(a, b)
lib.event_record(e1)
lib.sync()
lib.event_elapsed_ms(e0, e1, C.byref(ms))
print(f"{layout} {n}^3 ({route}): {ms.value / 50 * 1e3:.1f} us per launch over the last 50 of {reps} back-to-back launches = {2.0 * n ** 3 / (ms.value / 50 * 1e-3) / 1e12:.1f} TFLOP/s", file=sys.stderr)
