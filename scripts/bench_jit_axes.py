"""Fused chains over three / four axes: kernel-time workloads for `rocprofv3 --kernel-trace --stats` and wall times.

    python scripts/bench_jit_axes.py [--lib path/to/libmdhip.so] [--ab]

64x512x512 float32: the eager three-axis multiply (the yardstick: a streaming kernel of these bytes), the chain
`(x * g[:, None, :] + h[None, :, None]) ** 2` as three eager calls and as one lazy program, a two-output pair over the same leaves
(materialize_many), and the four-axis form at 32x64x32x256. Segments are separated by a tiny reduction so that a kernel trace
splits by order; `--ab` repeats the lazy chain under the options jit_u / jit_blocks / jit_axes_wide. `--lib` binds another
build of the library (the parent commit's, for the before side)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

args = sys.argv[1:]
lib = _capi.use_library(args[args.index("--lib") + 1]) if "--lib" in args else _capi.load()
rng = np.random.default_rng(0)
REPS = 20


def arr(*shape):
    return nd.asarray(rng.standard_normal(shape).astype(np.float32))


tiny = arr(64)


def seg(name, fn, nbytes):
    for _ in range(3):
        fn()
    lib.sync()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    lib.sync()
    dt = (time.perf_counter() - t0) / REPS
    print(f"{name:64s} {dt * 1e6:9.1f} us/call wall  {nbytes / dt / 1e9:8.1f} GB/s  ({nbytes / 1e6:.0f} MB)", flush=True)
    nd.sum(tiny).get()    # separator in the kernel trace
    lib.sync()


B, R, C = 64, 512, 512
x, g, h = arr(B, R, C), arr(B, 1, C), arr(1, R, 1)
n4 = x.size * 4
x4, g4, h4 = arr(32, 64, 32, 256), arr(1, 64, 1, 256), arr(32, 1, 32, 1)
m4 = x4.size * 4


def chain(a, b, c):
    return nd.power(nd.add(nd.multiply(a, b), c), 2)


nd.set_lazy(False)
seg("eager x * (B,1,C)", lambda: nd.multiply(x, g), 2 * n4)
seg("eager (x * (B,1,C) + (1,R,1)) ** 2, three calls", lambda: chain(x, g, h), 6 * n4)
seg("eager (N,C,H,W) * (1,C,1,W)", lambda: nd.multiply(x4, g4), 2 * m4)
nd.set_lazy(True)
seg("lazy (x * (B,1,C) + (1,R,1)) ** 2", lambda: nd.materialize(chain(x, g, h)), 2 * n4)
seg("lazy pair: chain, (x * g + h) * g  (materialize_many)",
    lambda: nd.materialize_many([chain(x, g, h), nd.multiply(nd.add(nd.multiply(x, g), h), g)]), 3 * n4)
seg("lazy ((N,C,H,W) * (1,C,1,W) + (N,1,H,1)) ** 2", lambda: nd.materialize(chain(x4, g4, h4)), 2 * m4)
if "--ab" in args:
    opt = lambda k, v: lib.debug_set_option(k.encode(), int(v))   # noqa: E731
    for u in (1, 2, 4):
        for blocks in (2, 4, 8):
            opt("jit_u", u)
            opt("jit_blocks", blocks)
            seg(f"lazy chain, jit_u = {u}, jit_blocks = {blocks}", lambda: nd.materialize(chain(x, g, h)), 2 * n4)
    opt("jit_u", 0)
    opt("jit_blocks", 0)
    opt("jit_axes_wide", 1)
    seg("lazy chain, 64-bit index form", lambda: nd.materialize(chain(x, g, h)), 2 * n4)
    opt("jit_axes_wide", 0)
    opt("jit", 0)
    seg("lazy chain, interpreter (jit = 0)", lambda: nd.materialize(chain(x, g, h)), 2 * n4)
    opt("jit", 1)
nd.set_lazy(False)
