#!/usr/bin/env python3
"""std and argmax over the MIDDLE axis of (B, R, C) arrays: wall time per call over back-to-back calls between two mdhip_sync,
after a warm-up; median of the repetitions with the spread (min, max, interquartile range), and the bytes per second that ONE read
of the array in that time amounts to (the algorithmic minimum of both functions; std's kernels read the array twice).
The method of scripts/perf_cliffs.py, repeated. Run it on two builds of the library to compare them; options var_batched /
arg_batched 0 (--ab) give the previous routes of the same build: the composition and k_arg_block / k_arg_thread.
usage: bench_middle_axis.py [--reps 40] [--calls 20] [--ab] [--only BxRxC[x..]] [--axis 1] [--trace]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

SHAPES = [(64, 512, 512), (8, 4096, 1024), (1024, 64, 256), (4, 64, 256)]


def measure(lib, fn, reps, calls):
    for _ in range(3):
        fn()
    lib.sync()
    ms = []
    for _ in range(reps):
        lib.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        lib.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / calls)
    return np.array(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--ab", action="store_true", help="also time each case with var_batched / arg_batched set to 0")
    ap.add_argument("--only", default=None, help="one shape, as BxRxC (or more extents)")
    ap.add_argument("--axis", type=int, default=1, help="the reduced axis")
    ap.add_argument("--trace", action="store_true", help="--calls calls of each case and no timing: the run to put under a kernel trace")
    a = ap.parse_args()
    if a.reps < 30 and not a.trace:
        ap.error("at least 30 repetitions")
    lib = _capi.load()
    nd.set_lazy(False)
    known = {}
    for name in ("var_batched", "arg_batched"):
        v = C.c_int64()
        try:
            lib.debug_get_option(name.encode(), C.byref(v))
            known[name] = True
        except ValueError:
            known[name] = False
    print(f"# library {lib.target}; options known: {known}; {a.reps} repetitions of {a.calls} back-to-back calls; times in ms per call")
    print(f"# {'case':44s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>9s} {'GB/s of one read':>17s}")
    shapes = [tuple(int(v) for v in a.only.split("x"))] if a.only else SHAPES
    rng = np.random.default_rng(0)
    for shape in shapes:
        for dt in (np.float32, np.float64):
            x = nd.asarray((rng.standard_normal(shape) * 3 + 10).astype(dt))
            nbytes = x.size * np.dtype(dt).itemsize
            cases = [("std", "var_batched", lambda: nd.std(x, axis=a.axis)), ("argmax", "arg_batched", lambda: nd.argmax(x, axis=a.axis))]
            for fname, opt, fn in cases:
                if a.trace:
                    for _ in range(a.calls):
                        fn()
                    lib.sync()
                    print(f"  {fname} {'x'.join(map(str, shape))} {np.dtype(dt).name}: {a.calls} calls", flush=True)
                    continue
                for off in ((False, True) if a.ab and known[opt] else (False,)):
                    if off:
                        lib.debug_set_option(opt.encode(), 0)
                    try:
                        ms = measure(lib, fn, a.reps, a.calls)
                    finally:
                        if off:
                            lib.debug_set_option(opt.encode(), 1)
                    med = float(np.median(ms))
                    q1, q3 = np.percentile(ms, [25, 75])
                    tag = f"{fname} {'x'.join(map(str, shape))} {np.dtype(dt).name}" + (f" [{opt}=0]" if off else "")
                    print(f"  {tag:44s} {med:9.4f} {ms.min():9.4f} {ms.max():9.4f} {q3 - q1:9.4f} {nbytes / med / 1e6:17.1f}", flush=True)


if __name__ == "__main__":
    main()
