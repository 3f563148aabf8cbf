#!/usr/bin/env python3
"""Lazy mode: reductions of a pending chain over a middle axis or its leading axes (the gradients of a (B,1,C) scale and of a (C,)
weight on a 3-D activation) — wall time per call over back-to-back calls between two mdhip_sync, after a warm-up; median of the
repetitions with the spread (min, max, interquartile range), and the bytes per second that ONE read of the chain's distinct operands
plus one write of the result in that time amounts to (the fused byte count). The method of scripts/bench_fused_rows.py. A call builds
the chain and reduces it, as a training step does; the chain is dropped unevaluated where the reduction is fused (counter
vm_reduce_axis) and materialised first where it is not. Run it on two builds of the library, alternated, to compare them: a build
without the fused form reports 0 fused calls and times the two-pass route.
usage: bench_fused_axis.py [--reps 40] [--calls 20] [--only NAME] [--trace]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402


def cases(rng):
    """(name, dtype, fused bytes, call)"""
    out = []

    def f(dt, *s):
        return nd.asarray(rng.standard_normal(s).astype(dt))

    def scale_grad(shape, dt):                      # sum(g * x, axis=1, keepdims=True): the gradient of a (B,1,C) scale
        g, x = f(dt, *shape), f(dt, *shape)
        n, kept = int(np.prod(shape)), shape[0] * shape[2]
        return (f"sum(g*x, 1, keepdims) {'x'.join(map(str, shape))} {np.dtype(dt).name}", (2 * n + kept) * np.dtype(dt).itemsize,
                lambda: nd.sum(nd.multiply(g, x), axis=1, keepdims=True))

    def gamma_grad(shape, dt):                      # sum(g * x * r, axis=(0, 1)), r of shape (B,R,1): the gradient of a (C,) weight
        g, x, r = f(dt, *shape), f(dt, *shape), f(dt, shape[0], shape[1], 1)
        n = int(np.prod(shape))
        return (f"sum(g*x*r, (0,1)) {'x'.join(map(str, shape))} {np.dtype(dt).name}", (2 * n + n // shape[2] + shape[2]) * np.dtype(dt).itemsize,
                lambda: nd.sum(nd.multiply(nd.multiply(g, x), r), axis=(0, 1)))

    out.append(scale_grad((64, 512, 512), np.float32))
    out.append(scale_grad((64, 512, 512), np.float64))
    out.append(scale_grad((8, 4096, 1024), np.float32))
    out.append(scale_grad((1024, 64, 256), np.float32))
    out.append(gamma_grad((64, 512, 512), np.float32))
    out.append(scale_grad((4, 64, 256), np.float32))       # launch cost: just above the floors (inner 256, n_red 64)
    out.append(scale_grad((4, 60, 256), np.float32))       # .. and just below them: not offered
    return out


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
    ap.add_argument("--only", default=None, help="cases whose name contains this text")
    ap.add_argument("--trace", action="store_true", help="--calls calls of each case and no timing: the run to put under a kernel trace")
    a = ap.parse_args()
    if a.reps < 30 and not a.trace:
        ap.error("at least 30 repetitions")
    lib = _capi.load()
    nd.set_lazy(True)
    print(f"# library {lib.target}; lazy mode; {a.reps} repetitions of {a.calls} back-to-back calls; times in ms per call")
    print(f"# {'case':58s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>9s} {'GB/s, fused bytes':>18s} {'fused':>6s}")
    for name, nbytes, fn in cases(np.random.default_rng(0)):
        if a.only and a.only not in name:
            continue
        if a.trace:
            for _ in range(a.calls):
                fn()
            lib.sync()
            print(f"  {name}: {a.calls} calls", flush=True)
            continue
        before = nd.FUSION_STATS.get("vm_reduce_axis", 0)
        fn()
        fused = nd.FUSION_STATS.get("vm_reduce_axis", 0) - before
        ms = measure(lib, fn, a.reps, a.calls)
        med = float(np.median(ms))
        q1, q3 = np.percentile(ms, [25, 75])
        print(f"  {name:58s} {med:9.4f} {ms.min():9.4f} {ms.max():9.4f} {q3 - q1:9.4f} {nbytes / med / 1e6:18.1f} {fused:6d}", flush=True)


if __name__ == "__main__":
    main()
