#!/usr/bin/env python3
"""Lazy mode: float16 chains recorded behind MDHIP_LAZY_F16 (ndarray.set_lazy_float16) against the same calls launched one by one
— wall time per call over back-to-back calls between two mdhip_sync, after a warm-up; median of the repetitions with the spread
(min, max, interquartile range), the bytes per second that ONE read of the chain's distinct operands plus one write of the result
in that time amounts to (the fused byte count), and the C-ABI compute calls one call makes. The method of
scripts/bench_fused_narrow.py. A call builds the chain and forces its result into memory.
On a build without the switch (the parent commit) the script measures lazy mode as it was: every float16 call is one native launch.
Run it on the two builds, alternated, to compare them; --no-half measures this build with the switch off.
usage: bench_fused_half.py [--reps 40] [--calls 20] [--only NAME] [--no-half] [--trace]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402
from bench_fused_narrow import count_calls, measure  # noqa: E402

f16, f32 = np.float16, np.float32


def gelu(x):
    """0.5 * x * (1 + tanh(0.7979 * (x + 0.044715 * x * x * x))): nine float16 calls"""
    cube = nd.multiply(nd.multiply(nd.multiply(x, 0.044715), x), x)
    t = nd.tanh(nd.multiply(nd.add(x, cube), 0.7979))
    return nd.multiply(nd.multiply(x, 0.5), nd.add(t, 1.0))


def cases(rng):
    """(name, fused bytes, call)"""
    def f(*s):
        return nd.asarray(rng.standard_normal(s).astype(f16))

    R, Cc = 8192, 4096
    n = R * Cc
    x, y, w, b = f(R, Cc), f(R, Cc), f(Cc), f(Cc)
    xs = f(256, 512)
    return [
        (f"x16 * w(C,) + b(C,) {R}x{Cc}", 4 * n + 4 * Cc, lambda: nd.materialize(nd.add(nd.multiply(x, w), b))),
        (f"maximum(x16 * w + b, 0) {R}x{Cc}", 4 * n + 4 * Cc, lambda: nd.materialize(nd.maximum(nd.add(nd.multiply(x, w), b), 0))),
        (f"gelu(x16) {R}x{Cc}", 4 * n, lambda: nd.materialize(gelu(x))),
        (f"sum(astype(x16 * y16, f32), -1) {R}x{Cc}", 4 * n + 4 * R, lambda: nd.materialize(nd.sum(nd.astype(nd.multiply(x, y), f32), axis=-1))),
        ("gelu(x16) 256x512", 4 * 256 * 512, lambda: nd.materialize(gelu(xs))),      # under 2^18 elements: the interpreter kernels, launch cost
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--only", default=None, help="cases whose name contains this text")
    ap.add_argument("--no-half", action="store_true", help="leave the float16 sub-switch off")
    ap.add_argument("--trace", action="store_true", help="--calls calls of each case and no timing: the run to put under a kernel trace")
    a = ap.parse_args()
    if a.reps < 30 and not a.trace:
        ap.error("at least 30 repetitions")
    lib = _capi.load()
    nd.set_lazy(True)
    half = hasattr(nd, "set_lazy_float16") and not a.no_half
    if half:
        nd.set_lazy_float16(True)
    print(f"# library {lib.target}; lazy mode, float16 loops {'recorded' if half else 'eager'}; {a.reps} repetitions of {a.calls} back-to-back calls; times in ms per call")
    print(f"# {'case':46s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>9s} {'GB/s, fused bytes':>18s}  C-ABI calls")
    for name, nbytes, fn in cases(np.random.default_rng(0)):
        if a.only and a.only not in name:
            continue
        if a.trace:
            for _ in range(a.calls):
                fn()
            lib.sync()
            print(f"  {name}: {a.calls} calls", flush=True)
            continue
        fn()
        seen = count_calls(lib, fn)
        ms = measure(lib, fn, a.reps, a.calls)
        med = float(np.median(ms))
        q1, q3 = np.percentile(ms, [25, 75])
        calls = ", ".join(f"{k} {v}" for k, v in sorted(seen.items()))
        print(f"  {name:46s} {med:9.4f} {ms.min():9.4f} {ms.max():9.4f} {q3 - q1:9.4f} {nbytes / med / 1e6:18.1f}  {calls}", flush=True)


if __name__ == "__main__":
    main()
