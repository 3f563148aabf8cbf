#!/usr/bin/env python3
"""Lazy mode: chains that read float16 / uint8 arrays and a chain stored as float16 — wall time per call over back-to-back calls
between two mdhip_sync, after a warm-up; median of the repetitions with the spread (min, max, interquartile range), the bytes per
second that ONE read of the chain's distinct operands plus one write of the result in that time amounts to (the fused byte count),
and the C-ABI compute calls one call makes (3 conversions / kernels on a build without the fused forms, 1 with them).
The method of scripts/bench_fused_rows.py. A call builds the chain and forces its result into memory, as the consumer of a mixed-
precision layer does. Run it on two builds of the library, alternated, to compare them.
usage: bench_fused_narrow.py [--reps 40] [--calls 20] [--only NAME] [--trace]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

f16, f32, f64 = np.float16, np.float32, np.float64


def cases(rng):
    """(name, fused bytes, call)"""
    out = []

    def f(dt, *s):
        return nd.asarray(rng.standard_normal(s).astype(dt))

    def scale_shift(R, Cc):
        x, w, b = f(f16, R, Cc), f(f32, R, Cc), f(f32, R, Cc)
        n = R * Cc
        return (f"astype(x16, f32) * w + b {R}x{Cc}", 14 * n,
                lambda: nd.materialize(nd.add(nd.multiply(nd.astype(x, f32), w), b)))

    def row_dot(R, Cc):
        x, y = f(f16, R, Cc), f(f32, R, Cc)
        n = R * Cc
        return (f"sum(astype(x16, f32) * y32, -1) {R}x{Cc}", 6 * n + 4 * R,
                lambda: nd.materialize(nd.sum(nd.multiply(nd.astype(x, f32), y), axis=-1)))

    def normalise(R, Cc):
        u, mean = nd.asarray(rng.integers(0, 256, (R, Cc)).astype(np.uint8)), f(f64, Cc)
        n = R * Cc
        return (f"u8 / 255.0 - mean(C,) {R}x{Cc}", 9 * n + 8 * Cc,
                lambda: nd.materialize(nd.subtract(nd.true_divide(u, 255.0), mean)))

    def half_store(R, Cc):
        x, w, b = f(f32, R, Cc), f(f32, R, Cc), f(f32, R, Cc)
        n = R * Cc
        return (f"astype(x32 * w32 + b32, f16) {R}x{Cc}", 14 * n,
                lambda: nd.materialize(nd.astype(nd.add(nd.multiply(x, w), b), f16)))

    for make in (scale_shift, row_dot, normalise, half_store):
        out.append(make(8192, 4096))
    out.append(scale_shift(256, 512))      # under 2^18 elements: the interpreter kernels, launch cost
    out.append(half_store(256, 512))
    return out


ENTRIES = ("binary", "unary", "convert", "reduce", "where", "vm_eval", "vm_reduce", "vm_eval_multi", "vm_eval_reduce_cols")


def count_calls(lib, fn):
    """C-ABI compute calls of one call of fn, by entry point"""
    seen, plain = {}, {}
    for name in ENTRIES:
        plain[name] = getattr(lib, name)

        def counting(*args, _n=name):
            try:
                return plain[_n](*args)
            finally:
                seen[_n] = seen.get(_n, 0) + 1
        setattr(lib, name, counting)
    try:
        fn()
        lib.sync()
    finally:
        for name in ENTRIES:
            setattr(lib, name, plain[name])
    return seen


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
