#!/usr/bin/env python3
"""A/B the thin and long-k float16 / int8 / uint8 products in ONE process: option gemm_narrow_skinny = 0 (the routes these products had:
convert + float32 streaming kernels, the generic narrow kernel, convert + long-k) against 1 (csrc/skinny.hip on the operands as they
are), alternating per shape, HIP-event timing, every shape warmed.

Per row: the median / min / max over ROUNDS timings of REPS calls each, for both options; `need` = the bytes the product needs (the big
operand once, the thin operand, the result) over the native median, as GB/s and as a share of 8 TB/s — the HBM bound, the one that
binds these products; `x` = option 0's median over option 1's. A row is marked SLOWER when option 1's median is above option 0's by
more than the larger of the two spreads (max - min). `native` = launches the counter gemm_narrow_thin_runs saw per call (0: the
planner declined, both columns time the same route).

Every timing walks COPIES distinct big operands (>= 512 MiB in all), so that no call finds its operand in the 256 MiB last-level
cache left there by the call before.

  python scripts/bench_narrow_thin.py [kind ...]          kinds: f16 f16->f32 i8 i8->i32 u8 (default: all)
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

KINDS = {"f16": (np.float16, None), "f16->f32": (np.float16, np.float32), "i8": (np.int8, None), "i8->i32": (np.int8, np.int32), "u8": (np.uint8, None)}
REPS = int(os.environ.get("THIN_REPS", "8"))
ROUNDS = int(os.environ.get("THIN_ROUNDS", "5"))
SCALE = int(os.environ.get("THIN_SCALE", "1"))          # divide every extent (a rehearsal on the CPU double)
FOOTPRINT = (512 << 20) // (SCALE * SCALE)
PEAK = 8e12


def data(rng, shape, dt):
    if dt == np.float16:
        return rng.standard_normal(shape, dtype=np.float32).astype(np.float16)
    lo, hi = (-128, 128) if dt == np.int8 else (0, 256)
    return rng.integers(lo, hi, shape, dtype=np.int16).astype(dt)


def clones(x, n):
    """x and n - 1 copies of it in memory of their own"""
    return [x] + [nd.copy(x) for _ in range(n - 1)]


def main():
    if os.environ.get("THIN_LIBRARY"):       # (a rehearsal on the CPU double: its path)
        _capi.use_library(os.environ["THIN_LIBRARY"])
    lib = _capi.load()
    nd.set_lazy(False)
    opt = lambda name, v: lib.debug_set_option(name.encode(), int(v))   # noqa: E731

    def runs():
        v = C.c_int64()
        lib.debug_get_option(b"gemm_narrow_thin_runs", C.byref(v))
        return v.value

    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
    ms = C.c_float()
    rng = np.random.default_rng(0)
    kinds = sys.argv[1:] or list(KINDS)
    print(f"# REPS {REPS} per timing, ROUNDS {ROUNDS}; us per call: median (min .. max)")
    print(f"# {'kind':9s} {'product':34s} {'lay':3s} {'native':6s} | {'option 0 us':>28s} | {'option 1 us':>28s} | {'need GB/s':>9s} {'of 8 TB/s':>9s} | {'x':>6s}")
    slower = 0
    for kind in kinds:
        dt, wide = KINDS[kind]
        esz, osz = np.dtype(dt).itemsize, np.dtype(wide or dt).itemsize
        mm = (lambda a, b: nd.matmul(a, b, dtype=wide)) if wide is not None else nd.matmul

        def measure(label, lay, calls, need):
            """calls: one (a, b) pair per copy of the big operand"""
            nonlocal slower
            res = {0: [], 1: []}
            native = 0
            for o in (0, 1):               # warm both routes on every copy
                opt("gemm_narrow_skinny", o)
                n0 = runs()
                for a, b in calls:
                    mm(a, b)
                if o:
                    native = (runs() - n0) // len(calls)
            for _ in range(ROUNDS):
                for o in (0, 1):
                    opt("gemm_narrow_skinny", o)
                    mm(*calls[-1])
                    lib.event_record(e0)
                    for r in range(REPS):
                        mm(*calls[r % len(calls)])
                    lib.event_record(e1)
                    lib.event_elapsed_ms(e0, e1, C.byref(ms))
                    res[o].append(ms.value * 1e3 / REPS)
            opt("gemm_narrow_skinny", 1)
            med = {o: sorted(v)[len(v) // 2] for o, v in res.items()}
            spread = max(max(v) - min(v) for v in res.values())
            flag = ""
            if native and med[1] > med[0] + spread:
                flag = "  SLOWER"
                slower += 1
            cols = " | ".join("%8.1f (%8.1f .. %8.1f)" % (med[o], min(res[o]), max(res[o])) for o in (0, 1))
            gbs = need / (med[1] * 1e-6) / 1e9
            print(f"  {kind:9s} {label:34s} {lay:3s} {native:6d} | {cols} | {gbs:9.0f} {100 * gbs * 1e9 / PEAK:8.1f}% | {med[0] / med[1]:6.2f}{flag}", flush=True)

        def copies(R, K):
            return max(1, -(-FOOTPRINT // (R * K * esz)))

        # a square matrix against a vector and 2 / 4 / 8 columns, the four layouts (N: C order, T: the transpose of a C-order array)
        for R in (8192 // SCALE, 4096 // SCALE):
            n = copies(R, R)
            As = clones(nd.asarray(data(rng, (R, R), dt)), n)
            for nc in (1, 2, 4, 8):
                B, Bt = nd.asarray(data(rng, (R, nc), dt)), nd.asarray(data(rng, (nc, R), dt))
                need = R * R * esz + R * nc * esz + R * nc * osz
                for lay, ta, b in (("NN", False, B), ("NT", False, Bt.T), ("TN", True, B), ("TT", True, Bt.T)):
                    measure(f"({R}, {R}) @ ({R}, {nc})", lay, [(a.T if ta else a, b) for a in As], need)
            del As
        # a few rows through a layer (thin M): weights (K, N) as they lie and as the transpose of (N, K)
        for K, N in ((16384 // SCALE, 4096 // SCALE), (4096 // SCALE, 16384 // SCALE)):
            n = copies(K, N)
            Ws, Wts = clones(nd.asarray(data(rng, (K, N), dt)), n), clones(nd.asarray(data(rng, (N, K), dt)), n)
            for m in (1, 8):
                x = nd.asarray(data(rng, (m, K), dt))
                need = K * N * esz + m * K * esz + m * N * osz
                measure(f"({m}, {K}) @ ({K}, {N})", "NN", [(x, w) for w in Ws], need)
                measure(f"({m}, {K}) @ ({K}, {N})", "NT", [(x, w.T) for w in Wts], need)
            del Ws, Wts
        # few outputs under a long k
        K = (4 << 20) // SCALE
        n = copies(1, 2 * K)
        vs = list(zip(clones(nd.asarray(data(rng, (K,), dt)), n), clones(nd.asarray(data(rng, (K,), dt)), n)))
        measure(f"dot({K}, {K})", "-", vs, 2 * K * esz + osz)
        del vs
        K = (1 << 20) // SCALE
        n = copies(32, K)
        ab = list(zip(clones(nd.asarray(data(rng, (16, K), dt)), n), clones(nd.asarray(data(rng, (K, 16), dt)), n)))
        measure(f"(16, {K}) @ ({K}, 16)", "NN", ab, 32 * K * esz + 256 * osz)
        del ab
        lib.empty_cache()
    print(f"# native-routed rows slower than option 0 beyond the spread: {slower}")


if __name__ == "__main__":
    main()
