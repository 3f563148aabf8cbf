#!/usr/bin/env python3
"""float16 / int8 products: the native call (csrc/gemm_narrow.hip) against the route it replaced, written out —
astype(float32 | int64) -> matmul -> astype — in ONE process, interleaved rounds, HIP-event timing, random data.

    gemm_bench_narrow.py [MxKxN ...]     default: 4096^3, 2048^3, 8192x4096x4096 (M x K x N), layouts NN / NT / TN
    GEMM_DTYPES=float16,int8 (default both), GEMM_REPS, GEMM_ROUNDS
    GEMM_MODE=widen: the wide-output products instead — matmul(a, b, dtype=float32 | int32), one native call — against the route a
    caller had without the keyword, matmul(astype(a, wide), astype(b, wide)); the narrow-output native call for orientation;
    `spread` is (max - min) / median of the native rounds.
Prints per shape, dtype and layout the median / min / max time of both routes, the speed-up, and the native rate with its fraction
of the dense matrix-core peak (float16 2.5 PFLOP/s, int8 5.0 POPS: MI355X_MICROARCH.md, Matrix cores)."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

REPS = int(os.environ.get("GEMM_REPS", "5"))
ROUNDS = int(os.environ.get("GEMM_ROUNDS", "5"))
PEAK = {"float16": 2.5e15, "int8": 5.0e15}
WIDE = {"float16": np.float32, "int8": np.int64}
WIDE_OUT = {"float16": np.float32, "int8": np.int32}
MODE = os.environ.get("GEMM_MODE", "narrow")


def main():
    lib = _capi.load()
    shapes = [(4096, 4096, 4096), (2048, 2048, 2048), (8192, 4096, 4096)]
    if len(sys.argv) > 1:
        shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
    rng = np.random.default_rng(0)
    e0, e1 = C.c_void_p(), C.c_void_p()
    lib.event_create(C.byref(e0)); lib.event_create(C.byref(e1))
    ms = C.c_float()

    def timed(fn):
        fn()
        lib.event_record(e0)
        for _ in range(REPS):
            fn()
        lib.event_record(e1)
        lib.event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value * 1e3 / REPS   # us per call

    for (M, K, N) in shapes:
        for dname in os.environ.get("GEMM_DTYPES", "float16,int8").split(","):
            if dname == "float16":
                a = rng.standard_normal((M, K)).astype(np.float16)
                b = rng.standard_normal((K, N)).astype(np.float16)
            else:
                a = rng.integers(-128, 128, (M, K)).astype(np.int8)
                b = rng.integers(-128, 128, (K, N)).astype(np.int8)
            A, B = nd.asarray(a), nd.asarray(b)
            At, Bt = nd.asarray(np.ascontiguousarray(a.T)), nd.asarray(np.ascontiguousarray(b.T))
            combos = (("NN", A, B), ("NT", A, Bt.T), ("TN", At.T, B))
            wide = WIDE[dname]
            res = {}
            if MODE == "widen":
                widen_rounds(timed, M, K, N, dname, combos)
                continue
            for _ in range(4):
                nd.matmul(A, B)
            for rnd in range(ROUNDS):
                for tag, x, y in combos:
                    native = lambda: nd.matmul(x, y)                                                       # noqa: E731
                    promote = lambda: nd.astype(nd.matmul(nd.astype(x, wide), nd.astype(y, wide)), x.dtype)   # noqa: E731
                    res.setdefault((tag, "native"), []).append(timed(native))
                    res.setdefault((tag, "promote"), []).append(timed(promote))
                    if rnd == 0:
                        assert np.array_equal(native().get(), promote().get()) if dname == "int8" else True, tag
            print(f"M={M} K={K} N={N} {dname}")
            for tag, _, _ in combos:
                nat, pro = sorted(res[(tag, "native")]), sorted(res[(tag, "promote")])
                mn, mp = nat[len(nat) // 2], pro[len(pro) // 2]
                rate = 2.0 * M * N * K / (mn * 1e-6)
                print(f"   {tag}  native med {mn:8.1f} min {nat[0]:8.1f} max {nat[-1]:8.1f} us   promote med {mp:8.1f} min {pro[0]:8.1f} "
                      f"max {pro[-1]:8.1f} us   x{mp / mn:5.2f}   {rate / 1e12:7.1f} T{'FLOP' if dname == 'float16' else 'OP'}/s = "
                      f"{100 * rate / PEAK[dname]:4.1f} % of peak", flush=True)


def widen_rounds(timed, M, K, N, dname, combos):
    wide = WIDE_OUT[dname]
    res = {}
    for _ in range(4):
        nd.matmul(combos[0][1], combos[0][2], dtype=wide)
    for rnd in range(ROUNDS):
        for tag, x, y in combos:
            native = lambda: nd.matmul(x, y, dtype=wide)                              # noqa: E731
            convert = lambda: nd.matmul(nd.astype(x, wide), nd.astype(y, wide))       # noqa: E731
            narrow = lambda: nd.matmul(x, y)                                          # noqa: E731
            for name, fn in (("native", native), ("convert", convert), ("narrow", narrow)):
                res.setdefault((tag, name), []).append(timed(fn))
            if rnd == 0 and dname == "int8":
                assert np.array_equal(native().get(), convert().get()), tag
    print(f"M={M} K={K} N={N} {dname} -> {np.dtype(wide).name}")
    for tag, _, _ in combos:
        nat, con, nar = (sorted(res[(tag, k)]) for k in ("native", "convert", "narrow"))
        mn, mc, mr = nat[len(nat) // 2], con[len(con) // 2], nar[len(nar) // 2]
        rate = 2.0 * M * N * K / (mn * 1e-6)
        print(f"   {tag}  native med {mn:8.1f} min {nat[0]:8.1f} max {nat[-1]:8.1f} us (spread {(nat[-1] - nat[0]) / mn:5.1%})   convert med {mc:8.1f} "
              f"min {con[0]:8.1f} max {con[-1]:8.1f} us   x{mc / mn:5.2f}   narrow-output med {mr:8.1f} us   {rate / 1e12:7.1f} "
              f"T{'FLOP' if dname == 'float16' else 'OP'}/s = {100 * rate / PEAK[dname]:4.1f} % of peak", flush=True)


if __name__ == "__main__":
    main()
