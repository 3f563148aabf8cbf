#!/usr/bin/env python3
"""What the matmul precision switch buys: the three modes and the fp32 plan, interleaved in ONE process.

  python scripts/bench_matmul_precision.py [--batches 20] [--reps 10] [--shapes MxKxN,..] [--out profiles/matmul_precision.txt] [--trace]

Arms: fp32 (option gemm_bf16x3 = 0: the MFMA fma chain), highest / high / medium (ndarray.set_matmul_precision) with the bf16
route FORCED (gemm_bf16x3 = 2) so that every shape is measured on the route whatever the floors are: the floors are what this
table sets. Per shape and batch every arm runs `reps` back-to-back products between two device events (the whole call: flag word,
split passes, product, the stand-in's empty launch), the arms in turn, batch after batch; then one more product per arm whose
main kernel carries the events itself (mdhip_event_attach_next): the product kernel alone. Call minus kernel is what the split
passes and the small launches cost. Reported: median and min - max over the batches, us per product.
Then the cfg2-shaped figure: passes/s of a 4096^2 forward + backward sweep (three products, workloads.make_cfg2) per mode with
the options at their DEFAULTS, i.e. with the floors as built. --shapes: these NN products instead of the list below, no sweep
(the shapes around a floor).
--trace: a short run of every arm and nothing else, for `rocprofv3 --kernel-trace --stats -- python scripts/bench_matmul_precision.py --trace`.
No GPU: an error, not a fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (M, K, N, layout, label)
SHAPES = [
    (4096, 4096, 4096, "NN", "4096^3"), (4096, 4096, 4096, "NT", "4096^3"), (4096, 4096, 4096, "TN", "4096^3"),
    (2048, 2048, 2048, "NN", "2048^3"), (8192, 4096, 4096, "NN", "8192 x 4096 x 4096"), (1024, 1024, 1024, "NN", "1024^3"),
    (1024, 4096, 4096, "NN", "1024-row panel of 4096^2"), (512, 4096, 4096, "NN", "512-row panel of 4096^2"),
]
ARMS = [("fp32", 0, "highest"), ("highest", 2, "highest"), ("high", 2, "high"), ("medium", 2, "medium")]
# MFMA floor of a mode: products x the bf16 instruction's time. DESIGN.md 4.4: 1.54 us per k-tile and CU for six products of a
# 256 x 128 x 32 tile (48 MFMAs of 16 passes per wave, two waves per SIMD, at an ASSUMED 2.0 GHz clock); one tile per CU and round.
FLOOR_US_PER_KTILE = {"highest": 1.54, "high": 1.54 / 2, "medium": 1.54 / 6}
CUS = 256


def floor_us(mode, M, K, N):
    rounds = -(-((M // 256) * (N // 128)) // CUS)
    return rounds * (K // 32) * FLOOR_US_PER_KTILE[mode]


def finish(args, lines):
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    from minidiff_amd import _capi, ndarray as nd
    lib = _capi.load()
    if lib.target != _capi.PRODUCT_TARGET:
        raise SystemExit("bench_matmul_precision: needs the HIP library on a gfx950 device")
    nd.set_lazy(False)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def event():
        e = C.c_void_p()
        lib.event_create(C.byref(e))
        return e

    def elapsed_us(e0, e1):
        ms = C.c_float()
        lib.event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value * 1e3

    def arm(force, mode):
        lib.debug_set_option(b"gemm_bf16x3", force)
        nd.set_matmul_precision(mode)

    def runs():
        v = C.c_int64()
        lib.debug_get_option(b"gemm_bf16x3_runs", C.byref(v))
        return v.value

    rng = np.random.default_rng(0)
    e0, e1 = event(), event()
    if args.trace:
        for (M, K, N, lay, label) in SHAPES[:3]:
            A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
            a = nd.asarray(np.ascontiguousarray(A.T)).T if lay[0] == "T" else nd.asarray(A)
            b = nd.asarray(np.ascontiguousarray(B.T)).T if lay[1] == "T" else nd.asarray(B)
            for _ in range(10):
                for name, force, mode in ARMS:
                    arm(force, mode)
                    nd.matmul(a, b)
            lib.sync()
        return
    say(f"# us per product, median (min - max) of {args.batches} batches of {args.reps} back-to-back products, the four arms interleaved in one process.")
    say("# call: device events around the batch (flag word, split passes, product, stand-in launch); kernel: the product kernel's own")
    say("# events, one launch per batch; passes: call - kernel. floor: products x the bf16 MFMA time of the tiles (assumed 2.0 GHz).")
    shapes = SHAPES
    if args.shapes:
        shapes = [tuple(int(v) for v in s.split("x")) + ("NN", s) for s in args.shapes.split(",")]
    for (M, K, N, lay, label) in shapes:
        A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
        a = nd.asarray(np.ascontiguousarray(A.T)).T if lay[0] == "T" else nd.asarray(A)
        b = nd.asarray(np.ascontiguousarray(B.T)).T if lay[1] == "T" else nd.asarray(B)
        ref = A.astype(np.float64) @ B if M * N * K <= 2048 ** 3 else None
        call = {n: [] for n, _, _ in ARMS}
        kern = {n: [] for n, _, _ in ARMS}
        for name, force, mode in ARMS:   # warm every arm (code objects, the allocator's blocks), check the route and the result
            arm(force, mode)
            r0 = runs()
            out = nd.matmul(a, b)
            assert runs() - r0 == (1 if force else 0), (label, name)
            if ref is not None:
                err = float(np.linalg.norm(out.get() - ref) / np.linalg.norm(ref))
                assert err < {"fp32": 3e-6, "highest": 3e-6, "high": 3e-5, "medium": 1e-2}[name], (label, name, err)
            for _ in range(30):
                nd.matmul(a, b)
        lib.sync()
        for _ in range(args.batches):
            for name, force, mode in ARMS:
                arm(force, mode)
                lib.event_record(e0)
                for _ in range(args.reps):
                    nd.matmul(a, b)
                lib.event_record(e1)
                call[name].append(elapsed_us(e0, e1) / args.reps)
                k0, k1 = event(), event()
                lib.event_attach_next(k0, k1)
                nd.matmul(a, b)
                left = C.c_int(0)
                lib.event_attach_cancel(C.byref(left))
                assert not left.value
                lib.sync()
                kern[name].append(elapsed_us(k0, k1))
                lib.event_destroy(k0); lib.event_destroy(k1)
        say(f"{label} {lay} (M {M} K {K} N {N})")
        for name, force, mode in ARMS:
            c, k = call[name], kern[name]
            fl = f"  floor {floor_us(mode, M, K, N):7.1f}" if force else ""
            say(f"   {name:8s} call {statistics.median(c):8.1f} ({min(c):8.1f} - {max(c):8.1f})   kernel {statistics.median(k):8.1f} ({min(k):8.1f} - {max(k):8.1f})"
                f"   passes {statistics.median(c) - statistics.median(k):7.1f}{fl}")
    if args.shapes:
        return finish(args, lines)
    # the cfg2-shaped sweep with the options at their defaults
    from minidiff_amd import workloads
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    md = build_engine(HipBackendTable, "bench")
    _, step = workloads.make_cfg2(md, n=4096)
    say("cfg2-shaped sweep (C = A @ B at 4096^2, C.backward(): three products), options at their defaults: passes/s, median (min - max)")
    sweep = {m: [] for m in ("highest", "high", "medium")}
    lib.debug_set_option(b"gemm_bf16x3", 1)
    for mode in sweep:
        nd.set_matmul_precision(mode)
        for _ in range(5):
            step()
    lib.sync()
    for _ in range(args.batches):
        for mode in sweep:
            nd.set_matmul_precision(mode)
            lib.event_record(e0)
            for _ in range(args.reps):
                step()
            lib.event_record(e1)
            sweep[mode].append(args.reps / (elapsed_us(e0, e1) * 1e-6))
    for mode, v in sweep.items():
        say(f"   {mode:8s} {statistics.median(v):8.1f} ({min(v):8.1f} - {max(v):8.1f})")
    nd.set_matmul_precision("highest")
    finish(args, lines)


if __name__ == "__main__":
    main()
