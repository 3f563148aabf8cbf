#!/usr/bin/env python3
"""astype, narrow copies and `where` on storage-only branches: the 16-byte vector kernels of csrc/narrow.hip against the one-element
kernels they stand in front of, in ONE process.

Two arms per case, alternated repetition by repetition:
  arm 1   options convert_vec / where_vec 1: k_nw_convert, k_nw_convert_axes, k_nw_where, k_nw_where_axes;
  arm 0   options 0: k_convert / k_nw_where_generic for everything — the route of the parent commit. (On a build from before the
          options both arms are that build's one route: run the script on it, MDHIP_LIB_VARIANT=.., to see that it times as arm 0.)
The method of scripts/bench_narrow_moments.py: wall time per call over --calls back-to-back calls between two mdhip_sync, after a
warm-up, --reps (>= 30) repetitions; median, min, max, interquartile range; TB/s = the algorithmic bytes (one read of every array
operand in its type + one write of the result in its type) over the median. `vec`: launches of a vector kernel the counters saw per
call. The verdict says whether arm 1 beats arm 0 by more than the larger of the two spreads (interquartile ranges).
--before / --after FILE: the arm 0 / arm 1 rows go to these files as well (profiles/convert_where_*.txt).
--trace: --calls arm-1 calls of each case and no timing — the run to put under a kernel trace.
usage: bench_convert_where.py [--reps 40] [--calls 20] [--before F] [--after F] [--trace]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402

OPTIONS = (b"convert_vec", b"where_vec")
COUNTERS = (b"convert_vec_runs", b"where_vec_runs")


def arm(lib, on):
    for name in OPTIONS:
        try:
            lib.debug_set_option(name, 1 if on else 0)
        except ValueError:
            pass


def vec_runs(lib):
    total = 0
    for name in COUNTERS:
        v = C.c_int64()
        try:
            lib.debug_get_option(name, C.byref(v))
            total += v.value
        except ValueError:
            pass
    return total


def measure_pair(lib, fn, reps, calls):
    for on in (True, False):
        arm(lib, on)
        for _ in range(3):
            fn()
    lib.sync()
    ms = {True: [], False: []}
    for _ in range(reps):
        for on in (True, False):
            arm(lib, on)
            lib.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            lib.sync()
            ms[on].append((time.perf_counter() - t0) * 1e3 / calls)
    arm(lib, True)
    return np.array(ms[True]), np.array(ms[False])


def row(tag, ms, nbytes, vec):
    med = float(np.median(ms))
    q1, q3 = np.percentile(ms, [25, 75])
    return f"  {tag:58s} {med:9.4f} {ms.min():9.4f} {ms.max():9.4f} {q3 - q1:9.4f} {nbytes / med / 1e9:8.3f} {vec:4d}", med, float(q3 - q1)


def cases(rng):
    """(tag, call, algorithmic bytes)"""
    R, Cn = 8192, 4096
    n = R * Cn
    x32 = nd.asarray(rng.standard_normal((R, Cn)).astype(np.float32) * 50)
    x16 = nd.asarray(rng.standard_normal((R, Cn)).astype(np.float16))
    xu8 = nd.asarray(rng.integers(0, 256, (R, Cn)).astype(np.uint8))
    xi8 = nd.asarray(rng.integers(-128, 128, (R, Cn)).astype(np.int8))
    yi8 = nd.asarray(rng.integers(-128, 128, (R, Cn)).astype(np.int8))
    y16 = nd.asarray(rng.standard_normal((R, Cn)).astype(np.float16))
    mask = nd.asarray(rng.random((R, Cn)) < 0.5)
    out = [("astype 8192x4096 float32 -> float16", lambda: x32.astype(np.float16), n * 6),
           ("astype 8192x4096 float16 -> float32", lambda: x16.astype(np.float32), n * 6),
           ("astype 8192x4096 uint8 -> float32", lambda: xu8.astype(np.float32), n * 5),
           ("astype 8192x4096 float32 -> int8", lambda: x32.astype(np.int8), n * 5),
           ("copy 8192x4096 float16", lambda: nd.copy(x16), n * 4),
           ("astype x16[:, :4032] -> float32", lambda: x16[:, :4032].astype(np.float32), R * 4032 * 6),
           ("copy x16[:, :4032]", lambda: nd.copy(x16[:, :4032]), R * 4032 * 4),
           ("where(mask, x16, 0) 8192x4096", lambda: nd.where(mask, x16, 0), n * 5),
           ("where(mask, x16, y16) 8192x4096", lambda: nd.where(mask, x16, y16), n * 7),
           ("where(mask, xi8, 0) 8192x4096", lambda: nd.where(mask, xi8, 0), n * 3),
           ("where(mask, xi8, yi8) 8192x4096", lambda: nd.where(mask, xi8, yi8), n * 4)]
    B, R3, C3 = 64, 512, 512
    m3 = nd.asarray(rng.random((B, R3, C3)) < 0.5)
    a3 = nd.asarray(rng.standard_normal((B, R3, C3)).astype(np.float16))
    b3 = nd.asarray(rng.standard_normal((B, 1, C3)).astype(np.float16))
    out.append(("where(m, a16, b16 (64, 1, 512)) 64x512x512", lambda: nd.where(m3, a3, b3), B * R3 * C3 * 5 + B * C3 * 2))
    a4 = nd.asarray(rng.standard_normal((4096, 4096)).astype(np.float32))
    b4 = nd.asarray(rng.standard_normal((4096, 4096)).astype(np.float32))
    out.append(("matmul(a32.astype(f16), b32.astype(f16)) 4096^2 (end to end)", lambda: nd.matmul(a4.astype(np.float16), b4.astype(np.float16)),
                2 * 4096 * 4096 * 6 + 3 * 4096 * 4096 * 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--before", default=None)
    ap.add_argument("--after", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.reps < 30 and not a.trace:
        ap.error("at least 30 repetitions")
    lib = _capi.load()
    nd.set_lazy(False)
    try:
        lib.debug_set_option(b"convert_vec", 1)
        known = True
    except ValueError:
        known = False
    head = [f"# library {lib.target}; options convert_vec / where_vec known: {known}; {a.reps} repetitions of {a.calls} back-to-back calls, the two arms alternating; "
            "times in ms per call", f"# {'case':58s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>9s} {'TB/s':>8s} {'vec':>4s}"]
    files = {False: open(a.before, "w") if a.before else None, True: open(a.after, "w") if a.after else None}
    for on, f in files.items():
        if f:
            f.write(f"# scripts/bench_convert_where.py, arm {int(on)} ({'vector kernels' if on else 'one-element kernels: the parent commit'})\n" + "\n".join(head) + "\n")
    print("\n".join(head))
    for tag, fn, nbytes in cases(np.random.default_rng(0)):
        if a.trace:
            arm(lib, True)
            for _ in range(a.calls):
                fn()
            lib.sync()
            print(f"  {tag}: {a.calls} calls", flush=True)
            continue
        vec = {}
        for on in (True, False):
            arm(lib, on)
            n0 = vec_runs(lib)
            fn()
            vec[on] = vec_runs(lib) - n0
        new, old = measure_pair(lib, fn, a.reps, a.calls)
        r_new, m_new, s_new = row(tag + " [1]", new, nbytes, vec[True])
        r_old, m_old, s_old = row(tag + " [0]", old, nbytes, vec[False])
        gain, spread = m_old - m_new, max(s_new, s_old)
        verdict = f"{m_old / m_new:5.2f}x, gain {gain:.4f} ms " + ("> " if gain > spread else "NOT > ") + f"spread {spread:.4f} ms"
        print(r_old + "\n" + r_new + "   " + verdict, flush=True)
        if files[False]:
            files[False].write(r_old + "\n")
        if files[True]:
            files[True].write(r_new + "   " + verdict + "\n")
    for f in files.values():
        if f:
            f.close()


if __name__ == "__main__":
    main()
