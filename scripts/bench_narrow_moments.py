#!/usr/bin/env python3
"""std and mean of float16 / small-integer arrays, read in their own type against the promote route, in ONE process.

Two arms per case, alternated repetition by repetition:
  native   nd.std through mdhip_var on the narrow array (option var_narrow 1), nd.mean as one sum of the narrow array in NumPy's
           accumulator (narrow.NATIVE_STATS True);
  promote  the route of the parent commit: convert the array to float32 / float64, run the wide kernels, demote (option var_narrow 0
           and narrow.NATIVE_STATS False).
The method of scripts/bench_middle_axis.py: wall time per call over --calls back-to-back calls between two mdhip_sync, after a
warm-up, --reps (>= 30) repetitions; median, min, max, interquartile range; and the bytes per second that ONE read of the NARROW
array in the median time amounts to (the algorithmic minimum; the column forms read it twice). The verdict column says whether the
native arm is faster by more than the spread: the medians differ by more than the sum of the two interquartile ranges.
--before / --after FILE: the promote / native rows go to these files as well (profiles/narrow_moments_*.txt).
--trace: --calls native calls of each case and no timing — the run to put under a kernel trace.
usage: bench_narrow_moments.py [--reps 40] [--calls 20] [--dtypes float16,int8,..] [--before F] [--after F] [--trace]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, narrow, ndarray as nd  # noqa: E402

CASES = [((8192, 4096), -1), ((8192, 4096), 0), ((64, 512, 512), 1)]
DTYPES = ["float16", "int8", "uint8", "int16", "uint32"]


def arm(lib, native):
    """(On a build from before option var_narrow — the parent commit — both arms are that build's one route: the promote route.)"""
    try:
        lib.debug_set_option(b"var_narrow", 1 if native else 0)
    except ValueError:
        pass
    narrow.NATIVE_STATS = bool(native)


def measure_pair(lib, fn, reps, calls):
    """[native ms], [promote ms]: the arms alternate inside every repetition."""
    for native in (True, False):
        arm(lib, native)
        for _ in range(3):
            fn()
    lib.sync()
    ms = {True: [], False: []}
    for _ in range(reps):
        for native in (True, False):
            arm(lib, native)
            lib.sync()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            lib.sync()
            ms[native].append((time.perf_counter() - t0) * 1e3 / calls)
    arm(lib, True)
    return np.array(ms[True]), np.array(ms[False])


def row(tag, ms, nbytes):
    med = float(np.median(ms))
    q1, q3 = np.percentile(ms, [25, 75])
    return f"  {tag:44s} {med:9.4f} {ms.min():9.4f} {ms.max():9.4f} {q3 - q1:9.4f} {nbytes / med / 1e6:17.1f}", med, float(q3 - q1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--dtypes", default=",".join(DTYPES))
    ap.add_argument("--before", default=None)
    ap.add_argument("--after", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    if a.reps < 30 and not a.trace:
        ap.error("at least 30 repetitions")
    lib = _capi.load()
    nd.set_lazy(False)
    try:
        lib.debug_set_option(b"var_narrow", 1)
        known = True
    except ValueError:
        known = False
    head = [f"# library {lib.target}; option var_narrow known: {known}; {a.reps} repetitions of {a.calls} back-to-back calls, the two arms alternating; times in ms per call",
            f"# {'case':44s} {'median':>9s} {'min':>9s} {'max':>9s} {'iqr':>9s} {'GB/s, 1 narrow read':>17s}"]
    files = {False: open(a.before, "w") if a.before else None, True: open(a.after, "w") if a.after else None}
    for native, f in files.items():
        if f:
            f.write(f"# scripts/bench_narrow_moments.py, the {'native' if native else 'promote (parent commit)'} arm\n" + "\n".join(head) + "\n")
    print("\n".join(head))
    rng = np.random.default_rng(0)
    for name in a.dtypes.split(","):
        dt = np.dtype(name)
        for shape, axis in CASES:
            h = (rng.standard_normal(shape) * 3 + 10).astype(dt) if dt.kind == "f" else rng.integers(0, 100, shape).astype(dt)
            x = nd.asarray(h)
            nbytes = x.size * dt.itemsize
            for fname, fn in (("std", lambda: nd.std(x, axis=axis)), ("mean", lambda: nd.mean(x, axis=axis))):
                tag = f"{fname} {'x'.join(map(str, shape))} axis {axis} {dt.name}"
                if a.trace:
                    arm(lib, True)
                    for _ in range(a.calls):
                        fn()
                    lib.sync()
                    print(f"  {tag}: {a.calls} calls", flush=True)
                    continue
                new, old = measure_pair(lib, fn, a.reps, a.calls)
                r_new, m_new, s_new = row(tag + " [native]", new, nbytes)
                r_old, m_old, s_old = row(tag + " [promote]", old, nbytes)
                gain = m_old - m_new
                verdict = f"{m_old / m_new:5.2f}x, gain {gain:.4f} ms " + ("> " if gain > s_new + s_old else "NOT > ") + f"spread {s_new + s_old:.4f} ms"
                print(r_old + "\n" + r_new + "   " + verdict, flush=True)
                if files[False]:
                    files[False].write(r_old + "\n")
                if files[True]:
                    files[True].write(r_new + "   " + verdict + "\n")
            del x
    for f in files.values():
        if f:
            f.close()


if __name__ == "__main__":
    main()
