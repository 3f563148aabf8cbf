#!/usr/bin/env python3
"""Host time per call of three lazy-mode calls whose device side is small, so that the launch planner of fusion.hip (it runs on
every call) shows if it got dearer: a small fused evaluation (interpreter kernel), and a fused full sum and a fused row sum just
above jit_min (generated kernels). The method of scripts/host_overhead.py `calls`: a warm-up, then bursts of back-to-back calls,
each burst started on an idle stream; microseconds per call, median and minimum over the bursts. Run it on two builds of the
library, alternated, a fresh process each. MDHIP_LIB_VARIANT=NAME selects the other build here: this script opens the library
through _capi.load() alone, so the process binds one library. (Under pytest that does not hold — the fixtures open the product
file by path — which is why profiles/fused_plan_trace.txt put the parent build in the product file's place instead.)
usage: fused_plan_host.py LABEL [--bursts 60] [--calls 100]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from minidiff_amd import _capi, ndarray as nd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("label")
    ap.add_argument("--bursts", type=int, default=60)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    lib = _capi.load()
    nd.set_lazy(True)
    rng = np.random.default_rng(0)
    s0, s1 = (nd.asarray(rng.standard_normal(8).astype(np.float32)) for _ in range(2))
    x, y = (nd.asarray(rng.standard_normal((512, 520)).astype(np.float32)) for _ in range(2))   # 266240 elements: just above jit_min = 2^18
    cases = (("eval sin(a)*b, (8,) f32", "vm_eval", lambda: nd.materialize(nd.multiply(nd.sin(s0), s1))),
             ("sum(x*y), (512, 520) f32", "vm_reduce", lambda: nd.sum(nd.multiply(x, y))),
             ("sum(x*y, axis=-1), (512, 520) f32", "vm_reduce_rows", lambda: nd.sum(nd.multiply(x, y), axis=-1)))
    for name, counter, f in cases:
        before = nd.FUSION_STATS[counter]
        f()
        fused = nd.FUSION_STATS[counter] - before
        for _ in range(1000):
            f()
        us = []
        for _ in range(a.bursts):
            lib.sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                f()
            us.append((time.perf_counter() - t0) / a.calls * 1e6)
        lib.sync()
        us.sort()
        print("%-8s%-36s median %6.2f us  min %6.2f us  (%d bursts of %d calls; fused calls per call: %d)"
              % (a.label, name, us[len(us) // 2], us[0], a.bursts, a.calls, fused), flush=True)


if __name__ == "__main__":
    main()
