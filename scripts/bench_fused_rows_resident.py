#!/usr/bin/env python3
"""Lazy mode: chains that continue past a row reduction, with MDHIP_LAZY_ROWS (ndarray.set_lazy_rows) off and on in ONE process.

  python scripts/bench_fused_rows_resident.py [--batches 20] [--reps 10] [--out-prefix profiles/fused_resident] [--trace]
  python scripts/bench_fused_rows_resident.py --long [--out-prefix profiles/fused_resident_long]

Cases (float32): softmax forward and the softmax gradient p * (g - sum(g * p)) on (8192, 2048) and (65536, 256), a mean / variance
layer norm with (C,) gamma and beta on (16384, 1024). A call builds the chain and forces its result into memory.
Per case and batch each arm — switch off, switch on, in turn — runs `reps` back-to-back calls between two device events: the whole
call, every launch it makes and the gaps between them, us per call. Then one more call of the switch-on arm whose staged kernel
carries the events itself (mdhip_event_attach_next): the kernel alone. Reported: median and min - max over the batches, the bytes
per second that ONE read of the distinct operands and one write of the result in the call's time amount to, the launches of generated
kernels per call, and on / off. <prefix>_before.txt gets the switch-off lines, <prefix>_after.txt the switch-on lines.
--trace: a few calls of every arm and nothing else, for
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_fused_rows_resident.py --trace
(the staged kernels are named k_fused_rowsres<NV>_.., the composed route's k_fused_redrowsw<NV>_.. and k_fused_eval_..).
--long: the long rows instead (float32): layer norm on (8192, 4096) and (4096, 8192), softmax and the softmax gradient on
(8192, 4096). The switch is on in both arms; they differ in ndarray.set_lazy_rows_max: 2048 (`_before`: such rows are not recorded,
the composed route) against 8192 (`_after`: a block per row, k_fused_rowsresb<G>_..). Same method, same columns.
No GPU: an error, not a fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from minidiff_amd import _capi, ndarray as nd  # noqa: E402


def softmax(x):
    m = nd.max(x, axis=-1, keepdims=True)
    e = nd.exp(nd.subtract(x, m))
    return nd.true_divide(e, nd.sum(e, axis=-1, keepdims=True))


def softmax_grad(p, g):
    return nd.multiply(p, nd.subtract(g, nd.sum(nd.multiply(g, p), axis=-1, keepdims=True)))


def layer_norm(x, gamma, beta):
    d = nd.subtract(x, nd.mean(x, axis=-1, keepdims=True))
    v = nd.mean(nd.multiply(d, d), axis=-1, keepdims=True)
    return nd.add(nd.multiply(nd.true_divide(d, nd.sqrt(nd.add(v, 1e-5))), gamma), beta)


def cases(rng, long_rows):
    """(name, fused bytes, call)"""
    def f(*s):
        return nd.asarray(rng.standard_normal(s).astype(np.float32))

    out = []
    if long_rows:
        for R, Cn in ((8192, 4096), (4096, 8192)):
            x, gamma, beta = f(R, Cn), f(Cn), f(Cn)
            out.append((f"layer norm {R}x{Cn}", 2 * R * Cn * 4 + 8 * Cn, lambda x=x, gamma=gamma, beta=beta: nd.materialize(layer_norm(x, gamma, beta))))
        R, Cn = 8192, 4096
        x, g = f(R, Cn), f(R, Cn)
        prev = nd.set_lazy_rows(False)
        p = nd.materialize(softmax(x))
        nd.set_lazy_rows(prev)
        n = R * Cn * 4
        out.append((f"softmax {R}x{Cn}", 2 * n, lambda: nd.materialize(softmax(x))))
        out.append((f"softmax gradient {R}x{Cn}", 3 * n, lambda: nd.materialize(softmax_grad(p, g))))
        return out
    for R, Cn in ((8192, 2048), (65536, 256)):
        x, g = f(R, Cn), f(R, Cn)
        prev = nd.set_lazy_rows(False)
        p = nd.materialize(softmax(x))
        nd.set_lazy_rows(prev)
        n = R * Cn * 4
        out.append((f"softmax {R}x{Cn}", 2 * n, lambda x=x: nd.materialize(softmax(x))))
        out.append((f"softmax gradient {R}x{Cn}", 3 * n, lambda p=p, g=g: nd.materialize(softmax_grad(p, g))))
    R, Cn = 16384, 1024
    x, gamma, beta = f(R, Cn), f(Cn), f(Cn)
    out.append((f"layer norm {R}x{Cn}", 2 * R * Cn * 4 + 8 * Cn, lambda: nd.materialize(layer_norm(x, gamma, beta))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out-prefix", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--long", action="store_true", help="rows of 4096 / 8192: set_lazy_rows_max 2048 against 8192, the switch on")
    a = ap.parse_args()
    lib = _capi.load()
    nd.set_lazy(True)
    before, after = [], []

    def arm(flag):
        if a.long:
            nd.set_lazy_rows(True)
            nd.set_lazy_rows_max(8192 if flag else 2048)
        else:
            nd.set_lazy_rows(flag)

    def say(lines, text):
        print(text, flush=True)
        lines.append(text)

    def event():
        e = C.c_void_p()
        lib.event_create(C.byref(e))
        return e

    def elapsed_us(e0, e1):
        ms = C.c_float()
        lib.event_elapsed_ms(e0, e1, C.byref(ms))
        return ms.value * 1e3

    def launched():
        st = (C.c_int64 * 2)()
        lib.vm_jit_stats(st)
        return int(st[1])

    names = ("on, MDHIP_LAZY_ROWS_MAX 2048", "on, MDHIP_LAZY_ROWS_MAX 8192") if a.long else ("off", "on")
    head = f"# library {lib.target}; lazy mode, MDHIP_LAZY_ROWS %s; {a.batches} batches of {a.reps} back-to-back calls, the two arms in turn; us per call"
    cols = f"# {'case':32s} {'call: median (min - max)':>32s} {'GB/s, fused bytes':>18s} {'generated launches':>19s}"
    say(before, head % names[0])
    say(before, cols)
    say(after, head % names[1])
    say(after, cols + "   staged kernel alone: median (min - max)   " + ("8192 / 2048" if a.long else "on / off"))
    e0, e1 = event(), event()
    for name, nbytes, fn in cases(np.random.default_rng(0), a.long):
        if a.trace:
            for flag in (False, True):
                arm(flag)
                for _ in range(5):
                    fn()
            lib.sync()
            print(f"  {name}: 5 calls per arm", flush=True)
            continue
        call, launches, kern, vals = {False: [], True: []}, {}, [], {}
        for flag in (False, True):      # warm both arms (code objects, the allocator's blocks); results agree
            arm(flag)
            l0, r0 = launched(), nd.FUSION_STATS["vm_eval_rows"]
            vals[flag] = fn().get()
            launches[flag] = launched() - l0
            assert nd.FUSION_STATS["vm_eval_rows"] - r0 == (1 if flag else 0), (name, flag)
            for _ in range(10):
                fn()
        scale = float(np.abs(vals[False]).max())
        assert float(np.abs(vals[True] - vals[False]).max()) <= 1e-5 * scale, name
        lib.sync()
        for _ in range(a.batches):
            for flag in (False, True):
                arm(flag)
                lib.event_record(e0)
                for _ in range(a.reps):
                    fn()
                lib.event_record(e1)
                call[flag].append(elapsed_us(e0, e1) / a.reps)
            k0, k1 = event(), event()
            lib.event_attach_next(k0, k1)
            fn()
            left = C.c_int(0)
            lib.event_attach_cancel(C.byref(left))
            assert not left.value
            lib.sync()
            kern.append(elapsed_us(k0, k1))
            lib.event_destroy(k0)
            lib.event_destroy(k1)
        for flag, lines in ((False, before), (True, after)):
            c = call[flag]
            med = statistics.median(c)
            text = f"  {name:32s} {med:12.1f} ({min(c):8.1f} - {max(c):8.1f}) {nbytes / med / 1e3:18.1f} {launches[flag]:19d}"
            if flag:
                text += f"   {statistics.median(kern):12.1f} ({min(kern):8.1f} - {max(kern):8.1f})   {med / statistics.median(call[False]):6.3f}"
            say(lines, text)
    if a.out_prefix and not a.trace:
        for suffix, lines in (("_before.txt", before), ("_after.txt", after)):
            os.makedirs(os.path.dirname(os.path.abspath(a.out_prefix)), exist_ok=True)
            with open(a.out_prefix + suffix, "w") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
