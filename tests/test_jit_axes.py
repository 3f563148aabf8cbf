"""Fused chains whose iteration space keeps three or four axes — `(x * g[:, None, :] + h[None, :, None]) ** 2`, the broadcasts of a
normalisation layer — as kernels generated at run time (csrc/fusion_jit.inc, the axes form of EVAL; k_vm_eval_axes is the
interpreter's counterpart and the fallback).

A. compile-only (no device): probe kind 5 turns every operator, every leaf read mode, both output types, three and four axes
   and up to 8 leaves into source that hiprtc compiles for gfx950; the multi-output probe takes the axes form by itself when
   the merged leaves keep three axes.
B. on the device: the generated kernel gives the bits of the interpreter and of the eager calls (same functors, nothing
   contracted: DESIGN.md §9), and it is the generated kernel that ran (mdhip_vm_jit_stats counts one launch per evaluation).
   Shapes sit at the smallest the axes geometry takes (65536 elements, inner extent a multiple of 4)."""
import ctypes as C
import os

import numpy as np
import pytest

from minidiff_amd import _capi

gpu = pytest.mark.gpu

UNARY = ["absolute", "sign", "ceil", "floor", "sin", "cos", "tan", "sinh", "cosh", "tanh", "exp", "log", "sqrt", "logical_not",
         "negative", "isnan"]
BINARY = ["add", "subtract", "multiply", "true_divide", "power", "mod", "floor_divide", "maximum", "minimum", "less", "less_equal",
          "greater", "greater_equal", "equal", "not_equal", "logical_and", "logical_or", "logical_xor"]
KIND_AXES = 5


@pytest.fixture(scope="module")
def product():
    if not os.path.exists(_capi.PRODUCT_LIB):
        pytest.skip("libmdhip.so not built")
    lib = _capi.Library(_capi.PRODUCT_LIB)  # dlopen only; the compile-only probe needs no GPU
    return lib, C.create_string_buffer(4096)


# ------------------------------------------------------------------------------------------------------------ A. compile only
def _built(arrs):
    from minidiff_amd import lazy as lz
    out = []
    for name, arr in arrs:
        assert arr._expr is not None, name
        prog, keep = lz.build_program(arr._expr, arr.shape)
        out.append((name, prog, keep, arr.dtype == np.bool_))
    return out


def _three_axis_programs(nd):
    """(B,R,C) . (B,1,C): the sizes do not matter to the probe, the descriptors do"""
    rng = np.random.default_rng(0)
    f32 = lambda *s: nd.asarray(rng.standard_normal(s).astype(np.float32))   # noqa: E731
    x, y, g, h = f32(2, 3, 8), f32(2, 3, 8), f32(2, 1, 8), f32(1, 3, 1)
    m = nd.asarray(rng.integers(0, 2, (2, 1, 8)).astype(bool))
    progs = []
    for name in UNARY:
        progs.append((name, getattr(nd, name)(nd.multiply(x, g))))
    for name in BINARY:
        progs.append((name, getattr(nd, name)(nd.add(x, g), y)))
        progs.append((name + "/const-left", getattr(nd, name)(2.0, nd.sin(nd.multiply(x, g)))))
    progs.append(("where", nd.where(nd.greater(nd.multiply(x, g), 0), nd.multiply(x, m), 0.25)))
    xd = nd.asarray(rng.standard_normal((2, 3, 8)))
    gi = nd.asarray(rng.integers(-3, 3, (2, 1, 8)))
    progs.append(("f64 + int64 leaf", nd.add(nd.exp(xd), gi)))
    progs.append(("bool result", nd.logical_and(nd.greater(nd.multiply(x, g), h), m)))
    x4, g4 = f32(2, 3, 2, 8), f32(1, 3, 1, 8)
    progs.append(("four axes", nd.power(nd.add(nd.multiply(x4, g4), 1.5), 2)))
    progs.append(("four axes, bool", nd.greater(nd.multiply(x4, g4), 0)))
    # every read mode with the hoisted sin / cos on each: unit stride (x, g), inner stride 0 with outer strides (h), one device
    # element behind a stride-0 view (seed)
    seed = nd.broadcast_to(nd.asarray(np.float32(0.5)), (2, 3, 8))
    progs.append(("leaf modes", nd.add(nd.add(nd.multiply(nd.sin(x), nd.cos(x)), nd.multiply(nd.sin(g), nd.cos(h))),
                                       nd.multiply(nd.multiply(nd.sin(seed), nd.cos(seed)), nd.sin(h)))))
    ls = [f32(2, 3, 8), f32(2, 1, 8), f32(1, 3, 1), f32(1, 1, 8), f32(2, 3, 1), f32(2, 1, 1), f32(1, 3, 8), f32(2, 3, 8)]
    acc = ls[0]
    for leaf in ls[1:]:
        acc = nd.add(nd.multiply(acc, 0.5), leaf)
    progs.append(("8 leaves", acc))
    return _built(progs)


def test_axes_kernels_compile(lib, on_gpu, product):
    """Probe kind 5: every unary and binary operator, where, a float64 program with an int64 leaf, bool results, four axes, every
    leaf read mode with hoisted sin / cos, 8 leaves — each compiles for gfx950. (The kind is new: its refusal is a ValueError.)"""
    from minidiff_amd import ndarray as nd
    plib, log = product
    prev = nd.set_lazy(True)
    try:
        progs = _three_axis_programs(nd)
    finally:
        nd.set_lazy(prev)
    names = [p[0] for p in progs]
    assert len(progs) == len(UNARY) + 2 * len(BINARY) + 7 and "8 leaves" in names
    assert [p[1].n_leaves for p in progs if p[0] == "8 leaves"] == [8]
    for name, prog, keep, is_bool in progs:
        plib.vm_jit_probe(prog, KIND_AXES, 0, int(is_bool), log, len(log))
        assert log.value.startswith(b"k_fused_evalaxes_"), (name, log.value[:40])   # the log of a probe starts with the kernel's name


def test_axes_wide_index_form_compiles(lib, on_gpu, product):
    """The 64-bit index form (2^31 vectors and more; option jit_axes_wide forces it) of a three- and a four-axis program."""
    from minidiff_amd import ndarray as nd
    plib, log = product
    prev = nd.set_lazy(True)
    try:
        progs = [p for p in _three_axis_programs(nd) if p[0] in ("leaf modes", "four axes", "bool result")]
    finally:
        nd.set_lazy(prev)
    old = C.c_int64()
    plib.debug_get_option(b"jit_axes_wide", C.byref(old))
    plib.debug_set_option(b"jit_axes_wide", 1)
    try:
        for name, prog, keep, is_bool in progs:
            plib.vm_jit_probe(prog, KIND_AXES, 0, int(is_bool), log, len(log))
    finally:
        plib.debug_set_option(b"jit_axes_wide", old.value)


def test_axes_multi_output_kernels_compile(lib, on_gpu, product):
    """mdhip_vm_jit_probe_multi on 2, 3 and 4 three-axis programs that share leaves (it takes the axes form by the merged geometry)."""
    from minidiff_amd import lazy as lz, ndarray as nd
    plib, log = product
    prev = nd.set_lazy(True)
    try:
        rng = np.random.default_rng(1)
        f32 = lambda *s: nd.asarray(rng.standard_normal(s).astype(np.float32))   # noqa: E731
        x, g, h = f32(2, 3, 8), f32(2, 1, 8), f32(1, 3, 1)
        s = nd.add(nd.multiply(x, g), h)
        arrs = [nd.multiply(nd.multiply(s, 2.0), g), nd.multiply(nd.multiply(s, 2.0), x), nd.where(nd.greater(s, 0.25), nd.sin(x), nd.cos(x)),
                nd.subtract(h, nd.exp(g))]
        for n in (2, 3, 4):
            progs = (_capi.VmProgram * n)()
            keep = []
            for k in range(n):
                prog, kp = lz.build_program(arrs[k]._expr, arrs[k].shape)
                progs[k] = prog
                keep.append(kp)
            plib.vm_jit_probe_multi(progs, n, log, len(log))
            assert log.value.startswith(b"k_fused_evalaxes%d_" % n), log.value[:40]      # the axes form, chosen by the merged geometry
        # .. and the same programs over leaves that collapse to (rows, inner) keep the two-axis form
        x2, g2, h2 = f32(6, 8), f32(1, 8), f32(6, 1)
        s2 = nd.add(nd.multiply(x2, g2), h2)
        flat = [nd.multiply(nd.multiply(s2, 2.0), g2), nd.multiply(nd.multiply(s2, 2.0), x2)]
        progs = (_capi.VmProgram * 2)()
        keep = [lz.build_program(a._expr, a.shape) for a in flat]
        for k in range(2):
            progs[k] = keep[k][0]
        plib.vm_jit_probe_multi(progs, 2, log, len(log))
        assert log.value.startswith(b"k_fused_eval2_"), log.value[:40]
    finally:
        nd.set_lazy(prev)


# ------------------------------------------------------------------------------------------------------------ B. device parity
S3, S4 = (8, 16, 512), (2, 8, 8, 512)


def _chains(z0):
    """the nine fused chains of tests/test_elementwise_accuracy.py, `(x*g + h)**2`, and a where(x*g > 0, ..) chain with a bool result"""
    return [
        ("x*y + z", lambda q, x, y, z, m: q.add(q.multiply(x, y), z)),
        ("z + x*y", lambda q, x, y, z, m: q.add(z, q.multiply(x, y))),
        ("x*y - z", lambda q, x, y, z, m: q.subtract(q.multiply(x, y), z)),
        ("z - x*y", lambda q, x, y, z, m: q.subtract(z, q.multiply(x, y))),
        ("(x + y)*z", lambda q, x, y, z, m: q.multiply(q.add(x, y), z)),
        ("x*x + y", lambda q, x, y, z, m: q.add(q.multiply(x, x), y)),
        ("x/y + z", lambda q, x, y, z, m: q.add(q.true_divide(x, y), z)),
        ("where(m, x*y, 0) + z", lambda q, x, y, z, m: q.add(q.where(m, q.multiply(x, y), z0), z)),
        ("exp(x)*y + z", lambda q, x, y, z, m: q.add(q.multiply(q.exp(x), y), z)),
        ("(x*y + z)**2", lambda q, x, y, z, m: q.power(q.add(q.multiply(x, y), z), 2)),
        ("where(x*y > 0, x, z) < 0.25", lambda q, x, y, z, m: q.less(q.where(q.greater(q.multiply(x, y), 0), x, z), 0.25)),
    ]


def _leaf_set(nd, name):
    """(x, y, z, m) device operands; every chain reads x and y, and these two alone already keep three (four) axes apart"""
    rng = np.random.default_rng(sum(map(ord, name)))
    dt = np.float64 if name == "float64" else np.float32
    f = lambda *s: nd.asarray(rng.standard_normal(s).astype(dt))          # noqa: E731
    b = lambda *s: nd.asarray(rng.integers(0, 2, s) == 1)                 # noqa: E731
    B, R, Cn = S3
    if name in ("x*(B,1,C) + (1,R,1)", "float64"):
        return f(B, R, Cn), f(B, 1, Cn), f(1, R, 1), b(B, R, Cn)
    if name == "(N,C,H,W)*(1,C,1,W)":
        N, Ch, H, W = S4
        return f(N, Ch, H, W), f(1, Ch, 1, W), f(N, Ch, H, W), b(N, Ch, H, W)
    if name == "sliced view":                     # x[:, ::2, :]: outer strides stay multiples of 4
        return f(B, 2 * R, Cn)[:, ::2, :], f(B, 1, Cn), f(B, R, Cn), b(B, R, Cn)
    if name == "inner stride 0":                  # y: inner stride 0, outer strides (0, 1)
        return f(B, R, Cn), f(1, R, 1), f(B, 1, Cn), b(B, R, Cn)
    if name == "0-d seed":                        # z: one device element behind a stride-0 view
        return f(B, R, Cn), f(B, 1, Cn), nd.broadcast_to(nd.asarray(dt(0.375)), S3), b(B, R, Cn)
    if name == "bool mask leaf":                  # m: a broadcast bool leaf (4-byte vector loads)
        return f(B, R, Cn), f(1, R, 1), f(B, R, Cn), b(B, 1, Cn)
    if name == "int32 leaf":
        return f(B, R, Cn), nd.asarray(rng.integers(-9, 10, (B, 1, Cn)).astype(np.int32)), f(1, R, 1), b(B, R, Cn)
    raise KeyError(name)


LEAF_SETS = ["x*(B,1,C) + (1,R,1)", "(N,C,H,W)*(1,C,1,W)", "sliced view", "inner stride 0", "0-d seed", "bool mask leaf", "int32 leaf",
             "float64"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    bad = _bits(got) != _bits(exp)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {tuple(np.argwhere(bad)[0])}"


def _launched(lib):
    st = (C.c_int64 * 2)()
    lib.vm_jit_stats(st)
    return int(st[1])


@gpu
@pytest.mark.parametrize("leaves", LEAF_SETS)
def test_axes_chains_bit_identical_gpu(lib, on_gpu, mdopt, leaves):
    """Every chain over one leaf set: the generated axes kernel (exactly one launch per evaluation) gives the bits of the
    interpreter (option jit = 0: no launch counted) and of the eager calls; the first chain once more in the 64-bit index form."""
    from minidiff_amd import ndarray as nd
    assert on_gpu
    prev = nd.set_lazy(False)
    try:
        x, y, z, m = _leaf_set(nd, leaves)
        chains = _chains(np.float64(0) if leaves == "float64" else np.float32(0))
        eager = [f(nd, x, y, z, m).get() for _, f in chains]
        assert eager[0].shape == (S4 if leaves == "(N,C,H,W)*(1,C,1,W)" else S3)
        assert eager[-1].dtype == np.bool_ and eager[0].dtype == (np.float64 if leaves == "float64" else eager[0].dtype)
        nd.set_lazy(True)
        mdopt("jit_min", 1)
        for jit, wide in ((1, 0), (0, 0), (1, 1)):
            mdopt("jit", jit)
            mdopt("jit_axes_wide", wide)
            for (label, f), e in list(zip(chains, eager))[:1 if wide else None]:
                what = f"{leaves}: {label}: lazy, jit = {jit}, jit_axes_wide = {wide}"
                r = f(nd, x, y, z, m)
                assert r._expr is not None and r._buf is None, what
                before = _launched(lib)
                got = r.get()
                assert _launched(lib) - before == jit, f"{what}: generated kernels launched"
                _same_bits(got, e, f"{what} against eager")
    finally:
        nd.set_lazy(prev)


@gpu
def test_axes_multi_output_gpu(lib, on_gpu, mdopt):
    """Two and four pending chains over shared three-axis leaves, forced by materialize_many: one call, one generated kernel, each
    result the bits of its single evaluation (generated and interpreted) and of eager; with jit = 0 the same bits and no launch."""
    from minidiff_amd import ndarray as nd
    assert on_gpu
    prev = nd.set_lazy(False)
    try:
        x, y, z, m = _leaf_set(nd, LEAF_SETS[0])
        chains = _chains(np.float32(0))[:10]      # (materialize_many shares a pass among float results)
        eager = [f(nd, x, y, z, m).get() for _, f in chains]
        nd.set_lazy(True)
        mdopt("jit_min", 1)
        mdopt("jit", 1)
        single = [f(nd, x, y, z, m).get() for _, f in chains]
        for jit in (1, 0):
            mdopt("jit", jit)
            for lo, n in ((0, 2), (2, 4), (6, 4)):
                what = f"chains {lo}..{lo + n - 1}, jit = {jit}"
                s0 = dict(nd.FUSION_STATS)
                outs = [f(nd, x, y, z, m) for _, f in chains[lo:lo + n]]
                assert all(o._expr is not None and o._buf is None for o in outs), what
                before = _launched(lib)
                nd.materialize_many(outs)
                assert nd.FUSION_STATS["vm_eval_multi"] - s0["vm_eval_multi"] == 1, f"{what}: materialize_many did not share a call"
                assert _launched(lib) - before == jit, f"{what}: generated kernels launched"
                for o, (label, _), e, s in zip(outs, chains[lo:lo + n], eager[lo:lo + n], single[lo:lo + n]):
                    _same_bits(o.get(), s, f"{what}: {label} against its single evaluation")
                    _same_bits(o.get(), e, f"{what}: {label} against eager")
    finally:
        nd.set_lazy(prev)


@gpu
@pytest.mark.parametrize("jit_u", [1, 2, 4])
def test_axes_trip_loop_gpu(lib, on_gpu, mdopt, jit_u):
    """The unrolled trip loop and its hand-over to the tail: with the grid capped at 10 blocks (option max_blocks) the 16384 vectors of
    these shapes take 6 (U = 1), 3 (U = 2) or 1 (U = 4) main trips of U vectors per lane, then a ragged tail. Three axes (a float and
    a bool result, two and four outputs), four axes and float64 (one chain); 32- and 64-bit index form: the bits of eager and of the
    interpreter. (Few programs per case: every one is a compilation.)"""
    from minidiff_amd import ndarray as nd
    assert on_gpu
    blocks, vectors = 10, S3[0] * S3[1] * S3[2] // 4
    gs = blocks * 256
    assert jit_u * gs < vectors and (jit_u == 1 or vectors % (jit_u * gs) != 0)      # at least one main trip, and a tail
    prev = nd.set_lazy(False)
    try:
        for leaves in (LEAF_SETS[0], LEAF_SETS[1], "float64"):
            x, y, z, m = _leaf_set(nd, leaves)
            chains = _chains(np.float64(0) if leaves == "float64" else np.float32(0))
            three = leaves == LEAF_SETS[0]
            picks = [chains[i] for i in ((0, 2, 7, 9, 10) if three else (9,) if leaves == "float64" else (9, 10))]
            singles = [(0, 4) if three else tuple(range(len(picks)))][0]
            nd.set_lazy(False)
            for name in ("max_blocks", "jit_u", "jit_axes_wide"):
                mdopt(name, 0)
            eager = [f(nd, x, y, z, m).get() for _, f in picks]
            nd.set_lazy(True)
            mdopt("jit_min", 1)
            mdopt("max_blocks", blocks)
            mdopt("jit_u", jit_u)
            for jit, wide in ((0, 0), (1, 0), (1, 1)) if leaves != "float64" else ((0, 0), (1, 0)):
                mdopt("jit", jit)
                mdopt("jit_axes_wide", wide)
                what = f"{leaves}: jit = {jit}, jit_u = {jit_u}, jit_axes_wide = {wide}, max_blocks = {blocks}"
                for (label, f), e in [(picks[i], eager[i]) for i in singles]:
                    before = _launched(lib)
                    got = f(nd, x, y, z, m).get()
                    assert _launched(lib) - before == jit, f"{what}: {label}: generated kernels launched"
                    _same_bits(got, e, f"{what}: {label} against eager")
                if not (jit and three):
                    continue
                for n in (2, 4):                     # the float results share a pass
                    outs = [f(nd, x, y, z, m) for _, f in picks[:n]]
                    before = _launched(lib)
                    nd.materialize_many(outs)
                    assert _launched(lib) - before == 1, f"{what}: {n} outputs: generated kernels launched"
                    for o, (label, _), e in zip(outs, picks, eager):
                        _same_bits(o.get(), e, f"{what}: {n} outputs: {label} against eager")
    finally:
        nd.set_lazy(prev)
