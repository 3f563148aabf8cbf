"""Lazy mode, MDHIP_LAZY_ROWS: a chain that continues PAST a trailing-axis reduction — softmax, its gradient, a mean / variance layer
norm — in one launch of a staged program (include/mdhip.h: MDHIP_VM_ROWRED, MDHIP_VM_SRC_ROW), rows held in registers.

CPU  the test double refuses staged programs, so the switch must change nothing there: same bits, same reduction counts; the rules by
     which a reduction stays pending and by which it is materialised; the program format and its validation; a compile-only check of
     the generated kernels through the product library's probe (kind 10; no device needed).
GPU  the staged launch against the COMPOSED route — mdhip_vm_reduce per stage, mdhip_vm_eval over the results as (n_out, 1) leaves,
     generated kernels forced — bit for bit (each stage combines in the order of the wave-per-row reduction); against NumPy with
     operands whose sums and products are exact in any order, through every leaf mode, outputs inside sentinel padding; special
     values; launch counts; the tape; refusals that compose."""
import ctypes as C
import os

import numpy as np
import pytest

from minidiff_amd import _capi
from minidiff_amd._capi import (B_ADD, B_MUL, B_SUB, B_TRUE_DIV, R_MAX, R_MIN, R_PROD, R_SUM, U_EXP, U_SIGN, U_SQRT, VM_BINARY, VM_PUSH,
                                VM_ROWRED, VM_SRC_CONST, VM_SRC_LEAF, VM_SRC_ROW, VM_SRC_STACK, VM_UNARY, vm_ctrl)

gpu = pytest.mark.gpu
f32, f64 = np.dtype(np.float32), np.dtype(np.float64)
ST, LF, CN, RW = VM_SRC_STACK, VM_SRC_LEAF, VM_SRC_CONST, VM_SRC_ROW
RED_STATS = ("vm_reduce", "vm_reduce_rows", "vm_reduce_axis", "vm_eval_reduce_cols", "deferred_cols")


@pytest.fixture
def rows_nd(lib):
    """lazy mode with the rows switch ON; both put back afterwards"""
    from minidiff_amd import ndarray as nd
    prev, prev_rows = nd.set_lazy(True), nd.set_lazy_rows(True)
    yield nd
    nd.set_lazy_rows(prev_rows)
    nd.set_lazy(prev)


@pytest.fixture(scope="module")
def product():
    if not os.path.exists(_capi.PRODUCT_LIB):
        pytest.skip("libmdhip.so not built")
    return _capi.Library(_capi.PRODUCT_LIB), C.create_string_buffer(1 << 16)   # dlopen only; the probe needs no GPU


def _same(got, exp, what):
    """bit for bit; a NaN matches any NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    gn, en = np.isnan(got), np.isnan(exp)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = (gn != en) | (~en & (np.ascontiguousarray(got).view(u) != np.ascontiguousarray(exp).view(u)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} against {exp[tuple(np.argwhere(bad)[0])]!r}"


def _launched(lib):
    st = (C.c_int64 * 2)()
    lib.vm_jit_stats(st)
    return int(st[1])


# ------------------------------------------------------------------------------------------------ the workloads, through the nd API
def _softmax(nd, x, axis=-1):
    m = nd.max(x, axis=axis, keepdims=True)
    e = nd.exp(nd.subtract(x, m))
    return nd.true_divide(e, nd.sum(e, axis=axis, keepdims=True))


def _log_softmax(nd, x):
    z = nd.subtract(x, nd.max(x, axis=-1, keepdims=True))
    return nd.subtract(z, nd.log(nd.sum(nd.exp(z), axis=-1, keepdims=True)))


def _layer_norm(nd, x, gamma, beta):
    d = nd.subtract(x, nd.mean(x, axis=-1, keepdims=True))
    v = nd.mean(nd.multiply(d, d), axis=-1, keepdims=True)
    return nd.add(nd.multiply(nd.true_divide(d, nd.sqrt(nd.add(v, 1e-5))), gamma), beta)


def _softmax_grad(nd, p, g):
    return nd.multiply(p, nd.subtract(g, nd.sum(nd.multiply(g, p), axis=-1, keepdims=True)))


def _operands(nd, dt, R, Cn, seed=0):
    rng = np.random.default_rng(seed)
    mk = lambda *s: nd.asarray(rng.standard_normal(s).astype(dt))     # noqa: E731
    return mk(R, Cn), mk(R, Cn), mk(Cn), mk(Cn)


def _workloads(nd, dt, R, Cn, seed=0):
    x, g, gamma, beta = _operands(nd, dt, R, Cn, seed)
    return [("softmax", lambda: _softmax(nd, x)), ("log-softmax", lambda: _log_softmax(nd, x)),
            ("layer norm", lambda: _layer_norm(nd, x, gamma, beta)), ("softmax gradient", lambda: _softmax_grad(nd, x, g))]


def _both(nd, make):
    """make() with the rows switch off, then on: (values off, values on, FUSION_STATS deltas off, on)"""
    out = []
    for flag in (False, True):
        prev = nd.set_lazy_rows(flag)
        try:
            s0 = dict(nd.FUSION_STATS)
            v = make()
            v = [a.get() for a in v] if isinstance(v, (list, tuple)) else v.get()
            out.append((v, {k: nd.FUSION_STATS[k] - s0[k] for k in s0}))
        finally:
            nd.set_lazy_rows(prev)
    return out[0][0], out[1][0], out[0][1], out[1][1]


# ----------------------------------------------------------------------------------------------- CPU: nothing changes where refused
@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_refused_programs_compose_to_the_switch_off_result(rows_nd, dt):
    """(6, 16): under the double every staged program is refused, and on a device this is below jit_min — either way the statistics are
    materialised by the switch-off route and the chain runs over them as leaves: same bits, same reduction counts, no staged launch."""
    nd = rows_nd
    for what, make in _workloads(nd, dt, 6, 16)[:3]:
        off, on, s_off, s_on = _both(nd, make)
        _same(on, off, what)
        assert [s_on[k] for k in RED_STATS] == [s_off[k] for k in RED_STATS], (what, s_off, s_on)
        assert s_on["vm_eval_rows"] == 0 and s_off["vm_eval_rows"] == 0


def _tape_softmax_xent(nd, dt, R, Cn):
    """softmax cross-entropy through the tape as tests/test_fused_rows.py issues it, the row sums with keepdims, and the probabilities
    read before the loss is formed (the one (R, C) value of the forward pass that is needed in memory): (loss, logits' gradient, p)"""
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    md = build_engine(HipBackendTable, "rows")
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((R, Cn)) * 3).astype(dt)
    y = np.zeros((R, Cn), dt)
    y[np.arange(R), rng.integers(0, Cn, R)] = 1
    X, Y = md.Tensor(x, allow_grad=True), md.Tensor(y)
    m = md.Tensor(nd.max(X._data, axis=-1, keepdims=True))
    z = X - m
    s = md.sum(md.exp(z), axis=(1,), keepdims=True)
    logp = z - md.log(s)
    p = md.exp(logp).as_numpy()
    loss = md.sum(md.sum(Y * logp, axis=(1,), keepdims=True)) / (-R)
    loss.backward()
    return loss.as_numpy(), X.grad.as_numpy(), p


@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_tape_softmax_composes_to_the_switch_off_result(rows_nd, dt):
    nd = rows_nd
    off, on, s_off, s_on = _both(nd, lambda: [nd.asarray(a) for a in _tape_softmax_xent(nd, dt, 6, 16)])
    _same(on[0], off[0], "loss")
    _same(on[1], off[1], "gradient")
    _same(on[2], off[2], "probabilities")
    assert [s_on[k] for k in RED_STATS] == [s_off[k] for k in RED_STATS], (s_off, s_on)


# ------------------------------------------------------------------------------------------- CPU: pending and materialising rules
def test_pending_and_materialising_rules(rows_nd):
    nd = rows_nd
    from minidiff_amd import lazy as lz
    rng = np.random.default_rng(1)
    xh = rng.standard_normal((6, 16)).astype(np.float32)
    x = nd.asarray(xh)
    # pending; read alone it is the eager value
    m = nd.max(x, axis=-1, keepdims=True)
    assert m._expr is not None and m._expr.kind == lz.ROWRED and m._buf is None and m.shape == (6, 1)
    _same(m.get(), xh.max(axis=-1, keepdims=True), "max read alone")
    assert m._expr is None
    for op in ("sum", "prod", "min"):
        r = getattr(nd, op)(x, axis=-1, keepdims=True)
        assert r._expr is not None and r._expr.kind == lz.ROWRED, op
        prev = nd.set_lazy(False)
        ref = getattr(nd, op)(x, axis=-1, keepdims=True).get()
        nd.set_lazy(prev)
        _same(r.get(), ref, f"{op} read alone")
    # per-row scalar arithmetic stays pending; over a pending operand the child is the operand's expression
    s = nd.sum(nd.multiply(x, x), axis=-1, keepdims=True)
    q = nd.sqrt(nd.true_divide(s, 16.0))
    assert s._expr.kind == lz.ROWRED and s._expr.args[0].kind == lz.BINARY and q._expr is not None and len(lz.live_rows(q._expr)) == 1
    np.testing.assert_allclose(q.get(), np.sqrt((xh * xh).sum(-1, keepdims=True) / 16), rtol=1e-6)
    assert s._expr is None, "materialising the consumer made the statistic concrete"
    # a consumer of another shape materialises the node first
    m = nd.max(x, axis=-1, keepdims=True)
    other = nd.add(m, nd.asarray(np.ones((6, 4), np.float32)))
    assert m._expr is None and other._expr is not None and not lz.live_rows(other._expr)
    _same(other.get(), xh.max(axis=-1, keepdims=True) + np.ones((6, 4), np.float32), "another shape")
    # statistics of different rows do not share a program
    y = nd.asarray(rng.standard_normal((6, 32)).astype(np.float32))
    a, b = nd.max(x, axis=-1, keepdims=True), nd.max(y, axis=-1, keepdims=True)
    c = nd.add(a, b)
    assert not lz.live_rows(c._expr)
    _same(c.get(), xh.max(axis=-1, keepdims=True) + y.get().max(axis=-1, keepdims=True), "rows of two lengths")
    # over the limits the chain materialises instead of failing: five statistics (four registers) ..
    t = x
    for op in ("sum", "max", "min", "prod", "sum"):
        t = nd.add(t, getattr(nd, op)(x, axis=-1, keepdims=True))
    assert t._expr is not None and len(lz.live_rows(t._expr)) <= lz.MAX_ROWS
    ref = xh + xh.sum(-1, keepdims=True)
    for op in ("max", "min", "prod", "sum"):
        ref = ref + getattr(xh, op)(-1, keepdims=True)
    np.testing.assert_allclose(t.get(), ref, rtol=1e-5, atol=1e-5)
    # .. and a chain longer than a program holds
    t = nd.subtract(x, nd.max(x, axis=-1, keepdims=True))
    for k in range(60):
        t = nd.add(nd.multiply(t, 1.0), 0.0)
    _same(t.get(), xh - xh.max(axis=-1, keepdims=True), "a long chain")
    # not recorded: keepdims=False, dtype=, out=, integer and float16 operands, rows longer than 2048, ragged rows
    assert nd.max(x, axis=-1)._expr is None
    assert nd.sum(x, axis=-1, keepdims=True, dtype=np.float64)._expr is None
    o = nd.asarray(np.zeros((6, 1), np.float32))
    assert nd.sum(x, axis=-1, keepdims=True, out=o) is o and o._expr is None
    _same(o.get(), nd.sum(x, axis=-1, keepdims=True).get(), "out=")
    assert nd.sum(nd.asarray(np.arange(96).reshape(6, 16)), axis=-1, keepdims=True)._expr is None
    assert nd.max(nd.asarray(xh.astype(np.float16)), axis=-1, keepdims=True)._expr is None
    assert nd.max(nd.asarray(np.zeros((256, 2052), np.float32)), axis=-1, keepdims=True)._expr is None
    assert nd.max(nd.asarray(np.zeros((6, 10), np.float32)), axis=-1, keepdims=True)._expr is None
    assert nd.max(x, axis=0, keepdims=True)._expr is None
    # the switch only matters inside lazy mode, and off is today's route
    nd.set_lazy(False)
    assert nd.max(x, axis=-1, keepdims=True)._expr is None
    nd.set_lazy(True)
    assert nd.set_lazy_rows(False) is True and not nd.lazy_rows_enabled()
    assert nd.max(x, axis=-1, keepdims=True)._expr is None
    assert nd.set_lazy_rows(True) is False and nd.lazy_rows_enabled()


def test_in_place_write_sees_the_recorded_bytes(rows_nd):
    """a pending statistic and the chains over it read the operand as it was when they were recorded"""
    nd = rows_nd
    xh = np.arange(96, dtype=np.float32).reshape(6, 16)
    x = nd.asarray(xh)
    p = nd.subtract(x, nd.max(x, axis=-1, keepdims=True))
    x += 100.0
    _same(p.get(), xh - xh.max(axis=-1, keepdims=True), "chain recorded before the write")
    # a PENDING operand that is materialised and then written in place: the statistic is the recorded expression's, read alone
    # and under a chain, whichever of them is read first
    for first in ("m", "p"):
        for write in ("add", "mul"):
            x = nd.asarray(xh)
            t = nd.multiply(x, 2.0)
            m = nd.max(t, axis=-1, keepdims=True)
            s = nd.sum(t, axis=-1, keepdims=True)
            p = nd.subtract(nd.subtract(t, m), s)
            t.get()
            if write == "add":
                t += 100.0
            else:
                t *= 0.0
            th = xh * np.float32(2.0)
            got = {}
            for name in ((first, "p") if first == "m" else (first, "m")):
                got[name] = (m if name == "m" else p).get()
            _same(got["m"], th.max(axis=-1, keepdims=True), f"max read {'first' if first == 'm' else 'second'}, operand {write}-ed in place")
            nd.set_lazy_rows(False)
            x2 = nd.asarray(xh)
            t2 = nd.multiply(x2, 2.0)
            ref = nd.subtract(nd.subtract(t2, nd.max(t2, axis=-1, keepdims=True)), nd.sum(t2, axis=-1, keepdims=True)).get()
            nd.set_lazy_rows(True)
            _same(got["p"], ref, f"chain, operand {write}-ed in place, {first} read first")
            _same(t.get(), th + 100 if write == "add" else th * 0, "the write itself")
    # the operand array is not kept alive by a statistic that outlives it
    import gc
    import weakref
    t = nd.multiply(nd.asarray(xh), 2.0)
    m = nd.max(t, axis=-1, keepdims=True)
    ref_t = weakref.ref(t)
    del t
    gc.collect()
    assert ref_t() is None
    _same(m.get(), (xh * np.float32(2.0)).max(axis=-1, keepdims=True), "statistic of an operand that is gone")


# ------------------------------------------------------------------------------------------------------------------ CPU: the format
def _kinds(prog):
    return [prog.ctrl[i] & 7 for i in range(prog.n_instr)]


def test_shared_statistic_is_one_stage(rows_nd):
    nd = rows_nd
    from minidiff_amd import lazy as lz
    x = nd.asarray(np.random.default_rng(0).standard_normal((6, 16)).astype(np.float32))
    p = _softmax(nd, x)
    assert len(lz.live_rows(p._expr)) == 2
    prog, keep = lz.build_program(p._expr, p.shape)
    red = [i for i in range(prog.n_instr) if prog.ctrl[i] & 7 == VM_ROWRED]
    assert len(red) == 2, "m is used by two later stages and costs one"
    assert [(prog.ctrl[i] >> 3) & 31 for i in red] == [R_MAX, R_SUM] and [(prog.ctrl[i] >> 15) & 7 for i in red] == [0, 1]
    assert [prog.imm[i] for i in red] == [16.0, 16.0] and prog.n_leaves == 1
    assert prog.n_instr == lz.cost(p._expr)[0] == 8
    # the layer norm: three statistics would be four stages if the mean were emitted per use; it has two
    q = _layer_norm(nd, x, nd.asarray(np.ones(16, np.float32)), nd.asarray(np.zeros(16, np.float32)))
    prog, keep = lz.build_program(q._expr, q.shape)
    assert _kinds(prog).count(VM_ROWRED) == 2 and prog.n_instr == lz.cost(q._expr)[0]


def _raw_program(dt, instrs, leaves, shape):
    prog = _capi.VmProgram()
    prog.n_instr, prog.n_leaves, prog.compute_dtype = len(instrs), len(leaves), _capi.F32 if dt == f32 else _capi.F64
    for i, (word, imm) in enumerate(instrs):
        prog.ctrl[i], prog.imm[i] = word, imm
    for i, a in enumerate(leaves):
        prog.leaves[i] = a.desc(shape)
    return prog


def _shape_like(dt, shape):
    d = _capi.ArrayDesc()
    d.dtype, d.ndim = _capi.F32 if dt == f32 else _capi.F64, len(shape)
    d.shape[:len(shape)] = shape
    return d


def test_staged_programs_are_refused_everywhere_else(rows_nd, lib, on_gpu, product):
    nd = rows_nd
    from minidiff_amd import lazy as lz
    plib, _ = product
    x = nd.asarray(np.random.default_rng(0).standard_normal((8, 16)).astype(np.float32))
    p = _softmax(nd, x)
    prog, keep = lz.build_program(p._expr, p.shape)
    out, red, col = nd.DeviceArray.empty((8, 16), np.float32), nd.DeviceArray.empty((8, 1), np.float32), nd.DeviceArray.empty((1, 16), np.float32)
    progs = (_capi.VmProgram * 2)(prog, prog)
    outs = (_capi.ArrayDesc * 2)(out.desc(), out.desc())
    for which, L in (("double or bound library", lib), ("product", plib)):
        with pytest.raises(ValueError):
            L.vm_reduce(prog, R_SUM, _shape_like(f32, (8, 16)), red.desc(), 2)
        with pytest.raises(ValueError):
            L.vm_eval_multi(progs, outs, 2)
        with pytest.raises(ValueError):
            L.vm_eval_reduce_cols(prog, R_SUM, out.desc(), col.desc())
    if not on_gpu:
        with pytest.raises(ValueError):
            lib.vm_eval(prog, out.desc())      # the double's one-element interpreter never sees kind 4


def test_malformed_staged_programs_are_refused(rows_nd, product):
    nd = rows_nd
    plib, log = product
    x = nd.asarray(np.zeros((8, 16), np.float32))
    push = (vm_ctrl(VM_PUSH, 0, 0, 0, LF, 0), 0.0)
    red = lambda k, op=R_MAX: (vm_ctrl(VM_ROWRED, op, 0, 0, 0, k), 16.0)          # noqa: E731
    sub_r = lambda k: (vm_ctrl(VM_BINARY, B_SUB, LF, 0, RW, k), 0.0)            # noqa: E731
    good = [push, red(0), sub_r(0)]
    plib.vm_jit_probe(_raw_program(f32, good, [x], (8, 16)), 10, 0, 0, log, len(log))
    assert log.value.decode().startswith("k_fused_rowsres1")
    bad = {
        "two values on the stack": [push, push, red(0), sub_r(0)],
        "a register read before it is written": [sub_r(0), red(0), sub_r(0)],
        "a register of a later stage": [push, red(0), sub_r(1)],
        "register 4": [push, red(0), push, red(1), push, red(2), push, red(3), push, red(4), sub_r(0)],
        "registers out of order": [push, red(1), sub_r(0)],
        "RND16 on a ROWRED": [push, (vm_ctrl(VM_ROWRED, R_MAX, 0, 0, 0, 0, True), 16.0), sub_r(0)],
        "a final stage that leaves nothing": [push, red(0)],
        "a final stage that leaves two": [push, red(0), push, push],
        "a reduce op that is not fused": [push, red(0, 4), sub_r(0)],
        "two row lengths": [push, red(0), push, (vm_ctrl(VM_ROWRED, R_MAX, 0, 0, 0, 1), 8.0), sub_r(0)],
        "a ragged row length": [push, (vm_ctrl(VM_ROWRED, R_MAX, 0, 0, 0, 0), 10.0), sub_r(0)],
        "a row register as the source of a unary": [push, red(0), push, (vm_ctrl(VM_UNARY, U_EXP, RW, 0, 0, 0), 0.0)],
    }
    for what, instrs in bad.items():
        with pytest.raises(ValueError):
            plib.vm_jit_probe(_raw_program(f32, instrs, [x], (8, 16)), 10, 0, 0, log, len(log))
        for kind in (0, 6):     # and the other kinds refuse every staged program, well formed or not
            with pytest.raises(ValueError):
                plib.vm_jit_probe(_raw_program(f32, instrs, [x], (8, 16)), kind, 0, 0, log, len(log))
    with pytest.raises(ValueError):
        plib.vm_jit_probe(_raw_program(f32, good, [x], (8, 16)), 6, 0, 0, log, len(log))
    with pytest.raises(ValueError):     # kind 10 takes staged programs only
        plib.vm_jit_probe(_raw_program(f32, [push], [x], (8, 16)), 10, 0, 0, log, len(log))


# ------------------------------------------------------------------------------------------------------------- CPU: compile-only
@pytest.mark.parametrize("n_red", [256, 512, 1024, 2048])
@pytest.mark.parametrize("dt", [f32, f64], ids=lambda d: d.name)
def test_staged_kernels_compile(rows_nd, product, dt, n_red):
    """softmax, log-softmax, layer norm and the softmax gradient at every NV, with the compiler's resource remarks: none spills"""
    nd = rows_nd
    from minidiff_amd import lazy as lz
    plib, log = product
    nv = {256: 1, 512: 2, 1024: 4, 2048: 8}[n_red]
    old = C.c_int64()
    plib.debug_get_option(b"jit_verbose", C.byref(old))
    plib.debug_set_option(b"jit_verbose", 2)
    try:
        for what, make in _workloads(nd, dt, 4, n_red):
            p = make()
            prog, keep = lz.build_program(p._expr, p.shape)
            plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
            text = log.value.decode()
            assert text.startswith(f"k_fused_rowsres{nv}_"), (what, text[:80])
            assert "ScratchSize [bytes/lane]: 0" in text and "ScratchSize [bytes/lane]: " in text, (what, n_red, dt, text)
    finally:
        plib.debug_set_option(b"jit_verbose", old.value)


def test_staged_kernels_compile_at_the_register_ceiling(rows_nd, product):
    """fusion.hip's VM_STAGED_HELD_MAX = 256 held registers per lane: a layer norm whose operand, gamma and beta are all full (R, C)
    leaves — four float64 vector leaves at NV = 8 hold exactly 256, six float32 ones 192 (a seventh does not fit a program next to
    two registers) — compiles without scratch; one leaf more is refused, not spilled."""
    nd = rows_nd
    from minidiff_amd import lazy as lz
    plib, log = product
    rng = np.random.default_rng(0)
    old = C.c_int64()
    plib.debug_get_option(b"jit_verbose", C.byref(old))
    plib.debug_set_option(b"jit_verbose", 2)
    try:
        for dt, n_leaves, fits in ((f64, 4, True), (f32, 6, True), (f64, 5, False)):
            ls = [nd.asarray(rng.standard_normal((4, 2048)).astype(dt)) for _ in range(n_leaves)]
            x = ls[0]
            for leaf in ls[1:-2]:
                x = nd.add(x, leaf)
            p = _layer_norm(nd, x, ls[-2], ls[-1])
            assert len(lz.live_rows(p._expr)) == 2
            prog, keep = lz.build_program(p._expr, p.shape)
            assert prog.n_leaves == n_leaves
            if not fits:
                with pytest.raises(ValueError):
                    plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
                continue
            plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
            text = log.value.decode()
            assert text.startswith("k_fused_rowsres8_") and "ScratchSize [bytes/lane]: 0" in text, (dt, n_leaves, text)
    finally:
        plib.debug_set_option(b"jit_verbose", old.value)


def test_staged_kernels_compile_with_narrow_leaves(rows_nd, product):
    nd = rows_nd
    from minidiff_amd import lazy as lz
    plib, log = product
    rng = np.random.default_rng(0)
    x = nd.asarray(rng.standard_normal((4, 512)).astype(np.float32))
    h = nd.asarray(rng.standard_normal((4, 512)).astype(np.float16))
    b = nd.asarray(rng.integers(0, 2, (4, 512)).astype(bool))
    for what, leafed in (("float16 leaf", nd.add(x, h)), ("bool leaf", nd.multiply(x, b))):
        p = _softmax(nd, leafed)
        prog, keep = lz.build_program(p._expr, p.shape)
        assert prog.n_leaves == 2
        plib.vm_jit_probe(prog, 10, 0, 0, log, len(log))
        assert log.value.decode().startswith("k_fused_rowsres2_"), what


# =================================================================================================================== GPU
N_RED = [4, 252, 256, 260, 512, 516, 1024, 1028, 2048]     # both sides of each NV step
N_OUT = [2, 3, 4, 5, 257]                                  # a partial last block


@pytest.fixture
def generated(mdopt):
    mdopt("jit", 1)
    mdopt("jit_min", 1)


def _ins(kind, op=0, ls=0, ll=0, rs=0, rl=0, imm=0.0):
    return (kind, op, ls, ll, rs, rl, imm)


def _abi_programs(n_red):
    """(name, leaves wanted, instructions): leaf 0 is x (n_out, n_red); `g` marks a (n_red,) vector leaf"""
    inv = 1.0 / n_red
    x_minus_max = [_ins(VM_PUSH, rs=LF, rl=0), _ins(VM_ROWRED, R_MAX), _ins(VM_BINARY, B_SUB, LF, 0, RW, 0)]
    softmax = [_ins(VM_PUSH, rs=LF, rl=0), _ins(VM_ROWRED, R_MAX),
               _ins(VM_BINARY, B_SUB, LF, 0, RW, 0), _ins(VM_UNARY, U_EXP), _ins(VM_ROWRED, R_SUM),
               _ins(VM_BINARY, B_SUB, LF, 0, RW, 0), _ins(VM_UNARY, U_EXP), _ins(VM_BINARY, B_TRUE_DIV, ST, 0, RW, 1)]
    # mean = sum(x) * (1/n); var = sum((x - mean)^2) * (1/n); (x - mean) / sqrt(var + eps) * gamma + beta — the mean's scaling is part
    # of every stage that uses it (a register holds what a ROWRED wrote: the sum)
    mean = [_ins(VM_PUSH, rs=RW, rl=0), _ins(VM_BINARY, B_MUL, ST, 0, CN, 0, inv)]
    centred = mean + [_ins(VM_BINARY, B_SUB, LF, 0, ST, 0)]
    layer_norm = [_ins(VM_PUSH, rs=LF, rl=0), _ins(VM_ROWRED, R_SUM)] + \
        centred + centred + [_ins(VM_BINARY, B_MUL, ST, 0, ST, 0), _ins(VM_ROWRED, R_SUM)] + \
        centred + [_ins(VM_PUSH, rs=RW, rl=1), _ins(VM_BINARY, B_MUL, ST, 0, CN, 0, inv), _ins(VM_BINARY, B_ADD, ST, 0, CN, 0, 1e-5),
                   _ins(VM_UNARY, U_SQRT), _ins(VM_BINARY, B_TRUE_DIV, ST, 0, ST, 0), _ins(VM_BINARY, B_MUL, ST, 0, LF, 1),
                   _ins(VM_BINARY, B_ADD, ST, 0, LF, 2)]
    # x * prod(sign(x)) - min(x): the other two reduce ops
    prod_min = [_ins(VM_PUSH, rs=LF, rl=0), _ins(VM_UNARY, U_SIGN), _ins(VM_ROWRED, R_PROD), _ins(VM_PUSH, rs=LF, rl=0), _ins(VM_ROWRED, R_MIN),
                _ins(VM_BINARY, B_MUL, LF, 0, RW, 0), _ins(VM_BINARY, B_SUB, ST, 0, RW, 1)]
    return [("x - max(x)", 1, x_minus_max), ("softmax", 1, softmax), ("layer norm", 3, layer_norm), ("x * prod(sign x) - min(x)", 1, prod_min)]


def _words(instrs, n_red):
    """ctrl words and immediates of a staged program: the ROWREDs write registers 0, 1, .. and carry the row length"""
    out, regs = [], 0
    for (k, op, ls, ll, rs, rl, imm) in instrs:
        if k == VM_ROWRED:
            out.append((vm_ctrl(k, op, 0, 0, 0, regs), float(n_red)))
            regs += 1
        else:
            out.append((vm_ctrl(k, op, ls, ll, rs, rl), imm))
    return out


def _composed(nd, lib, dt, instrs, leaves, shape, n_red):
    """The reference: every stage through mdhip_vm_reduce into an (n_out, 1) array, a row register read becoming a read of that
    array as a leaf; the final stage through mdhip_vm_eval. Existing entry points only."""
    stats, stage, nl = [], [], len(leaves)
    mask = 1 << (len(shape) - 1)

    def plain(seq):
        out = []
        for (k, op, ls, ll, rs, rl, imm) in seq:
            if ls == RW:
                ls, ll = LF, nl + ll
            if rs == RW:
                rs, rl = LF, nl + rl
            out.append((vm_ctrl(k, op, ls, ll, rs, rl), imm))
        return out

    for ins in instrs:
        if ins[0] == VM_ROWRED:
            prog = _raw_program(dt, plain(stage), list(leaves) + stats, shape)
            res = nd.DeviceArray.empty(shape[:-1] + (1,), dt)
            lib.vm_reduce(prog, ins[1], _shape_like(dt, shape), res.desc(), mask)
            stats.append(res)
            stage = []
        else:
            stage.append(ins)
    out = nd.DeviceArray.empty(shape, dt)
    lib.vm_eval(_raw_program(dt, plain(stage), list(leaves) + stats, shape), out.desc())
    return out.get()


PAD, SENTINEL = 64, -12345.0


def _staged_padded(nd, lib, prog, shape, dt):
    """mdhip_vm_eval of a staged program into the middle of a sentinel-filled block: (values, the block's margins untouched)"""
    n = int(np.prod(shape))
    block = nd.asarray(np.full(n + 2 * PAD, SENTINEL, dt))
    out = nd.reshape(block[PAD:PAD + n], shape)
    l0 = _launched(lib)
    lib.vm_eval(prog, out.desc())
    assert _launched(lib) - l0 == 1
    host = block.get()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + n:] == SENTINEL).all(), "written outside out"
    return host[PAD:PAD + n].reshape(shape)


@gpu
@pytest.mark.parametrize("n_red", N_RED)
def test_staged_launch_equals_the_composed_route_gpu(rows_nd, lib, on_gpu, generated, n_red):
    nd = rows_nd
    assert on_gpu
    for dt in (f32, f64):
        for n_out in N_OUT:
            rng = np.random.default_rng(n_red * 1000 + n_out)
            x = nd.asarray((rng.standard_normal((n_out, n_red)) * 2).astype(dt))
            gamma, beta = nd.asarray(rng.standard_normal(n_red).astype(dt)), nd.asarray(rng.standard_normal(n_red).astype(dt))
            for what, n_leaves, instrs in _abi_programs(n_red):
                leaves = [x, gamma, beta][:n_leaves]
                shape = (n_out, n_red)
                got = _staged_padded(nd, lib, _raw_program(dt, _words(instrs, n_red), leaves, shape), shape, dt)
                _same(got, _composed(nd, lib, dt, instrs, leaves, shape, n_red), f"{what} {dt.name} {shape}")


def _exact_cases(nd, dt, shape, axes):
    """operands whose row sums and products are exact in float32 in any order: integers in [-8, 8] (a row of 2048: |sum| <= 2^14,
    times a weight in [-3, 3] and an element: < 2^24), products of signs. Every leaf mode: dense, a sliced view with a row stride
    larger than the row, an (n_out, 1) leaf, a row-invariant leaf, constants, a float16 leaf, a bool leaf."""
    rng = np.random.default_rng(sum(shape))
    kshape = tuple(1 if i in axes else n for i, n in enumerate(shape))
    rshape = tuple(n if i in axes else 1 for i, n in enumerate(shape))
    wide = list(shape)
    wide[axes[0]] += 4 if axes[0] == len(shape) - 1 else 1        # the slice below keeps whole 16-byte groups
    big = rng.integers(-8, 9, wide).astype(dt)
    sl = tuple(slice(0, n) for n in shape)
    xs_h = big[sl]
    x_h = rng.integers(1, 9, shape).astype(dt) * rng.choice([-1, 1], shape).astype(dt)
    c_h, w_h = rng.integers(-8, 9, kshape).astype(dt), rng.integers(-3, 4, rshape).astype(dt)
    y_h, b_h = rng.integers(-8, 9, shape).astype(np.float16), rng.integers(0, 2, shape).astype(bool)
    xs, x, c, w, y, b = nd.asarray(big)[sl], nd.asarray(x_h), nd.asarray(c_h), nd.asarray(w_h), nd.asarray(y_h), nd.asarray(b_h)
    kw = dict(axis=axes, keepdims=True)
    yb_h = y_h.astype(dt) * b_h
    return [
        ("x - rowmax(x)", lambda: nd.subtract(nd.add(xs, c), nd.max(nd.add(xs, c), **kw)), (xs_h + c_h) - (xs_h + c_h).max(**kw)),
        ("x * rowsum(x)", lambda: nd.multiply(nd.multiply(xs, w), nd.sum(nd.multiply(xs, w), **kw)), (xs_h * w_h) * (xs_h * w_h).sum(**kw)),
        ("where(x == rowmin(x), 1, 0) * rowsum(y)",
         lambda: nd.multiply(nd.where(nd.equal(x, nd.min(x, **kw)), dt.type(1), dt.type(0)), nd.sum(nd.multiply(nd.astype(y, dt), b), **kw)),
         np.where(x_h == x_h.min(**kw), dt.type(1), dt.type(0)) * yb_h.sum(**kw)),
        ("x / rowprod(sign(x))", lambda: nd.true_divide(nd.multiply(x, 2.0), nd.prod(nd.sign(x), **kw)), (x_h * 2.0) / np.sign(x_h).prod(**kw)),
    ]


@gpu
@pytest.mark.parametrize("shape,axes", [((3, 5, 260), (2,)), ((5, 4, 65 * 4), (1, 2)), ((2, 3, 2048), (2,)), ((257, 4), (1,))], ids=str)
def test_exact_against_numpy_gpu(rows_nd, lib, on_gpu, generated, shape, axes):
    nd = rows_nd
    assert on_gpu
    from minidiff_amd import lazy as lz
    for dt in (f32, f64):
        for what, make, ref in _exact_cases(nd, dt, shape, axes):
            p = make()
            assert p._expr is not None and lz.live_rows(p._expr), what
            prog, keep = lz.build_program(p._expr, p.shape)
            _same(_staged_padded(nd, lib, prog, shape, dt), ref.astype(dt), f"{what} {dt.name} {shape} (C-ABI)")
            s0 = nd.FUSION_STATS["vm_eval_rows"]
            _same(p.get(), ref.astype(dt), f"{what} {dt.name} {shape}")
            assert nd.FUSION_STATS["vm_eval_rows"] - s0 == 1, what


@gpu
def test_special_values_gpu(rows_nd, lib, on_gpu, generated):
    nd = rows_nd
    assert on_gpu
    for dt in (f32, f64):
        for n_red in (8, 516):
            xh = np.random.default_rng(n_red).standard_normal((6, n_red)).astype(dt)
            xh[1, 3] = np.nan
            xh[2, :] = -np.inf
            xh[3, n_red - 1] = np.inf
            xh[4, 0], xh[4, 5] = np.nan, np.inf
            x = nd.asarray(xh)
            off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, x))
            assert s_on["vm_eval_rows"] == 1 and s_off["vm_eval_rows"] == 0
            _same(on, off, f"softmax {dt.name} {n_red}")
            assert np.isnan(on[2]).all() and np.isnan(on[3, n_red - 1]) and np.isfinite(on[0]).all() and np.isfinite(on[5]).all()


@gpu
def test_launch_counts_gpu(rows_nd, lib, on_gpu, generated):
    nd = rows_nd
    assert on_gpu
    for dt in (f32, f64):
        for what, make in _workloads(nd, dt, 64, 260, seed=5):
            vals, stats, launches = {}, {}, {}
            for flag in (False, True):
                nd.set_lazy_rows(flag)
                s0, l0 = dict(nd.FUSION_STATS), _launched(lib)
                vals[flag] = make().get()
                launches[flag] = _launched(lib) - l0
                stats[flag] = {k: nd.FUSION_STATS[k] - s0[k] for k in s0}
            off, on, s_off, s_on = vals[False], vals[True], stats[False], stats[True]
            # on: ONE generated launch and nothing else; off: the fused row reduction and the fused evaluation (and, for the
            # softmax, the eager max in front of them: three launches)
            assert launches[True] == 1 and s_on["vm_eval_rows"] == 1, (what, launches, s_on)
            assert s_on["vm_eval"] == 0 and all(s_on[k] == 0 for k in RED_STATS), (what, s_on)
            assert launches[False] == 2 and s_off["vm_eval_rows"] == 0 and s_off["vm_reduce_rows"] == 1 and s_off["vm_eval"] == 1, (what, launches, s_off)
            if what == "layer norm":
                # with the switch off the mean of the CONCRETE x is the eager reduction, whose order of combination is not the fused
                # kernels': the two runs differ as a lazy and an eager run do, and are held to the bound tests/test_fused_rows.py has
                # for that comparison (test_softmax_cross_entropy_and_scale_gradient_gpu: 1e-6 / 1e-13 of the norm)
                tol = 1e-6 if dt == f32 else 1e-13
                on64, off64 = on.astype(np.float64), off.astype(np.float64)
                assert np.linalg.norm(on64 - off64) <= tol * np.linalg.norm(off64), (what, dt, np.linalg.norm(on64 - off64) / np.linalg.norm(off64))
            else:
                _same(on, off, f"{what} {dt.name}")
        x = _operands(nd, dt, 64, 260)[0]
        l0 = _launched(lib)
        p = _softmax(nd, x)
        assert _launched(lib) == l0, "nothing launches before the bytes are needed"
        p.get()
        assert _launched(lib) - l0 == 1


@gpu
def test_long_rows_take_the_composed_route_gpu(rows_nd, lib, on_gpu, generated):
    nd = rows_nd
    assert on_gpu
    xh = np.random.default_rng(0).standard_normal((256, 2052)).astype(np.float32)
    x = nd.asarray(xh)
    off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, x))
    assert s_on["vm_eval_rows"] == 0 and s_on == s_off
    _same(on, off, "rows of 2052")
    e = np.exp(xh.astype(np.float64) - xh.max(-1, keepdims=True))
    np.testing.assert_allclose(on, e / e.sum(-1, keepdims=True), rtol=2e-6, atol=0)


@gpu
@pytest.mark.parametrize("dt,tol", [(f32, 1e-6), (f64, 1e-13)], ids=["float32", "float64"])
def test_softmax_cross_entropy_through_the_tape_gpu(rows_nd, lib, on_gpu, generated, dt, tol):
    """(256, 64) logits, loss and logits' gradient: bit-equal to the switch-off lazy run, and against eager mode within the bound of
    tests/test_fused_rows.py::test_softmax_cross_entropy_and_scale_gradient_gpu (1e-6 / 1e-13 relative)."""
    nd = rows_nd
    assert on_gpu
    off, on, s_off, s_on = _both(nd, lambda: [nd.asarray(a) for a in _tape_softmax_xent(nd, dt, 256, 64)])
    assert s_on["vm_eval_rows"] == 1 and s_off["vm_eval_rows"] == 0, s_on       # the probabilities: max, row sum and chain in one launch
    _same(on[0], off[0], "loss")
    _same(on[1], off[1], "gradient")
    _same(on[2], off[2], "probabilities")
    nd.set_lazy(False)
    try:
        l_e, g_e, p_e = _tape_softmax_xent(nd, dt, 256, 64)
    finally:
        nd.set_lazy(True)
    l_e, g_e, l_l, g_l = l_e.astype(np.float64), g_e.astype(np.float64), on[0].astype(np.float64), on[1].astype(np.float64)
    assert abs(l_l - l_e) <= tol * abs(l_e), (dt, l_l, l_e)
    assert np.linalg.norm(g_l - g_e) <= tol * np.linalg.norm(g_e), (dt, np.linalg.norm(g_l - g_e) / np.linalg.norm(g_e))
    assert np.linalg.norm(on[2].astype(np.float64) - p_e) <= tol * np.linalg.norm(p_e.astype(np.float64))


@gpu
def test_refusals_compose_gpu(rows_nd, lib, on_gpu, generated, mdopt):
    nd = rows_nd
    assert on_gpu
    rng = np.random.default_rng(9)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)          # noqa: E731
    flat = nd.asarray(f(64 * 260 + 4))
    unaligned = nd.reshape(flat[1:1 + 64 * 260], (64, 260))
    strided = nd.asarray(f(64, 520))[:, ::2]
    x = nd.asarray(f(64, 260))

    def five():
        t = x
        for op in ("sum", "max", "min", "max", "sum"):
            t = nd.add(nd.multiply(t, 0.5), getattr(nd, op)(nd.multiply(x, t), axis=-1, keepdims=True))
        return t

    for what, make in (("an unaligned leaf", lambda: _softmax(nd, unaligned)), ("a strided inner axis", lambda: _softmax(nd, strided)),
                       ("five row statistics", five)):
        off, on, s_off, s_on = _both(nd, make)
        assert s_on["vm_eval_rows"] == 0, what
        _same(on, off, what)
    mdopt("jit", 0)
    off, on, s_off, s_on = _both(nd, lambda: _softmax(nd, x))
    assert s_on["vm_eval_rows"] == 0 and s_on == s_off
    _same(on, off, "jit off")
