"""Lazy mode, float16 loops: with the sub-switch on (MDHIP_LAZY_F16 / ndarray.set_lazy_float16) a call that NumPy
resolves to a float16 loop is recorded into a float32 program whose instruction carries MDHIP_VM_RND16 — the value is rounded to
binary16 once per recorded call, as NumPy's half loops (float32 arithmetic, one rounding) and the eager kernels of csrc/narrow.hip do.
That is NOT astype(float32 chain, float16), which rounds once at the end: every test below that compares bits also shows that its
inputs tell the two apart.

References: the SAME call with lazy mode off on the same build, and NumPy's own float16 result wherever NumPy is correctly rounded
(+ - * /, sqrt, abs, negative, maximum / minimum, comparisons, where, casts); transcendentals against the eager call only. Bits are
compared, a NaN matching any NaN. On the device the evaluations go through the C-ABI into a view inside a sentinel-filled base, and
the whole base is checked; operands are views inside sentinel bases too (the helpers of tests/test_fused_narrow.py).

  unmarked   the switch (off: today's route; on: pending, NumPy's dtype), (x * y) + z rounded per call, weak scalars, what
             md_vm_check refuses, mixing with float32 / float64 loops, astype(chain, float32) and the reductions behind it, the
             in-place write
  gpu        each case through the generated kernels (launches counted) and through the interpreter: all 65536 binary16 patterns,
             one geometry per evaluation kernel, the hoisted sin / cos, every reduction form, two consumers of one chain

Sums are taken over integer-valued products (|x|, |y| <= 50: a product above 2048 is not a binary16 and is rounded to an even
integer, so the per-call rounding shows) whose absolute values add up to less than 2^24: every partial sum is an exact float32
whatever the order, and the sums are compared exactly."""
import numpy as np
import pytest

from minidiff_amd import _capi

from test_fused_narrow import PAD, _bits, _dev, _eager, _launched, _run, _same, generated, lazy_nd, product  # noqa: F401  (fixtures)

gpu = pytest.mark.gpu
f16, f32, f64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)


@pytest.fixture
def half_nd(lazy_nd):
    """lazy mode with the float16 sub-switch on; both restored"""
    prev = lazy_nd.set_lazy_float16(True)
    yield lazy_nd
    lazy_nd.set_lazy_float16(prev)


def _rand16(rng, shape):
    return rng.standard_normal(shape).astype(f16)


def _per_call_and_once(x, y, z):
    """(x * y) + z as NumPy's float16 loops give it (rounded after each call) and rounded once at the end"""
    with np.errstate(all="ignore"):
        per_call = (x * y) + z
        once = (x.astype(f32) * y.astype(f32) + z.astype(f32)).astype(f16)
    assert per_call.dtype == f16
    return per_call, once


def _differ(a, b):
    return float((_bits(a) != _bits(b)).mean())


# ------------------------------------------------------------------------------------------------------------- both builds (unmarked)
def _operands(nd, rng, shape=(4, 8)):
    x16, y16 = _rand16(rng, shape), _rand16(rng, shape)
    i8 = rng.integers(-100, 100, shape).astype(np.int8)
    u8 = rng.integers(0, 5, shape).astype(np.uint8)
    m = rng.random(shape) < 0.5
    return (x16, y16, i8, u8, m), tuple(nd.asarray(v) for v in (x16, y16, i8, u8, m))


def test_switch_off_float16_loops_stay_eager(lazy_nd):
    """set_lazy(True) alone: float16 + float16, float16 * 2.0 and exp(uint8) launch at once, as before the switch existed"""
    nd = lazy_nd
    assert not nd.lazy_float16_enabled()
    _, (x16, y16, i8, u8, m) = _operands(nd, np.random.default_rng(4))
    for r in (nd.add(x16, x16), nd.multiply(x16, 2.0), nd.exp(u8), nd.where(m, x16, y16), nd.less(x16, 0.1)):
        assert r._expr is None and r._buf is not None


def test_switch_on_float16_loops_are_recorded(half_nd):
    """.. and with the switch on they are pending, with NumPy's dtype and NumPy's bits; int8 * int8 is still eager. The switch
    returns its previous setting and acts only while lazy mode is on."""
    nd = half_nd
    assert nd.lazy_float16_enabled() and nd.set_lazy_float16(True) is True
    (x, y, i, u, mk), (x16, y16, i8, u8, m) = _operands(nd, np.random.default_rng(4))
    with np.errstate(all="ignore"):
        cases = {
            "add(x16, x16)": (lambda: nd.add(x16, x16), x + x),
            "multiply(x16, 2.0)": (lambda: nd.multiply(x16, 2.0), x * 2.0),
            "exp(u8)": (lambda: nd.exp(u8), None),
            "sqrt(u8)": (lambda: nd.sqrt(u8), np.sqrt(u)),
            "where(m, x16, y16)": (lambda: nd.where(m, x16, y16), np.where(mk, x, y)),
            "less(x16, 0.1)": (lambda: nd.less(x16, 0.1), x < 0.1),
            "true_divide(b, b)": (lambda: nd.true_divide(m, m), np.true_divide(mk, mk)),
            "sin(b)": (lambda: nd.sin(m), None),
            "add(x16, i8)": (lambda: nd.add(x16, i8), x + i),
            "isnan(x16)": (lambda: nd.isnan(x16), np.isnan(x)),
        }
    for name, (make, ref) in cases.items():
        e = make()
        assert e._expr is not None and e._buf is None, f"{name}: launched eagerly"
        assert e._expr.cdt == (_capi.F64 if e.dtype == f64 else _capi.F32), name      # (bool / bool: float64 in NumPy 2, float16 before)
        eager = _eager(nd, make)
        assert e.dtype == eager.dtype, (name, e.dtype, eager.dtype)
        s0 = nd.FUSION_STATS["vm_eval"]
        got = e.get()
        assert nd.FUSION_STATS["vm_eval"] - s0 == 1, name
        _same(got, eager, f"{name} against the eager call")
        if ref is not None:
            _same(got, ref, f"{name} against NumPy")
    r = nd.multiply(i8, i8)
    assert r._expr is None and r._buf is not None and r.dtype == np.int8
    # the sub-switch without lazy mode does nothing
    prev = nd.set_lazy(False)
    try:
        r = nd.add(x16, x16)
        assert r._expr is None and r._buf is not None
    finally:
        nd.set_lazy(prev)


@pytest.mark.parametrize("n", [72, 65536], ids=["(6, 12)", "65536 values"])
def test_mul_add_rounds_after_each_call(half_nd, n):
    """(x * y) + z: one vm_eval, NumPy's per-call bits — on inputs that separate per-call rounding from rounding once in more than
    10 % of elements (the reference alone: 23 % on the large input), so a kernel that ignores MDHIP_VM_RND16 cannot pass"""
    nd = half_nd
    rng = np.random.default_rng(11)
    shape = (6, 12) if n == 72 else (n,)
    x, y, z = _rand16(rng, shape), _rand16(rng, shape), _rand16(rng, shape)
    per_call, once = _per_call_and_once(x, y, z)
    frac = _differ(per_call, once)
    print(f"(x * y) + z, {n} values: per-call and once-rounded differ in {100 * frac:.1f} % of elements")
    assert frac > 0.10
    dx, dy, dz = nd.asarray(x), nd.asarray(y), nd.asarray(z)
    make = lambda: nd.add(nd.multiply(dx, dy), dz)      # noqa: E731
    e = make()
    assert e._expr is not None and e._buf is None and e.dtype == f16 and e._expr.n == 2
    ctrl, _, _ = nd._lz.emit(e._expr)
    assert all(c & _capi.VM_RND16 for c in ctrl), [hex(c) for c in ctrl]
    s0 = nd.FUSION_STATS["vm_eval"]
    got = e.get()
    assert nd.FUSION_STATS["vm_eval"] - s0 == 1
    _same(got, per_call, "(x * y) + z against NumPy's float16 loops")
    _same(got, _eager(nd, make), "(x * y) + z against the eager calls")


def test_weak_scalars_are_float16_values(half_nd):
    """x16 * 0.1 multiplies by float16(0.1), x16 + 1e5 adds infinity, less(x16, 0.1) compares against float16(0.1)"""
    nd = half_nd
    rng = np.random.default_rng(12)
    x = _rand16(rng, (8, 16))
    x.ravel()[:4] = np.array([0.1, 0.09998, 0.10004, -0.1], dtype=f16)      # float16(0.1) itself and its neighbours
    dx = nd.asarray(x)
    with np.errstate(all="ignore"):
        refs = {
            "x * 0.1": (lambda: nd.multiply(dx, 0.1), x * 0.1),
            "x + 1e5": (lambda: nd.add(dx, 1e5), x + np.float16(np.inf)),
            "x + 70000": (lambda: nd.add(dx, 70000), x + np.float16(np.inf)),
            "less(x, 0.1)": (lambda: nd.less(dx, 0.1), x < 0.1),
            "0.1 - x": (lambda: nd.subtract(0.1, dx), 0.1 - x),
            "x * float16(0.3)": (lambda: nd.multiply(dx, np.float16(0.3)), x * np.float16(0.3)),
            "where(x < 0, 0.1, x)": (lambda: nd.where(nd.less(dx, 0), 0.1, dx), np.where(x < 0, np.float16(0.1), x)),
        }
    assert (x < 0.1).sum() != (x.astype(f32) < np.float32(0.1)).sum()       # the comparison tells float16(0.1) from float32(0.1)
    for name, (make, ref) in refs.items():
        e = make()
        assert e._expr is not None and e._buf is None, name
        got = e.get()
        _same(got, ref, f"{name} against NumPy")
        _same(got, _eager(nd, make), f"{name} against the eager call")


def test_md_vm_check_refuses_the_bit_where_it_means_nothing(half_nd, lib):
    """MDHIP_VM_RND16 under compute_dtype float64, on PUSH and on WHERE: ValueError; on UNARY / BINARY of a float32 program: accepted"""
    nd = half_nd
    x32 = nd.asarray(np.ones((4, 8), dtype=f32))
    m = nd.asarray(np.ones((4, 8), dtype=bool))
    out = nd.DeviceArray.empty((4, 8), np.float32)

    def program(e, flag_kind, cdt=None):
        prog, keep = nd._lz.build_program(e._expr, e.shape)
        hit = 0
        for i in range(prog.n_instr):
            if prog.ctrl[i] & 7 == flag_kind:
                prog.ctrl[i] |= _capi.VM_RND16
                hit += 1
        assert hit
        if cdt is not None:
            prog.compute_dtype = cdt
        return prog, keep

    unary, binary = nd.exp(nd.exp(x32)), nd.add(nd.exp(x32), x32)
    where = nd.where(m, nd.exp(x32), x32)
    for e, kind in ((unary, _capi.VM_UNARY), (binary, _capi.VM_BINARY)):
        prog, keep = program(e, kind)
        lib.vm_eval(prog, out.desc())
        ref = _eager(nd, lambda: nd.astype(nd.astype(nd.exp(nd.astype(nd.astype(nd.exp(x32), np.float16), np.float32)), np.float16), np.float32)) \
            if kind == _capi.VM_UNARY else None
        if ref is not None:
            _same(out.get(), ref, "exp(exp(x)) with both values rounded through binary16")
        prog, keep = program(e, kind, _capi.F64)
        with pytest.raises(ValueError, match="float32"):
            lib.vm_eval(prog, nd.DeviceArray.empty((4, 8), np.float64).desc())
    for e, kind in ((unary, _capi.VM_PUSH), (where, _capi.VM_WHERE)):
        prog, keep = program(e, kind)
        with pytest.raises(ValueError, match="binary16"):
            lib.vm_eval(prog, out.desc())
    assert _capi.vm_ctrl(_capi.VM_UNARY, 3, rnd16=True) == _capi.vm_ctrl(_capi.VM_UNARY, 3) | (1 << 18)


def _int_pair(rng, shape, axis=None):
    """integer-valued float16 operands whose products need the per-call rounding (module docstring)"""
    x, y = rng.integers(-50, 51, shape).astype(f16), rng.integers(-50, 51, shape).astype(f16)
    prod = x * y                                                # NumPy's float16 product: rounded
    exact = x.astype(np.int64) * y.astype(np.int64)
    assert (prod.astype(np.int64) != exact).any()               # the rounding shows ..
    assert np.abs(prod.astype(f64)).sum(axis=axis).max() < 2 ** 24   # .. and every partial sum of a reduced slice is exact
    return x, y, prod


def test_mixing_with_wider_loops(half_nd, on_gpu):
    """(x16 * y16) * w32 is ONE float32 program with the inner product rounded; + d64 materialises the float16 chain first;
    astype(x16 * y16, float32) is pending and launches nothing; sum of it — full, columns, rows — accumulates in float32"""
    nd = half_nd
    rng = np.random.default_rng(13)
    x, y, z = _rand16(rng, (8, 16)), _rand16(rng, (8, 16)), _rand16(rng, (8, 16))
    w, d = rng.standard_normal((8, 16)).astype(f32), rng.standard_normal((8, 16))
    dx, dy, dz, dw, dd = (nd.asarray(v) for v in (x, y, z, w, d))
    h = nd.multiply(dx, dy)
    e = nd.multiply(h, dw)
    assert e._buf is None and h._buf is None and e.dtype == f32 and e._expr.n == 2 and len(e._expr.leaves) == 3
    ctrl, _, _ = nd._lz.emit(e._expr)
    assert [bool(c & _capi.VM_RND16) for c in ctrl] == [True, False]
    s0 = nd.FUSION_STATS["vm_eval"]
    got = e.get()
    assert nd.FUSION_STATS["vm_eval"] - s0 == 1 and h._buf is None
    _same(got, (x * y) * w, "(x16 * y16) * w32 against NumPy")
    assert _differ(got, x.astype(f32) * y.astype(f32) * w) > 0.10
    # float64: another program type — the float16 chain is evaluated, then read as a leaf
    h = nd.multiply(dx, dy)
    e = nd.add(h, dd)
    assert h._buf is not None and e._buf is None and e.dtype == f64 and list(e._expr.leaves.values())[0] is h
    _same(e.get(), (x * y) + d, "(x16 * y16) + d64 against NumPy")
    # astype(chain, float32): the same expression
    h = nd.add(nd.multiply(dx, dy), dz)
    s0 = dict(nd.FUSION_STATS)
    a = nd.astype(h, np.float32)
    assert a._buf is None and h._buf is None and a._expr is h._expr and a.dtype == f32 and dict(nd.FUSION_STATS) == s0
    _same(a.get(), ((x * y) + z).astype(f32), "astype((x16 * y16) + z16, float32) against NumPy")
    assert h._buf is None
    _same(h.get(), (x * y) + z, "the chain itself, afterwards")
    # reductions behind the cast
    xi, yi, prod = _int_pair(rng, (16, 32))
    di, dj = nd.asarray(xi), nd.asarray(yi)
    for axis, stat in ((None, "vm_reduce"), (0, "vm_reduce"), (-1, "vm_reduce_rows")):
        h = nd.multiply(di, dj)
        s0 = nd.FUSION_STATS[stat]
        r = nd.sum(nd.astype(h, np.float32), axis=axis)
        if on_gpu or axis != -1:     # (the CPU double fuses full and column reductions only: a row sum evaluates the float32 array first)
            assert nd.FUSION_STATS[stat] - s0 == 1, (axis, stat)
        assert h._buf is None and r.dtype == f32, (axis, stat)
        _same(np.asarray(r.get()), np.asarray(prod.astype(f64).sum(axis=axis).astype(f32)), f"sum(astype(x16 * y16, float32), {axis})")
    # a reduction of the float16 chain itself stays on the eager route: the chain is evaluated, the eager kernel reduces it
    h = nd.multiply(di, dj)
    r = nd.max(h)
    assert h._buf is not None and r.dtype == f16 and float(r.get()) == float(prod.max())


def test_write_into_an_operand_evaluates_the_chain_first(half_nd):
    nd = half_nd
    rng = np.random.default_rng(14)
    x, y = _rand16(rng, (4, 8)), _rand16(rng, (4, 8))
    dx, dy = nd.asarray(x), nd.asarray(y)
    h = nd.multiply(dx, dy)
    assert h._buf is None
    nd.add(dx, 1, out=dx)
    assert h._buf is not None, "the write did not evaluate the pending chain"
    _same(h.get(), x * y, "x16 * y16 recorded before x16 += 1")
    _same(dx.get(), x + np.float16(1), "x16 += 1")


# ------------------------------------------------------------------------------------------------------------------------- device
@gpu
@pytest.mark.parametrize("chain", ["(x * w) + c", "sqrt(abs(x)) * w"])
def test_all_binary16_patterns_gpu(half_nd, lib, on_gpu, generated, chain):
    """every binary16 pattern as x, (256, 256), w = 0.3 and c = 1.5 as float16 arrays: NumPy's bits (subnormals, overflow to
    infinity, NaN as in the eager kernels); rounding once would differ on thousands of patterns"""
    nd = half_nd
    x = np.arange(65536, dtype=np.uint16).view(f16).reshape(256, 256)
    w, c = np.full((256, 256), 0.3, dtype=f16), np.full(256, 1.5, dtype=f16)
    dx, dw, dc = _dev(nd, x), _dev(nd, w), _dev(nd, c)
    with np.errstate(all="ignore"):
        if chain == "(x * w) + c":
            make = lambda: nd.add(nd.multiply(dx, dw), dc)      # noqa: E731
            ref, once = (x * w) + c, (x.astype(f32) * w.astype(f32) + c.astype(f32)).astype(f16)
        else:
            make = lambda: nd.multiply(nd.sqrt(nd.absolute(dx)), dw)      # noqa: E731
            ref, once = np.sqrt(np.abs(x)) * w, (np.sqrt(np.abs(x.astype(f32))) * w.astype(f32)).astype(f16)
    nan = np.isnan(ref)
    n_once = int(((_bits(ref) != _bits(once)) & ~nan).sum())
    print(f"{chain}: rounding once differs on {n_once} of 65536 patterns")
    assert n_once > 1000
    got = _run(nd, lib, make, 1 if generated else 0, what=chain)
    assert got.dtype == f16
    _same(got, ref, f"{chain} against NumPy")
    _same(got, _eager(nd, make), f"{chain} against the eager calls")


GEOMS = ["1-D", "rows", "three axes", "four axes", "(37, 45)", "off alignment", "bool"]


@gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_geometries_gpu(half_nd, lib, on_gpu, generated, geom):
    """maximum(x * w + b, 0) - z, one geometry per evaluation kernel (fast form with row vectors, three and four collapsed axes, the
    generic kernel for rows of 45 and for a view one element off its alignment), and less(x * w + b, z) with a bool result"""
    nd = half_nd
    rng = np.random.default_rng(15)
    shapes = {"1-D": ((4096,), (4096,), (4096,)), "rows": ((64, 256), (256,), (256,)), "three axes": ((8, 32, 256), (8, 1, 256), (1, 32, 1)),
              "four axes": ((4, 8, 8, 256), (1, 8, 1, 256), (1, 8, 1, 256)), "(37, 45)": ((37, 45), (45,), (37, 1)),
              "off alignment": ((1024,), (1024,), (1024,)), "bool": ((64, 256), (256,), (256,))}
    sx, sw, sb = shapes[geom]
    x, w, b, z = _rand16(rng, sx), _rand16(rng, sw), _rand16(rng, sb), _rand16(rng, sx)
    dx, dw, db, dz = _dev(nd, x, off=PAD + 1 if geom == "off alignment" else PAD), _dev(nd, w), _dev(nd, b), _dev(nd, z)
    if geom == "off alignment":
        assert (dx._buf.ptr + dx._offset * 2) % 8 != 0
    with np.errstate(all="ignore"):
        if geom == "bool":
            make = lambda: nd.less(nd.add(nd.multiply(dx, dw), db), dz)      # noqa: E731
            ref, once = (x * w + b) < z, (x.astype(f32) * w.astype(f32) + b.astype(f32)) < z.astype(f32)
        else:
            make = lambda: nd.subtract(nd.maximum(nd.add(nd.multiply(dx, dw), db), 0), dz)      # noqa: E731
            ref = np.maximum(x * w + b, 0) - z
            once = (np.maximum(x.astype(f32) * w.astype(f32) + b.astype(f32), 0) - z.astype(f32)).astype(f16)
    assert ref.dtype == (np.bool_ if geom == "bool" else f16) and (ref != once).any()
    l0 = _launched(lib)
    if geom == "(37, 45)":          # which kernel takes rows of 45 is the library's choice: the launches are not counted here
        e = make()
        assert e._expr is not None and e._buf is None
        got = e.get()
    else:
        got = _run(nd, lib, make, 0 if geom == "off alignment" or not generated else 1, what=geom)
    if not generated:
        assert _launched(lib) == l0
    _same(got, ref, f"{geom} against NumPy")
    _same(got, _eager(nd, make), f"{geom} against the eager calls")


@gpu
@pytest.mark.parametrize("chain", ["sin(x) * cos(x)", "sin(x) + x", "cos(x) - sin(x * x)"])
def test_hoisted_sin_cos_is_rounded_where_it_is_used_gpu(half_nd, lib, on_gpu, generated, chain):
    """sin / cos of a leaf are computed ahead of the generated body (one sincos when both occur): a flagged sin / cos must round the
    hoisted value; against the eager calls"""
    nd = half_nd
    x = (np.random.default_rng(16).standard_normal((64, 256)) * 3).astype(f16)
    dx = _dev(nd, x)
    make = {"sin(x) * cos(x)": lambda: nd.multiply(nd.sin(dx), nd.cos(dx)),
            "sin(x) + x": lambda: nd.add(nd.sin(dx), dx),
            "cos(x) - sin(x * x)": lambda: nd.subtract(nd.cos(dx), nd.sin(nd.multiply(dx, dx)))}[chain]
    got = _run(nd, lib, make, 1 if generated else 0, what=chain)
    _same(got, _eager(nd, make), f"{chain} against the eager calls")


RED_FORMS = {
    "full": ((64, 256), None, "vm_reduce"),
    "columns": ((512, 256), 0, "vm_reduce"),
    "rows, a wave per row": ((256, 512), -1, "vm_reduce_rows"),
    "rows, a block per row": ((300, 4096), -1, "vm_reduce_rows"),
    "middle axis": ((8, 64, 256), 1, "vm_reduce_axis"),
}


@gpu
@pytest.mark.parametrize("form", list(RED_FORMS))
@pytest.mark.parametrize("op", ["sum", "max"])
def test_reductions_behind_the_cast_gpu(half_nd, lib, on_gpu, generated, op, form):
    """op(astype(x16 * y16, float32)) in the form's one pass, the chain still pending: max bit-equal to the eager route, sum exact
    (module docstring) against the float64 sum of NumPy's float16 product"""
    nd = half_nd
    shape, axis, stat = RED_FORMS[form]
    x, y, prod = _int_pair(np.random.default_rng(17), shape, axis)
    dx, dy = _dev(nd, x), _dev(nd, y)
    make = lambda: getattr(nd, op)(nd.astype(nd.multiply(dx, dy), np.float32), axis=axis)      # noqa: E731
    h = nd.multiply(dx, dy)
    s0, l0 = nd.FUSION_STATS[stat], _launched(lib)
    r = getattr(nd, op)(nd.astype(h, np.float32), axis=axis)
    assert nd.FUSION_STATS[stat] - s0 == 1, f"{op}, {form}: not fused"
    assert _launched(lib) - l0 == (1 if generated else 0), f"{op}, {form}: {_launched(lib) - l0} generated launches"
    assert h._buf is None and r.dtype == f32
    got = np.asarray(r.get())
    _same(got, np.asarray(getattr(np, op)(prod.astype(f64), axis=axis).astype(f32)), f"{op}, {form}, against NumPy's float16 product")
    _same(got, np.asarray(_eager(nd, make)), f"{op}, {form}, against the eager route")


@gpu
def test_two_consumers_and_a_float32_consumer_gpu(half_nd, lib, on_gpu, generated):
    """h = x16 * y16 consumed twice: both consumers recompute it and agree with NumPy; consumed by a float32 program it gives the
    bits of materialising it first"""
    nd = half_nd
    rng = np.random.default_rng(18)
    x, y, z = _rand16(rng, (64, 256)), _rand16(rng, (64, 256)), _rand16(rng, (64, 256))
    w = rng.standard_normal(256).astype(f32)
    dx, dy, dz, dw = _dev(nd, x), _dev(nd, y), _dev(nd, z), _dev(nd, w)
    h = nd.multiply(dx, dy)
    a, b = nd.add(h, dz), nd.subtract(h, dz)
    _same(a.get(), (x * y) + z, "first consumer")
    _same(b.get(), (x * y) - z, "second consumer")
    assert h._buf is None
    joined = _run(nd, lib, lambda: nd.multiply(nd.multiply(dx, dy), dw), 1 if generated else 0, what="(x16 * y16) * w32")
    h = nd.multiply(dx, dy).materialize()
    first = nd.multiply(h, dw).get()
    _same(joined, first, "(x16 * y16) * w32: joined against materialised first")
    _same(joined, (x * y) * w, "(x16 * y16) * w32 against NumPy")


def test_generated_kernels_compile_with_the_bit(half_nd, product):
    """every generated kind for a flagged chain — dense, row-broadcast and column-broadcast float16 leaves, a hoisted sin and cos next
    to computed ones — compiles (no device needed), and carries another name than its unflagged twin: the cache signature holds the
    whole ctrl words"""
    nd = half_nd
    plib, log = product
    x2, r2, c2 = nd.asarray(np.ones((8, 16), f16)), nd.asarray(np.ones((8, 1), f16)), nd.asarray(np.ones(16, f16))
    x3, g3 = nd.asarray(np.ones((2, 8, 16), f16)), nd.asarray(np.ones((2, 1, 16), f16))

    def chains():
        e2 = nd.add(nd.multiply(nd.multiply(nd.sin(x2), nd.cos(x2)), r2), nd.sin(nd.multiply(x2, c2)))
        e3 = nd.multiply(nd.add(nd.sin(x3), x3), g3)
        return (nd.astype(e2, np.float32), nd.astype(e3, np.float32)) if e2.dtype == f16 else (e2, e3)

    names = {}
    for flagged in (True, False):
        prev = nd.set_lazy_float16(flagged)
        try:
            if flagged:
                e2, e3 = chains()
            else:       # the same chain over float32 copies of the leaves' values: same instructions, no bit
                x2, r2, c2, x3, g3 = (nd.astype(v, np.float32) for v in (x2, r2, c2, x3, g3))
                e2, e3 = chains()
        finally:
            nd.set_lazy_float16(prev)
        assert e2._buf is None and e3._buf is None
        p2, k2 = nd._lz.build_program(e2._expr, e2.shape)
        p3, k3 = nd._lz.build_program(e3._expr, e3.shape)
        assert any(p2.ctrl[i] & _capi.VM_RND16 for i in range(p2.n_instr)) == flagged
        for kind in (range(10) if flagged else (0, 5)):      # (the twin: both eval forms are enough to compare names)
            plib.vm_jit_probe(p3 if kind in (5, 8, 9) else p2, kind, _capi.R_SUM, 0, log, len(log))      # raises with the compiler's log
            names.setdefault(kind, []).append(log.value.split(b"\n")[0])
    for kind in (0, 5):
        a, b = names[kind]
        assert a != b and a.startswith(b"k_fused_eval") and b.startswith(b"k_fused_eval"), (kind, a, b)
