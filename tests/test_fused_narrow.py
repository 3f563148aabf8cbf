"""Lazy mode: chains that READ storage-only arrays (float16, int8/16, uint8/16/32/64) and chains STORED as float16.

A storage-only operand is a leaf of a fused program whenever NumPy's loop for the call is float32 / float64: it is read in its own
type and converted on load. astype(narrow, float32 | float64) is such a leaf by itself; astype(pending chain, float16) stores the
chain's value as float16 in the same pass (one rounding).

References: the SAME call with lazy mode off on the same build (that route is untouched and pinned to NumPy elsewhere), and NumPy
itself wherever NumPy is correctly rounded (+ - * /, comparisons, where, casts). Everything is compared as raw bits, a NaN
matching any NaN. On the device the evaluations go through the C-ABI into a view inside a sentinel-filled base of this module's
own, and the whole base is checked; operands are views inside sentinel bases too.

  unmarked   the forms are pending, materialise in one vm_eval without a convert call, every leaf dtype in float32 and float64
             programs, a full and a column reduction per dtype, the in-place write, the float16 store offered and refused (double)
  gpu        each case through the generated kernels (jit = 1, jit_min = 1, launches counted) and through the interpreter (jit = 0):
             all 65536 two-byte patterns, all byte values, the uint32 / uint64 edges, one geometry per kernel, the four reductions
             in every reduction form, two programs sharing a float16 leaf, the float16 store at every midpoint."""
import ctypes as C

import numpy as np
import pytest

from minidiff_amd import _capi

from test_fused_axis import _chain_length as _cols_chain_length, _nb, _ru      # the column kernels' geometry, as derived there
from test_fused_rows import _chain_length as _rows_chain_length                 # .. and the row kernels'

gpu = pytest.mark.gpu
f16, f32, f64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
NARROW = [np.dtype(t) for t in (np.float16, np.int8, np.uint8, np.int16, np.uint16, np.uint32, np.uint64)]
PAD = 16            # sentinel elements in front of and behind every view: a multiple of 16 B for every element size
SENT = -777.0       # output sentinel (exact in float16)
CODES = {"sum": _capi.R_SUM, "prod": _capi.R_PROD, "max": _capi.R_MAX, "min": _capi.R_MIN}


@pytest.fixture
def lazy_nd(lib):
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(True)
    yield nd
    nd.set_lazy(prev)


@pytest.fixture(params=["generated", "interpreter"])
def generated(request, mdopt):
    """True: the hiprtc-compiled kernels at any size; False: the interpreter kernels."""
    mdopt("jit_min", 1)
    mdopt("jit", 1 if request.param == "generated" else 0)
    return request.param == "generated"


def _launched(lib):
    st = (C.c_int64 * 2)()
    lib.vm_jit_stats(st)
    return int(st[1])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, exp, what):
    """bit for bit; a NaN matches any NaN"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} against {exp.dtype}{exp.shape}"
    if got.dtype.kind == "f":
        gn, en = np.isnan(got), np.isnan(exp)
        bad = (gn != en) | (~en & (_bits(got) != _bits(exp)))
    else:
        bad = _bits(got) != _bits(exp)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {i}: {got[i]!r} against {exp[i]!r}")


def _eager(nd, make):
    prev = nd.set_lazy(False)
    try:
        return make().get()
    finally:
        nd.set_lazy(prev)


def _in_sentinel(dt):
    return np.nan if dt.kind == "f" else (1 if dt.kind == "b" else 0x5A)


def _dev(nd, a, off=PAD):
    """`a` on the device as a dense view that starts `off` elements into a sentinel base (off = PAD: aligned for every vector load)"""
    a = np.ascontiguousarray(a)
    base = np.full(a.size + off + PAD, _in_sentinel(a.dtype), dtype=a.dtype)
    base[off:off + a.size] = a.ravel()
    return nd.asarray(base)._view(off, a.shape, nd._c_strides(a.shape))


def _run(nd, lib, make, launches, odt=None, what=""):
    """The evaluation of a pending array as DeviceArray._materialize makes it, into a view inside a sentinel base of this module's
    own: -> the values; the base around them must be untouched and `launches` generated kernels launched."""
    e = make()
    assert e._expr is not None and e._buf is None, f"{what}: should be pending"
    odt = np.dtype(odt or e.dtype)
    prog, keep = nd._lz.build_program(e._expr, e.shape)
    base = nd.asarray(np.full(e.size + 2 * PAD, SENT, dtype=odt))
    view = base._view(PAD, e.shape, nd._c_strides(e.shape))
    l0 = _launched(lib)
    lib.vm_eval(prog, view.desc())
    assert _launched(lib) - l0 == launches, f"{what}: {_launched(lib) - l0} generated launches, {launches} expected"
    del keep
    whole = base.get()
    pad = np.full(PAD, SENT, dtype=odt)
    assert np.array_equal(_bits(whole[:PAD]), _bits(pad)) and np.array_equal(_bits(whole[-PAD:]), _bits(pad)), f"{what}: wrote outside the view"
    return whole[PAD:-PAD].reshape(e.shape)


def _values(dt, n, rng):
    """n values of a storage-only dtype: random bit patterns (float16: every class of value; integers: the whole range) with the
    extremes planted"""
    bits = rng.integers(0, 1 << (8 * dt.itemsize), n, dtype=np.uint64).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize])
    v = bits.view(dt).copy()
    if dt.kind == "f":
        edge = np.array([0x0000, 0x8000, 0x0001, 0x03FF, 0x0400, 0x7BFF, 0x7C00, 0xFC00, 0x7E00, 0xFBFF], dtype=np.uint16).view(f16)
    else:
        info = np.iinfo(dt)
        edge = np.array([info.min, info.max, 0, 1, info.max // 2 + 1], dtype=dt)
    v[:min(n, edge.size)] = edge[:n]
    return v


# ------------------------------------------------------------------------------------------------------------- both builds (unmarked)
def _forms(nd, rng, shape=(6, 12)):
    x16 = rng.standard_normal(shape).astype(f16)
    y32 = rng.standard_normal(shape).astype(f32)
    m = rng.random(shape) < 0.5
    i16 = rng.integers(-30000, 30000, shape).astype(np.int16)
    u8 = rng.integers(0, 256, shape).astype(np.uint8)
    dx, dy, dm, di, du = (nd.asarray(v) for v in (x16, y32, m, i16, u8))
    return {
        "multiply(x16, y32)": (lambda: nd.multiply(dx, dy), x16.astype(f32) * y32),
        "where(m, x16, y32)": (lambda: nd.where(dm, dx, dy), np.where(m, x16, y32)),
        "sin(i16)": (lambda: nd.sin(di), None),
        "true_divide(u8, 255.0)": (lambda: nd.true_divide(du, 255.0), u8 / 255.0),
        "astype(x16, float32)": (lambda: nd.astype(dx, np.float32), x16.astype(f32)),
        "less(x16, y32)": (lambda: nd.less(dx, dy), x16 < y32),
    }


FORM_NAMES = ["multiply(x16, y32)", "where(m, x16, y32)", "sin(i16)", "true_divide(u8, 255.0)", "astype(x16, float32)", "less(x16, y32)"]


@pytest.mark.parametrize("form", FORM_NAMES)
def test_storage_only_operands_stay_pending(lazy_nd, monkeypatch, form):
    """Calls whose loop is float32 / float64 are recorded although an operand is storage-only (on the parent commit each of them
    launched at once); materialising is ONE vm_eval and no conversion pass; the bits are the eager call's and NumPy's."""
    nd = lazy_nd
    make, ref = _forms(nd, np.random.default_rng(3))[form]
    converts = []
    real = nd._lib().convert
    monkeypatch.setattr(nd._lib(), "convert", lambda *a: (converts.append(1), real(*a))[1])
    e = make()
    assert e._expr is not None and e._buf is None, f"{form}: launched eagerly"
    s0 = nd.FUSION_STATS["vm_eval"]
    got = e.get()
    assert nd.FUSION_STATS["vm_eval"] - s0 == 1 and not converts, (form, nd.FUSION_STATS["vm_eval"] - s0, len(converts))
    monkeypatch.undo()
    _same(got, _eager(nd, make), f"{form} against the eager call")
    if ref is not None:
        _same(got, ref, f"{form} against NumPy")


def test_storage_only_loops_stay_eager(lazy_nd):
    """loops whose dtype is storage-only itself are not recorded: float16 + float16, int8 * int8, exp(uint8), float16 * 2.0"""
    nd = lazy_nd
    rng = np.random.default_rng(4)
    x16 = nd.asarray(rng.standard_normal((4, 8)).astype(f16))
    i8 = nd.asarray(rng.integers(-100, 100, (4, 8)).astype(np.int8))
    u8 = nd.asarray(rng.integers(0, 5, (4, 8)).astype(np.uint8))
    for r, dt in ((nd.add(x16, x16), f16), (nd.multiply(i8, i8), np.int8), (nd.exp(u8), f16), (nd.multiply(x16, 2.0), f16),
                  (nd.astype(x16, np.int32), np.int32), (nd.astype(i8, np.float16), f16)):
        assert r._expr is None and r._buf is not None and r.dtype == dt, (r.dtype, dt)


@pytest.mark.parametrize("wide", [f32, f64], ids=["w32", "w64"])
@pytest.mark.parametrize("dt", NARROW, ids=[d.name for d in NARROW])
def test_every_leaf_dtype_in_a_two_instruction_program(lazy_nd, dt, wide):
    """x * w + b with x of every storage-only dtype and w, b float32 / float64: the program computes in NumPy's loop dtype for the
    pair (float32 only where the narrow type fits it) and gives NumPy's bits (* and + are correctly rounded)."""
    nd = lazy_nd
    rng = np.random.default_rng(5)
    shape = (5, 12)
    x = _values(dt, 60, rng).reshape(shape)
    w, b = rng.standard_normal(shape).astype(wide), rng.standard_normal(shape).astype(wide)
    dx, dw, db = nd.asarray(x), nd.asarray(w), nd.asarray(b)
    make = lambda: nd.add(nd.multiply(dx, dw), db)      # noqa: E731
    e = make()
    assert e._expr is not None and e._buf is None and e._expr.n == 2 and len(e._expr.leaves) == 3
    with np.errstate(all="ignore"):
        ref = x * w + b
    assert e.dtype == ref.dtype == np.result_type(dt, wide)
    got = e.get()
    _same(got, ref, f"{dt.name} in a {ref.dtype.name} program against NumPy")
    _same(got, _eager(nd, make), f"{dt.name} in a {ref.dtype.name} program against the eager calls")


@pytest.mark.parametrize("dt", NARROW, ids=[d.name for d in NARROW])
def test_full_and_column_reduction_per_leaf_dtype(lazy_nd, dt):
    """sum(x * w) over everything and over axis 0 with a storage-only x: fused (vm_reduce), the operand stays pending; integer-valued
    operands, so the sums are exact whatever the order"""
    nd = lazy_nd
    rng = np.random.default_rng(6)
    shape = (9, 12)
    x = rng.integers(0 if dt.kind == "u" else -9, 10, shape).astype(dt)
    w = rng.integers(-4, 5, shape).astype(f32)
    dx, dw = nd.asarray(x), nd.asarray(w)
    prods = x.astype(np.int64) * w.astype(np.int64)
    for axis, ref in ((None, prods.sum()), (0, prods.sum(axis=0))):
        e = nd.multiply(dx, dw)
        assert e._expr is not None and e._buf is None
        s0 = nd.FUSION_STATS["vm_reduce"]
        r = nd.sum(e, axis=axis)
        got = r.get()
        assert nd.FUSION_STATS["vm_reduce"] - s0 == 1 and e._buf is None, (dt.name, axis)
        assert got.dtype == np.result_type(dt, f32)
        assert np.array_equal(got.astype(np.int64), ref), (dt.name, axis, got, ref)


def test_a_write_into_the_source_flushes_the_pending_cast(lazy_nd):
    """y = astype(x16, float32) reads x16 when it is evaluated: an in-place write into x16 evaluates y first"""
    nd = lazy_nd
    x = np.random.default_rng(7).standard_normal((4, 8)).astype(f16)
    dx = nd.asarray(x)
    y = nd.astype(dx, np.float32)
    assert y._expr is not None and y._buf is None
    nd.multiply(dx, 0, out=dx)
    assert y._buf is not None, "the write did not evaluate the pending cast"
    _same(y.get(), x.astype(f32), "astype(x16, float32) after x16 *= 0")
    assert not dx.get().any()
    # .. and a consumer of the pending cast reads x16 itself (no float copy): it is flushed by the write as well
    dx = nd.asarray(x)
    z = nd.add(nd.astype(dx, np.float32), 1.0)
    assert z._buf is None and list(z._expr.leaves.values())[0] is dx
    nd.multiply(dx, 0, out=dx)
    _same(z.get(), x.astype(f32) + np.float32(1.0), "astype(x16, float32) + 1 after x16 *= 0")


def test_the_pending_cast_never_aliases_its_source(lazy_nd):
    nd = lazy_nd
    x = np.arange(32, dtype=np.uint8).reshape(4, 8)
    dx = nd.asarray(x)
    y = nd.astype(dx, np.float64)
    got = y.get()
    assert y._buf is not None and y._buf is not dx._buf and y.dtype == f64
    _same(got, x.astype(f64), "astype(u8, float64)")
    s = nd.sum(nd.astype(dx, np.float64))        # a reduction of the root leaf: fused, exact
    assert float(s.get()) == float(x.sum())


@pytest.mark.parametrize("wide", [f32, f64], ids=["f32", "f64"])
def test_float16_store_is_offered_and_the_double_refuses_cpu(lazy_nd, on_gpu, monkeypatch, wide):
    """astype(pending chain, float16): mdhip_vm_eval is called with a float16 `out` (not on the parent commit); the double checks the
    dtype and refuses, and the fallback — evaluate, then convert — gives NumPy's float16"""
    if on_gpu:
        pytest.skip("other twin")
    nd = lazy_nd
    rng = np.random.default_rng(8)
    x, w = (rng.standard_normal((6, 12)) * 100).astype(wide), rng.standard_normal((6, 12)).astype(wide)
    dx, dw = nd.asarray(x), nd.asarray(w)
    offered = []
    real = nd._lib().vm_eval

    def spy(prog, out):
        offered.append(int(out.dtype))
        return real(prog, out)

    monkeypatch.setattr(nd._lib(), "vm_eval", spy)
    e = nd.multiply(dx, dw)
    assert e._buf is None
    r = nd.astype(e, np.float16)
    assert offered[0] == _capi.F16 and offered[1:] == [_capi.F32 if wide == f32 else _capi.F64], offered
    _same(r.get(), (x * w).astype(f16), "astype(chain, float16) through the fallback")


@pytest.fixture(scope="module")
def product():
    import os
    if not os.path.exists(_capi.PRODUCT_LIB):
        pytest.skip("libmdhip.so not built")
    return _capi.Library(_capi.PRODUCT_LIB), C.create_string_buffer(4096)      # dlopen only: the compile-only probe needs no GPU


def test_generated_kernels_compile_for_storage_only_leaves(lazy_nd, product):
    """every generated kind with a dense, a row-broadcast and a column-broadcast leaf of float16 / uint8 / uint64 (a 2-byte struct, the
    uint8 value type next to bool's uint8_t, an 8-byte type: the three ways the generated loads differ), the plain eval for the other
    four, and the float16 store from float32 and float64 in both eval forms"""
    nd = lazy_nd
    plib, log = product
    n = 0
    for dt in NARROW:
        wide = f32 if dt.itemsize < 4 else f64
        x2, r2, c2 = nd.asarray(np.ones((8, 16), dt)), nd.asarray(np.ones((8, 1), dt)), nd.asarray(np.ones(16, dt))
        w2 = nd.asarray(np.ones((8, 16), wide))
        e2 = nd.add(nd.multiply(nd.multiply(x2, w2), r2), c2)
        x3, g3, w3 = nd.asarray(np.ones((2, 8, 16), dt)), nd.asarray(np.ones((2, 1, 16), dt)), nd.asarray(np.ones((2, 8, 16), wide))
        e3 = nd.multiply(nd.multiply(x3, w3), g3)
        assert e2._buf is None and e3._buf is None
        p2, k2 = nd._lz.build_program(e2._expr, e2.shape)
        p3, k3 = nd._lz.build_program(e3._expr, e3.shape)
        kinds = range(10) if dt in (f16, np.dtype(np.uint8), np.dtype(np.uint64)) else (0,)
        for kind in kinds:
            plib.vm_jit_probe(p3 if kind in (5, 8, 9) else p2, kind, _capi.R_SUM, 0, log, len(log))      # raises with the compiler's log
            n += 1
    for wide in (f32, f64):
        a, b = nd.asarray(np.ones((2, 8, 16), wide)), nd.asarray(np.ones((2, 1, 16), wide))
        e = nd.multiply(a, b)
        p, k = nd._lz.build_program(e._expr, e.shape)
        for kind, tag in ((0, b"k_fused_evalh_"), (5, b"k_fused_evalaxesh_")):
            plib.vm_jit_probe(p, kind, 0, 2, log, len(log))
            assert log.value.startswith(tag), log.value[:40]
            n += 1
    assert n == 38


# ------------------------------------------------------------------------------------------------------------------------- device
TWO_BYTE = [f16, np.dtype(np.int16), np.dtype(np.uint16)]


@gpu
@pytest.mark.parametrize("geom", ["1-D", "2-D", "axes"])
@pytest.mark.parametrize("wide", [f32, f64], ids=["w32", "w64"])
@pytest.mark.parametrize("dt", TWO_BYTE, ids=[d.name for d in TWO_BYTE])
def test_all_two_byte_patterns_gpu(lazy_nd, lib, on_gpu, generated, dt, wide, geom):
    """all 65536 patterns of a two-byte leaf as one (8, 32, 256) array — exactly the 2^16 elements k_vm_eval_axes needs — times a
    float32 / float64 operand: dense 1-D, 2-D against a (C,) row, three axes against a (B, 1, C) broadcast"""
    nd = lazy_nd
    x = np.arange(65536, dtype=np.uint16).view(dt)
    rng = np.random.default_rng(10)
    if geom == "1-D":
        g = rng.standard_normal(65536).astype(wide)
    elif geom == "2-D":
        x, g = x.reshape(256, 256), rng.standard_normal(256).astype(wide)
    else:
        x, g = x.reshape(8, 32, 256), rng.standard_normal((8, 1, 256)).astype(wide)
    dx, dg = _dev(nd, x), _dev(nd, g)
    make = lambda: nd.multiply(dx, dg)      # noqa: E731
    got = _run(nd, lib, make, 1 if generated else 0, what=f"{dt.name} {geom}")
    with np.errstate(all="ignore"):
        ref = x * g
    _same(got, ref, f"{dt.name} x {wide.name}, {geom}, against NumPy")
    _same(got, _eager(nd, make), f"{dt.name} x {wide.name}, {geom}, against the eager call")


ONE_BYTE = [np.dtype(np.int8), np.dtype(np.uint8)]


@gpu
@pytest.mark.parametrize("wide", [f32, f64], ids=["w32", "w64"])
@pytest.mark.parametrize("dt", ONE_BYTE, ids=[d.name for d in ONE_BYTE])
def test_all_byte_values_gpu(lazy_nd, lib, on_gpu, generated, dt, wide):
    """all 256 values of a one-byte leaf, tiled: 2-D (4-byte vector loads) and 1-D with a tail"""
    nd = lazy_nd
    rng = np.random.default_rng(11)
    x = np.tile(np.arange(256, dtype=np.uint8).view(dt), 8)
    for shape, gshape in (((8, 256), (256,)), ((2051,), (2051,))):
        xs = np.resize(x, shape)
        g = rng.standard_normal(gshape).astype(wide)
        dx, dg = _dev(nd, xs), _dev(nd, g)
        make = lambda: nd.subtract(nd.true_divide(dx, dg), 0.5)      # noqa: E731
        got = _run(nd, lib, make, 1 if generated else 0, what=f"{dt.name} {shape}")
        _same(got, xs / g - wide.type(0.5), f"{dt.name} / {wide.name} - 0.5, {shape}, against NumPy")
        _same(got, _eager(nd, make), f"{dt.name} / {wide.name} - 0.5, {shape}, against the eager calls")


@gpu
@pytest.mark.parametrize("dt", [np.dtype(np.uint32), np.dtype(np.uint64)], ids=["uint32", "uint64"])
def test_wide_unsigned_edges_gpu(lazy_nd, lib, on_gpu, generated, dt):
    """uint32 / uint64 leaves of float64 programs: 0, 2^32 - 1, 2^53 + 1 (a tie: to even), 2^63 and 2^64 - 1 — one rounding from the
    unsigned value, never through int64"""
    nd = lazy_nd
    edges = [0, 1, 2**31, 2**32 - 1] + ([2**53 + 1, 2**53 + 3, 2**63 - 1, 2**63, 2**63 + 1025, 2**64 - 1] if dt.itemsize == 8 else [])
    rng = np.random.default_rng(12)
    for shape in ((1027,), (4, 256), (8, 32, 256)):
        x = np.resize(np.array(edges, dtype=dt), shape)
        n = x.size
        x.ravel()[rng.integers(0, n, n // 2)] = _values(dt, n // 2, rng)
        g = rng.standard_normal(shape[-1] if len(shape) < 3 else (8, 1, 256))
        dx, dg = _dev(nd, x), _dev(nd, g)
        make = lambda: nd.add(dx, dg)      # noqa: E731
        got = _run(nd, lib, make, 1 if generated else 0, what=f"{dt.name} {shape}")
        assert got.dtype == f64
        _same(got, x + g, f"{dt.name} + float64, {shape}, against NumPy")
        _same(got, _eager(nd, make), f"{dt.name} + float64, {shape}, against the eager call")


GEOMS = ["1-D, 4k", "1-D, 4k + 1", "1-D, 4k + 2", "1-D, 4k + 3", "(R,1) and (C,) narrow", "sliced 3-D view", "(B,1,C) narrow",
         "[::2] view", "off its alignment by one element"]


@gpu
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("dt", [f16, np.dtype(np.uint8), np.dtype(np.uint64)], ids=["float16", "uint8", "uint64"])
def test_geometries_gpu(lazy_nd, lib, on_gpu, generated, dt, geom):
    """one geometry per evaluation kernel: vector body + tail, row and column broadcasts of NARROW leaves, the axes form over a
    sliced view and with a narrow (B,1,C) leaf, and the two that must take the generic kernel (no generated form: 0 launches)"""
    nd = lazy_nd
    rng = np.random.default_rng(13)
    wide = f32 if dt.itemsize < 4 else f64
    jit = 1 if generated else 0
    if geom.startswith("1-D"):
        n = 1024 + int(geom[-1]) if geom[-1] != "k" else 1024
        x, y = _values(dt, n, rng), rng.standard_normal(n).astype(wide)
        dx, dy = _dev(nd, x), _dev(nd, y)
        make, ref = (lambda: nd.multiply(dx, dy)), lambda: x * y
    elif geom == "(R,1) and (C,) narrow":
        a, xr, xc = rng.standard_normal((24, 40)).astype(wide), _values(dt, 24, rng).reshape(24, 1), _values(dt, 40, rng)
        da, dr, dc = _dev(nd, a), _dev(nd, xr), _dev(nd, xc)
        make, ref = (lambda: nd.add(nd.multiply(da, dr), dc)), lambda: a * xr + xc
    elif geom == "sliced 3-D view":
        xb, y = _values(dt, 8 * 32 * 260, rng).reshape(8, 32, 260), rng.standard_normal((8, 32, 256)).astype(wide)
        db, dy = _dev(nd, xb), _dev(nd, y)
        dx = db._view(db._offset, (8, 32, 256), db._strides)
        x = xb[:, :, :256]
        make, ref = (lambda: nd.multiply(dx, dy)), lambda: x * y
    elif geom == "(B,1,C) narrow":
        a, x = rng.standard_normal((8, 32, 256)).astype(wide), _values(dt, 8 * 256, rng).reshape(8, 1, 256)
        da, dx = _dev(nd, a), _dev(nd, x)
        make, ref = (lambda: nd.multiply(da, dx)), lambda: a * x
    elif geom == "[::2] view":
        xb, y = _values(dt, 2048, rng), rng.standard_normal(1024).astype(wide)
        db, dy = _dev(nd, xb), _dev(nd, y)
        dx = db._view(db._offset, (1024,), (2,))
        x = xb[::2]
        make, ref, jit = (lambda: nd.multiply(dx, dy)), (lambda: x * y), 0
    else:
        x, y = _values(dt, 1024, rng), rng.standard_normal(1024).astype(wide)
        dx, dy = _dev(nd, x, off=PAD + 1), _dev(nd, y)
        assert (dx._buf.ptr + dx._offset * dt.itemsize) % min(16, 4 * dt.itemsize) != 0
        make, ref, jit = (lambda: nd.multiply(dx, dy)), (lambda: x * y), 0
    got = _run(nd, lib, make, jit, what=f"{dt.name}, {geom}")
    with np.errstate(all="ignore"):
        _same(got, ref(), f"{dt.name}, {geom}, against NumPy")
    _same(got, _eager(nd, make), f"{dt.name}, {geom}, against the eager calls")


# ---- reductions of a chain with a narrow leaf ----
# form -> (shape, axis, the counter of ndarray.FUSION_STATS that must move)
RED_FORMS = {
    "full": ((4099,), None, "vm_reduce"),
    "columns, tiled (n_red 256)": ((256, 64), 0, "vm_reduce"),
    "columns, strips (n_red 640)": ((640, 64), 0, "vm_reduce"),
    "eval + column reduction": ((512, 1024), 0, "vm_eval_reduce_cols"),
    "rows, a wave per row": ((64, 256), -1, "vm_reduce_rows"),
    "rows, a block per row": ((256, 2052), -1, "vm_reduce_rows"),
    "middle axis": ((2, 64, 256), 1, "vm_reduce_axis"),
}


def _reduce_fused(nd, lib, generated, make, op, form, what):
    """op(pending chain) in the form's one pass -> (result, the evaluated chain or None)"""
    shape, axis, stat = RED_FORMS[form]
    e = make()
    assert e._expr is not None and e._buf is None and e.shape == shape, f"{what}: the chain should be pending"
    l0 = _launched(lib)
    if form == "eval + column reduction":
        if not generated:
            stat = "vm_eval"        # the one-pass kernel is a generated one: without it the two passes run separately
        d0 = nd.FUSION_STATS["deferred_cols"]
        r = getattr(nd, op)(e, axis=axis)
        assert nd.FUSION_STATS["deferred_cols"] - d0 == 1, f"{what}: the column reduction was not owed"
        s0 = nd.FUSION_STATS[stat]
        val = e.get()
        assert nd.FUSION_STATS[stat] - s0 == 1, f"{what}: {stat} did not move"
        got = r.get()
        if generated:
            assert _launched(lib) - l0 == 1, f"{what}: {_launched(lib) - l0} generated launches"
        return got, val
    s0 = nd.FUSION_STATS[stat]
    r = getattr(nd, op)(e, axis=axis)
    assert nd.FUSION_STATS[stat] - s0 == 1, f"{what}: not fused"
    assert _launched(lib) - l0 == (1 if generated else 0), f"{what}: {_launched(lib) - l0} generated launches"
    assert e._buf is None, f"{what}: the reduction materialised its operand"
    return r.get(), None


RED_LEAVES = [f16, np.dtype(np.int8)]


@gpu
@pytest.mark.parametrize("form", list(RED_FORMS))
@pytest.mark.parametrize("op", ["sum", "prod", "max", "min"])
@pytest.mark.parametrize("dt", RED_LEAVES, ids=[d.name for d in RED_LEAVES])
def test_exact_reductions_gpu(lazy_nd, lib, on_gpu, generated, dt, op, form):
    """op(x * w) with a narrow x, exact whatever the order: sums of integer-valued products (below 2^24), products of +-2^k factors,
    max / min with the extreme planted in the first and in the last element of the array"""
    nd = lazy_nd
    shape, axis, _ = RED_FORMS[form]
    rng = np.random.default_rng(14)
    n = int(np.prod(shape))
    if op == "sum":
        x, w = rng.integers(-8, 9, shape).astype(dt), rng.integers(-4, 5, shape).astype(f32)
    elif op == "prod":
        n_red = n if axis is None else shape[axis]
        p = min(0.25, 6.0 / n_red)          # a handful of 2s and halves per reduced slice: no partial product leaves float32's range
        x = rng.choice(np.array([1, -1, 2], dtype=dt), size=shape, p=[0.5 - p / 2, 0.5 - p / 2, p])
        w = rng.choice(np.array([1.0, 0.5], dtype=f32), size=shape, p=[1 - p, p])
    else:
        x, w = rng.integers(-8, 9, shape).astype(dt), np.ones(shape, dtype=f32)
        big = {"max": 127, "min": -128}[op] if dt.kind == "i" else {"max": 60000.0, "min": -60000.0}[op]
        x.ravel()[0] = x.ravel()[-1] = big
    dx, dw = _dev(nd, x), _dev(nd, w)
    make = lambda: nd.multiply(dx, dw)      # noqa: E731
    got, val = _reduce_fused(nd, lib, generated, make, op, form, f"{op}, {dt.name}, {form}")
    chain = x.astype(f32) * w
    ref = getattr(np, op)(chain.astype(f64), axis=axis).astype(f32)
    _same(np.asarray(got), np.asarray(ref), f"{op}, {dt.name}, {form}")
    if val is not None:
        _same(val, chain, f"{op}, {dt.name}, {form}: the evaluated chain")


@gpu
@pytest.mark.parametrize("form", list(RED_FORMS))
def test_random_float_sums_gpu(lazy_nd, lib, on_gpu, generated, form):
    """sum(x16 * y32), random: |got - ref| <= k u sum|v| per output, ref the long-double sum of the eagerly evaluated chain, k the
    longest chain of additions of the kernel as built — derived in tests/test_fused_rows.py (row kernels) and tests/test_fused_axis.py
    (column kernels; rows per trip from the leaves' 2 + 4 bytes per element); the full reduction's order spreads over lanes, waves and
    blocks, and ANY order of n terms satisfies k = n - 1, which is what is asserted for it"""
    nd = lazy_nd
    shape, axis, _ = RED_FORMS[form]
    rng = np.random.default_rng(15)
    x, y = rng.standard_normal(shape).astype(f16), rng.standard_normal(shape).astype(f32)
    dx, dy = _dev(nd, x), _dev(nd, y)
    make = lambda: nd.multiply(dx, dy)      # noqa: E731
    got, _ = _reduce_fused(nd, lib, generated, make, "sum", form, f"sum, {form}")
    v = _eager(nd, make)
    wide = v.astype(np.longdouble)
    ref, mass = wide.sum(axis=axis), np.abs(wide).sum(axis=axis)
    if form == "full":
        k = v.size - 1
    elif form == "eval + column reduction" and not generated:
        k = shape[0] - 1        # two passes: the column sum is the eager kernel's, of which only "some order of n_red terms" is claimed here
    elif form.startswith("rows"):
        k = _rows_chain_length(shape[-1], generated)
    else:
        n_red, inner, outer = shape[-2], shape[-1], (shape[0] if len(shape) == 3 else 1)
        kind = "interpreter" if not generated else "strips" if n_red >= 512 else "tiled"
        k = _cols_chain_length(n_red, kind, _nb(outer, n_red, inner, _ru([2, 4])) if kind == "strips" else 1)
    ratio = float((np.abs(np.asarray(got).astype(np.longdouble).reshape(np.shape(ref)) - ref) / (2.0 ** -24 * mass)).max())
    print(f"sum(x16 * y32), {form}, {'generated' if generated else 'interpreter'}: ratio {ratio:.3f}, k = {k}")
    assert ratio <= k, (form, ratio, k)


@gpu
@pytest.mark.parametrize("shape, gshape", [((64, 256), (256,)), ((8, 32, 256), (8, 1, 256))], ids=["two axes", "three axes"])
def test_two_programs_share_a_float16_leaf_gpu(lazy_nd, lib, on_gpu, generated, shape, gshape):
    """x16 * g and x16 + g evaluated together: ONE vm_eval_multi call, one generated launch that reads x16 once"""
    nd = lazy_nd
    rng = np.random.default_rng(16)
    x, g = _values(f16, int(np.prod(shape)), rng).reshape(shape), rng.standard_normal(gshape).astype(f32)
    dx, dg = _dev(nd, x), _dev(nd, g)
    a, b = nd.multiply(dx, dg), nd.add(dx, dg)
    s0, l0 = nd.FUSION_STATS["vm_eval_multi"], _launched(lib)
    nd.materialize_many([a, b])
    assert nd.FUSION_STATS["vm_eval_multi"] - s0 == 1
    assert _launched(lib) - l0 == (1 if generated else 0), _launched(lib) - l0
    with np.errstate(all="ignore"):
        _same(a.get(), x * g, "x16 * g")
        _same(b.get(), x + g, "x16 + g")


def _half_store_inputs(wide):
    """Every float16 midpoint neighbourhood, the overflow threshold, the subnormal range; float64: the values that round differently
    through float32"""
    h = np.arange(0x7C00, dtype=np.uint16).view(f16).astype(f64)                 # every finite magnitude, ascending
    mid = (h[:-1] + h[1:]) / 2                                                   # exact in float32 (one more bit than float16)
    top = 65520.0                                                                # the midpoint of float16's largest and 2^16: ties to inf
    pts = np.concatenate([h, mid, [top, 65536.0, 1e5, 2.0 ** -25, 2.0 ** -26, np.inf, np.nan]])
    if wide == f32:
        p = pts.astype(f32)
        v = np.concatenate([p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))])
    else:
        m = np.concatenate([mid, [top, 2.0 ** -25]])
        # m (1 +- 2^-30) rounds to m in float32 — a tie, then to even — but lies strictly on one side of it
        v = np.concatenate([pts, np.nextafter(pts, np.inf), np.nextafter(pts, -np.inf), m * (1 + 2.0 ** -30), m * (1 - 2.0 ** -30)])
    return np.concatenate([v, -v]).astype(wide)


@gpu
@pytest.mark.parametrize("geom", ["two axes", "three axes"])
@pytest.mark.parametrize("wide", [f32, f64], ids=["f32", "f64"])
def test_chain_stored_as_float16_gpu(lazy_nd, lib, on_gpu, generated, monkeypatch, wide, geom):
    """astype(chain, float16): one vm_eval with a float16 out, no convert call, one rounding to nearest even from float32 and from
    float64 alike — NumPy's astype(float16) of the eagerly evaluated chain, bit for bit"""
    nd = lazy_nd
    v = _half_store_inputs(wide)
    if wide == f64:      # the double-rounding cases are in: through float32 at least one of them lands elsewhere
        with np.errstate(all="ignore"):
            assert (_bits(v.astype(f32).astype(f16)) != _bits(v.astype(f16)))[~np.isnan(v)].any()
    rows = -(-v.size // (32 * 256))
    v = np.resize(v, (rows, 32, 256))
    if geom == "two axes":
        v, ones = v.reshape(rows * 32, 256), np.ones(256, dtype=wide)
    else:
        ones = np.ones((rows, 1, 256), dtype=wide)
    dv, d1 = _dev(nd, v), _dev(nd, ones)
    make = lambda: nd.multiply(dv, d1)      # noqa: E731
    with np.errstate(all="ignore"):
        ref = _eager(nd, make).astype(f16)
    got = _run(nd, lib, make, 1 if generated else 0, odt=f16, what=f"float16 store, {wide.name}, {geom}")
    _same(got, ref, f"float16 store from {wide.name}, {geom}")
    # the public call: one evaluation, no conversion pass, the chain stays pending
    converts = []
    real = nd._lib().convert
    monkeypatch.setattr(nd._lib(), "convert", lambda *a: (converts.append(1), real(*a))[1])
    e = make()
    s0, l0 = nd.FUSION_STATS["vm_eval"], _launched(lib)
    r = nd.astype(e, np.float16)
    assert r.dtype == f16 and r._buf is not None and e._buf is None
    assert nd.FUSION_STATS["vm_eval"] - s0 == 1 and not converts and _launched(lib) - l0 == (1 if generated else 0)
    monkeypatch.undo()
    _same(r.get(), ref, f"astype(chain, float16) from {wide.name}, {geom}")


@gpu
def test_float16_store_one_dimensional_and_generic_gpu(lazy_nd, lib, on_gpu, generated):
    """.. over a 1-D chain with a tail, and through the generic kernel (a strided leaf)"""
    nd = lazy_nd
    rng = np.random.default_rng(17)
    v = (rng.standard_normal(2051) * 300).astype(f32)
    dv = _dev(nd, v)
    make = lambda: nd.multiply(dv, 1.5)      # noqa: E731
    _same(_run(nd, lib, make, 1 if generated else 0, odt=f16, what="1-D"), (v * np.float32(1.5)).astype(f16), "float16 store, 1-D with a tail")
    db = _dev(nd, np.repeat(v, 2))
    ds = db._view(db._offset, (2051,), (2,))
    make = lambda: nd.multiply(ds, 1.5)      # noqa: E731
    _same(_run(nd, lib, make, 0, odt=f16, what="strided"), (v * np.float32(1.5)).astype(f16), "float16 store, generic kernel")


@gpu
def test_other_forms_refuse_float16_outputs_gpu(lazy_nd, lib, on_gpu):
    """the multi-output and the eval + column-reduce forms store the compute dtype only: a float16 out is a value error"""
    nd = lazy_nd
    x = nd.asarray(np.ones((512, 1024), dtype=f32))
    a, b = nd.multiply(x, 2.0), nd.add(x, 1.0)
    progs, outs = (_capi.VmProgram * 2)(), (_capi.ArrayDesc * 2)()
    keep = []
    for k, e in enumerate((a, b)):
        progs[k], kp = nd._lz.build_program(e._expr, e.shape)
        keep.append(kp)
        o = nd.DeviceArray.empty(e.shape, np.float16)
        keep.append(o)
        outs[k] = o.desc()
    with pytest.raises(ValueError, match="float16"):
        lib.vm_eval_multi(progs, outs, 2)
    red = nd.DeviceArray.empty((1, 1024), np.float32)
    with pytest.raises(ValueError, match="float16"):
        lib.vm_eval_reduce_cols(progs[0], _capi.R_SUM, outs[0], red.desc())
