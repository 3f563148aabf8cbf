"""The 16-byte vector kernels behind mdhip_convert and behind `where` on storage-only branches (csrc/narrow.hip: k_nw_convert,
k_nw_convert_axes, k_nw_where, k_nw_where_axes), bit for bit against NumPy and against the one-element kernels they stand in front
of (options convert_vec / where_vec = 0: k_convert, k_nw_where_generic). Counters convert_vec_runs / where_vec_runs: +1 for every
launch of a vector kernel the host issues.

Where the numbers come from (the launchers of narrow.hip):
  floor            both conversion forms and both `where` forms run from 2**14 elements on; below, the call keeps the generic kernel.
  E (conversion)   16 / (size of the narrower side) elements per lane and trip, at most 8 where one side is 8 bytes wide: int8 ->
                   float32 16, float16 <-> float32 8, float64 -> int8 8, uint32 -> uint64 4, uint64 -> float64 2. The source is on
                   min(16, E * its element size) bytes, the output likewise.
  E (where)        16 / sizeof(S); cond on E bytes, branches and output on 16.
  grid             md_grid_for(groups + 1, 256, cap): cap = option max_blocks, else 8 blocks per CU (VEC/VEC `where`: 4). The geometry
                   tests set max_blocks = 32: a grid trip is 8192 groups (16384 uint64 elements: the floor), so "one group past a trip" and "two trips + 5 groups + 3
                   elements" (the two-in-flight loop, the one-group loop and the tail all run) are a MiB at most. One conversion
                   runs at the default cap as well (2048 * 256 + 1 groups).
  axes             two to four collapsed axes, inner stride 1 on both sides (where: 0 or 1 for cond and the branches), inner % E == 0,
                   outer strides and base addresses on the vector alignment; (34, 480) = 16320 elements is the refusal below the floor.

Data: every operand is a view inside a sentinel-padded base, the output a view inside a sentinel base of this module's own, and the
WHOLE output base is compared on raw bits. Conversions: tests/test_elementwise_paths.py's _cast_values (in range of the destination,
rounding cases planted at vector, tail and trip boundaries), then exhaustive float16 sources, every float16 rounding boundary from
float32 and float64, and out-of-range / NaN floats into the integers (against option 0 only: NumPy leaves them undefined). `where`:
branches of arbitrary bit patterns (float16: all 65536, signalling NaNs included) — a selection moves bits.

Each test has a CPU twin on the test double (values against NumPy, the options exist, the counters stay 0) and a gpu twin."""
import ctypes as C

import numpy as np
import pytest

from minidiff_amd import _capi
from minidiff_amd import ndarray as nd
from test_elementwise_paths import ALL12, N7, PAD, _bits, _cast_values, _counter, _same_bits, _sentinel, _twins
from test_elementwise_paths import b8, f16, f32, f64, i8, i16, i32, i64, u8, u16, u32, u64

FLOOR = 1 << 14
MD_BLOCK, MD_NUM_CUS = 256, 256
CAP = 32                                   # option max_blocks of the geometry tests: a trip of 2-element groups is the floor
TRIP = CAP * MD_BLOCK                      # groups per grid trip under it
DEFAULT_TRIP = MD_NUM_CUS * 8 * MD_BLOCK   # .. at the default cap (VEC/VEC `where`: 4 per CU)
INTS = (i8, i16, i32, i64, u8, u16, u32, u64)


def E_cv(s, d):
    lo, hi = min(s.itemsize, d.itemsize), max(s.itemsize, d.itemsize)
    e = 16 // lo
    return 8 if hi == 8 and e > 8 else e


@pytest.fixture(autouse=True)
def eager():
    prev = nd.set_lazy(False)
    yield
    nd.set_lazy(prev)


def _opt(name):
    v = C.c_int64()
    nd._lib().debug_get_option(name.encode(), C.byref(v))
    return v.value


def _counted(name, fn):
    n0 = _opt(name)
    r = fn()
    return r, _opt(name) - n0


def _id(a):
    return a


class Arr:
    """`vals` dense inside a 1-D sentinel base from element `off`, then `cut` (works on NumPy and on device arrays alike)."""

    def __init__(self, vals, cut=None, off=PAD):
        vals = np.ascontiguousarray(vals)
        self.shape, self.n, self.cut, self.off, self.dt = vals.shape, vals.size, cut or _id, off, vals.dtype
        self.base = np.full(self.n + 2 * PAD + 2, _sentinel(vals.dtype), dtype=vals.dtype)
        self.base[off:off + self.n] = vals.ravel()

    def of(self, base):
        return self.cut(base[self.off:self.off + self.n].reshape(self.shape))

    @property
    def view(self):
        return self.of(self.base)


def _out(dt, shape, cut=None):
    return Arr(np.full(shape, _sentinel(dt), dtype=dt), cut)


def _convert(x, odt, out=None):
    """lib.convert of x (an Arr) into a sentinel base -> (the whole base afterwards, what NumPy expects of it)"""
    out = out or _out(odt, x.view.shape)
    with np.errstate(all="ignore"):
        ref = x.view.astype(odt)
    expect = out.base.copy()
    out.of(expect)[...] = ref
    dx, dob = nd.asarray(x.base), nd.asarray(out.base)
    nd._lib().convert(x.of(dx).desc(), out.of(dob).desc())
    return dob.get(), expect


def _check_convert(x, odt, on_gpu, mdopt, taken, what, out=None, defined=None):
    """One conversion: against NumPy (where `defined`, a mask over the output base, or everywhere), its routing, and the
    one-element route (gpu)."""
    (got, expect), runs = _counted("convert_vec_runs", lambda: _convert(x, odt, out))
    g, r = _bits(got), _bits(expect)
    if defined is None:
        _same_bits(got, expect, what)
    else:
        assert np.array_equal(g[defined], r[defined]), (what, int((g[defined] != r[defined]).sum()))
    if not on_gpu:
        assert runs == 0, what
        return got
    assert runs == (1 if taken else 0), (what, runs)
    mdopt("convert_vec", 0)
    (old, _), runs = _counted("convert_vec_runs", lambda: _convert(x, odt, out))
    mdopt("convert_vec", 1)
    assert runs == 0, what
    _same_bits(got, old, what + ("against convert_vec = 0",))
    return got


# ---- 1. options and counters --------------------------------------------------------------------------------------------------------
def _options(case, mdopt, on_gpu):
    assert _opt("convert_vec") == 1 and _opt("where_vec") == 1
    for name in ("convert_vec_runs", "where_vec_runs"):
        before = _opt(name)
        mdopt(name, before + 5)
        assert _opt(name) == before + 5
        mdopt(name, before)
    mdopt("convert_vec", 0)
    mdopt("where_vec", 0)
    assert _opt("convert_vec") == 0 and _opt("where_vec") == 0


test_options, test_options_gpu = _twins(["table"])(_options)


# ---- 2. routing ---------------------------------------------------------------------------------------------------------------------
def _f16_vals(shape, seed):
    x = np.random.default_rng(seed).standard_normal(shape).astype(f16)
    x.reshape(-1)[:6] = np.array([np.nan, np.inf, -0.0, 6e-8, -np.inf, 65504], dtype=f16)
    return x


def _f16_small(shape, seed):
    """quarters in (-100, 100): in range of int8, truncation visible"""
    return (np.random.default_rng(seed).integers(-400, 401, shape) / 4.0).astype(f16)


#        id                       source -> Arr                                                    dst   out cut                      taken
CONVERT_ROUTES = {
    "stream-floor":              (lambda: Arr(_f16_vals(FLOOR, 1)),                                f32,  None,                        True),
    "stream-below-floor":        (lambda: Arr(_f16_vals(FLOOR - 1, 2)),                            f32,  None,                        False),
    "stream-source-off-by-one":  (lambda: Arr(_f16_vals(FLOOR, 3), off=PAD + 1),                   f32,  None,                        False),
    "stream-option-0":           (lambda: Arr(_f16_vals(FLOOR, 4)),                                f32,  None,                        None),
    "axes-2d":                   (lambda: Arr(_f16_vals((37, 496), 5), lambda a: a[:, :480]),      f32,  None,                        True),
    "axes-2d-copy":              (lambda: Arr(_f16_vals((37, 496), 6), lambda a: a[:, :480]),      f16,  None,                        True),
    "axes-2d-into-slice":        (lambda: Arr(_f16_vals((37, 480), 7)),                            f32,  ((37, 496), lambda a: a[:, :480]), True),
    "axes-3d":                   (lambda: Arr(_f16_vals((5, 37, 104), 8), lambda a: a[:, :, :96]), f32,  None,                        True),
    "axes-4d":                   (lambda: Arr(_f16_small((3, 5, 37, 40), 9), lambda a: a[..., :32]), i8, None,                        True),
    "axes-row-stride-481":       (lambda: Arr(_f16_vals((37, 481), 10), lambda a: a[:, :480]),     f32,  None,                        False),
    "axes-inner-not-multiple":   (lambda: Arr(_f16_vals((37, 496), 11), lambda a: a[:, :476]),     f32,  None,                        False),
    "axes-below-floor":          (lambda: Arr(_f16_vals((34, 496), 12), lambda a: a[:, :480]),     f32,  None,                        False),
    "strided-inner":             (lambda: Arr(_f16_vals((37, 960), 13), lambda a: a[:, ::2]),      f32,  None,                        False),
}


def _convert_route(case, mdopt, on_gpu):
    mk, odt, ocut, taken = CONVERT_ROUTES[case]
    x = mk()
    out = _out(odt, ocut[0], ocut[1]) if ocut else None
    if taken is None:
        mdopt("convert_vec", 0)
    _check_convert(x, odt, on_gpu, mdopt, bool(taken), (case,), out)


test_convert_routing, test_convert_routing_gpu = _twins(list(CONVERT_ROUTES))(_convert_route)


# ---- 3. geometry of the conversion stream -------------------------------------------------------------------------------------------
GEOM_PAIRS = {"int8-float32": (i8, f32), "float16-float32": (f16, f32), "float32-float16": (f32, f16), "float64-int8": (f64, i8), "uint32-uint64": (u32, u64)}


def _geom_sizes(E):
    return [FLOOR, FLOOR + E - 1, (TRIP + 1) * E, (2 * TRIP + 5) * E + 3]


def _convert_geometry(case, mdopt, on_gpu):
    s, d = GEOM_PAIRS[case]
    E = E_cv(s, d)
    if on_gpu:
        mdopt("max_blocks", CAP)
    for n in _geom_sizes(E):
        assert n >= FLOOR
        rng = np.random.default_rng([s.num, d.num, n])
        vals = _cast_values(s, d, n, rng, E, TRIP)
        with np.errstate(all="ignore"):
            ref = vals.astype(d)
            assert not np.array_equal(_bits(np.roll(vals, 1).astype(d)), _bits(ref)), (case, n, "rolled by one, same reference")
        for nt in ((0, 1) if on_gpu and n <= FLOOR + E else (None,)):
            if nt is not None:
                mdopt("nt", nt)
            _check_convert(Arr(vals), d, on_gpu, mdopt, True, (case, n, nt))
        if on_gpu:
            mdopt("nt", -1)


test_convert_geometry, test_convert_geometry_gpu = _twins(list(GEOM_PAIRS))(_convert_geometry)


@pytest.mark.gpu
def test_convert_default_grid_gpu(lib, on_gpu, mdopt):
    """One group past a trip of the default grid (8 blocks per CU): lane 0 alone runs the two-in-flight loop."""
    assert on_gpu
    n = (DEFAULT_TRIP + 1) * 8 + 5
    vals = _cast_values(f32, f16, n, np.random.default_rng(77), 8, DEFAULT_TRIP)
    _check_convert(Arr(vals), f16, True, mdopt, True, ("default grid", n))


# ---- 4. all 144 pairs ---------------------------------------------------------------------------------------------------------------
def _all_pairs(case, mdopt, on_gpu):
    s = np.dtype(case)
    n = FLOOR + 3
    for d in ALL12:
        E = E_cv(s, d)
        vals = _cast_values(s, d, n, np.random.default_rng([s.num, d.num]), E, TRIP)
        if s == u64 and d.kind == "f":              # the upper unsigned half into every float type
            vals[40:44] = np.array([1 << 63, (1 << 63) + (1 << 40), (1 << 64) - 1, (1 << 63) + 1], dtype=u64)
        _check_convert(Arr(vals), d, on_gpu, mdopt, True, (s.name, d.name))


test_all_pairs, test_all_pairs_gpu = _twins([d.name for d in ALL12])(_all_pairs)


# ---- 5. exhaustive and boundary conversions -----------------------------------------------------------------------------------------
def _base_mask(out_like, mask_view):
    """A mask over an output base: True on the padding, mask_view on the view."""
    m = np.ones(out_like.base.shape, dtype=bool)
    out_like.of(m)[...] = mask_view
    return m


def _every_half(case, mdopt, on_gpu):
    d = np.dtype(case)
    vals = np.arange(65536, dtype=u16).view(f16)
    assert vals.size >= FLOOR
    v64 = vals.astype(f64)
    if d.kind == "f":
        defined = ~np.isnan(v64)
    elif d == b8:
        defined = np.ones(65536, dtype=bool)
    else:
        info = np.iinfo(d)
        with np.errstate(invalid="ignore"):
            defined = np.isfinite(v64) & (np.trunc(v64) >= info.min) & (np.trunc(v64) <= info.max)
    out = _out(d, vals.shape)
    got = _check_convert(Arr(vals), d, on_gpu, mdopt, True, ("every float16", d.name), defined=_base_mask(out, defined))
    if d.kind == "f":                               # NaN as NaN
        assert np.isnan(out.of(got)[np.isnan(v64)]).all()


test_every_half, test_every_half_gpu = _twins([d.name for d in ALL12])(_every_half)


def _half_midpoints():
    """float64: the midpoint between every finite non-negative float16 and its successor (65504 -> 65536)."""
    h = np.arange(0x7C00, dtype=u16).view(f16).astype(f64)
    nxt = np.append(h[1:], 65536.0)
    return (h + nxt) / 2


def _rounding_values(src):
    mid = _half_midpoints().astype(src)
    assert np.array_equal(mid.astype(f64), _half_midpoints())
    extra = np.array([65504, 65520, 2.0 ** -24, 2.0 ** -25], dtype=src)
    pts = np.concatenate([mid, extra])
    parts = [pts, np.nextafter(pts, src.type(np.inf)), np.nextafter(pts, src.type(-np.inf))]
    if src == f64:                                  # what a detour through float32 rounds the wrong way
        parts += [mid * (1 + 2.0 ** -30), mid * (1 - 2.0 ** -30)]
    x = np.concatenate(parts)
    return np.concatenate([x, -x])


def _to_half_boundaries(case, mdopt, on_gpu):
    src = np.dtype(case)
    vals = _rounding_values(src)
    assert vals.size >= FLOOR
    if src == f64:                                  # the detour's answer differs from the single rounding on some of them
        with np.errstate(over="ignore"):
            assert (vals.astype(f32).astype(f16).view(u16) != vals.astype(f16).view(u16)).any()
    _check_convert(Arr(vals), f16, on_gpu, mdopt, True, (case, "-> float16 boundaries"))


test_to_half_boundaries, test_to_half_boundaries_gpu = _twins(["float32", "float64"])(_to_half_boundaries)


def _float_to_int_out_of_range(case, mdopt, on_gpu):
    """Compared against the one-element route only (NumPy leaves these undefined): the values wrap from 64 bits."""
    src = np.dtype(case)
    sp = np.array([2.0 ** 31, -2.0 ** 31, 2.0 ** 63, -2.0 ** 63, 1e30, -1e30, np.nan, -np.nan, np.inf, -np.inf, 2.0 ** 32 + 5, -2.0 ** 32 - 5, 2.0 ** 64,
                   2.0 ** 63 + 2.0 ** 41, -2.0 ** 31 - 4096, 3e9, -3e9, 200.5, -200.5, 70000.0, 1.9e19, -1.9e19], dtype=f64).astype(src)
    vals = np.tile(sp, FLOOR // sp.size + 1)[:FLOOR + 5]
    for d in INTS:
        out = _out(d, vals.shape)
        _check_convert(Arr(vals), d, on_gpu, mdopt, True, (case, d.name, "out of range"), defined=_base_mask(out, np.zeros(vals.size, dtype=bool)))


test_float_to_int_out_of_range, test_float_to_int_out_of_range_gpu = _twins(["float32", "float64"])(_float_to_int_out_of_range)


# ---- 6. where -----------------------------------------------------------------------------------------------------------------------
def _patterns(dt, shape, salt):
    """Arbitrary bit patterns of dt (float16: a permutation of all 65536, repeated)."""
    n = int(np.prod(shape))
    if dt == f16:
        perm = np.random.default_rng(salt).permutation(65536).astype(u16)
        return np.tile(perm, n // 65536 + 1)[:n].view(f16).reshape(shape)
    return _counter(np.dtype(f"u{dt.itemsize}"), n, salt).view(dt).reshape(shape)


def _mask(shape, salt):
    return _counter(b8, int(np.prod(shape)), salt).reshape(shape)


def _where(c, a, b):
    """lib.where of Arr / Python-scalar operands into a sentinel base -> (the whole base afterwards, what NumPy expects of it)"""
    views = [v.view if isinstance(v, Arr) else v for v in (c, a, b)]
    ref = np.where(*views)
    out = _out(ref.dtype, ref.shape)
    expect = out.base.copy()
    out.of(expect)[...] = ref
    dob = nd.asarray(out.base)
    descs, keep = [], []                            # (keep: the device operands live until the call returns)
    for v in (c, a, b):
        if isinstance(v, Arr):
            keep.append(v.of(nd.asarray(v.base)))
            descs.append(keep[-1].desc(ref.shape))
        else:
            descs.append(nd._scalar_desc(v, _capi.F64 if isinstance(v, float) else _capi.I64))
    nd._lib().where(descs[0], descs[1], descs[2], out.of(dob).desc())
    return dob.get(), expect


def _signalling(base):
    if base.dtype != f16:
        return np.zeros(base.shape, dtype=bool)
    b = base.view(u16)
    return ((b & 0x7C00) == 0x7C00) & ((b & 0x03FF) != 0) & ((b & 0x0200) == 0)


def _check_where(c, a, b, on_gpu, mdopt, taken, what):
    (got, expect), runs = _counted("where_vec_runs", lambda: _where(c, a, b))
    if not on_gpu:
        # (the double selects through the carrier, md_half_to_double: a float16 NaN comes out as the canonical one — NaN as NaN there)
        assert runs == 0, what
        nan = np.isnan(expect) if expect.dtype == f16 else np.zeros(expect.shape, dtype=bool)
        assert np.array_equal(_bits(got)[~nan], _bits(expect)[~nan]) and np.isnan(got[nan]).all(), what
        return
    ok = ~_signalling(expect)                       # (the generic kernel passes float16 through float32: a signalling NaN comes out quiet)
    if taken:
        _same_bits(got, expect, what)
    else:
        assert np.array_equal(_bits(got)[ok], _bits(expect)[ok]), what
    assert runs == (1 if taken else 0), (what, runs)
    mdopt("where_vec", 0)
    (old, _), runs = _counted("where_vec_runs", lambda: _where(c, a, b))
    mdopt("where_vec", 1)
    assert runs == 0, what
    assert np.array_equal(_bits(got)[ok], _bits(old)[ok]), what + ("against where_vec = 0",)


def _scalars(dt):
    if dt == f16:
        return 0.1, -2.3
    return (3, 7) if dt.kind == "u" else (-3, 7)


def _where_operands(dt, mode, shape, salt):
    sa, sb = _scalars(dt)
    a = Arr(_patterns(dt, shape, salt + 1)) if mode[0] == "V" else sa
    b = Arr(_patterns(dt, shape, salt + 2)) if mode[1] == "V" else sb
    return Arr(_mask(shape, salt)), a, b


WHERE_ROUTES = ["VV", "VS", "SV", "below-floor", "int8-condition", "two-dtypes", "condition-off-by-one", "option-0", "axes-row-branch", "axes-3d-branch",
                "axes-sliced-branch", "axes-broadcast-condition", "axes-below-floor"]


def _where_route(case, mdopt, on_gpu):
    dt = f16
    if case in ("VV", "VS", "SV"):
        _check_where(*_where_operands(dt, case, (FLOOR,), 1), on_gpu, mdopt, True, (case,))
    elif case == "below-floor":
        _check_where(*_where_operands(dt, "VS", (FLOOR - 1,), 2), on_gpu, mdopt, False, (case,))
    elif case == "int8-condition":
        c, a, b = _where_operands(dt, "VS", (FLOOR,), 3)
        _check_where(Arr(c.view.astype(i8) * 5), a, b, on_gpu, mdopt, False, (case,))
    elif case == "two-dtypes":
        c, a, _ = _where_operands(dt, "VS", (FLOOR,), 4)
        a = Arr(np.random.default_rng(4).standard_normal(FLOOR).astype(f16))
        _check_where(c, a, Arr(np.random.default_rng(5).standard_normal(FLOOR).astype(f32)), on_gpu, mdopt, False, (case,))
    elif case == "condition-off-by-one":
        c, a, b = _where_operands(dt, "VV", (FLOOR,), 5)
        _check_where(Arr(c.view, off=PAD + 1), a, b, on_gpu, mdopt, False, (case,))
    elif case == "option-0":
        mdopt("where_vec", 0)
        _check_where(*_where_operands(dt, "VV", (FLOOR,), 6), on_gpu, mdopt, False, (case,))
    elif case == "axes-below-floor":
        _check_where(Arr(_mask((34, 480), 7)), Arr(_patterns(dt, (34, 480), 8)), Arr(_patterns(dt, (480,), 9)), on_gpu, mdopt, False, (case,))
    else:
        for dt in (i8, f16, u64):
            if case == "axes-row-branch":
                ops = Arr(_mask((35, 480), 10)), Arr(_patterns(dt, (35, 480), 11)), Arr(_patterns(dt, (480,), 12))
            elif case == "axes-3d-branch":
                ops = Arr(_mask((5, 37, 96), 13)), Arr(_patterns(dt, (5, 1, 96), 14)), _scalars(dt)[1]
            elif case == "axes-sliced-branch":
                ops = Arr(_mask((35, 480), 15)), Arr(_patterns(dt, (35, 496), 16), lambda a: a[:, :480]), Arr(_patterns(dt, (35, 480), 17))
            else:
                ops = Arr(_mask((5, 37, 1), 18)), Arr(_patterns(dt, (5, 37, 96), 19)), Arr(_patterns(dt, (3, 5, 37, 96), 20))
            _check_where(*ops, on_gpu, mdopt, True, (case, dt.name))


test_where_routing, test_where_routing_gpu = _twins(WHERE_ROUTES)(_where_route)


def _where_stream(case, mdopt, on_gpu):
    dt = np.dtype(case)
    E = 16 // dt.itemsize
    if on_gpu:
        mdopt("max_blocks", CAP)
    for mode in ("VV", "VS", "SV"):
        for n in (FLOOR, FLOOR + E - 1, (TRIP + 1) * E, (2 * TRIP + 5) * E + 3):
            assert n >= FLOOR
            c, a, b = _where_operands(dt, mode, (n,), n % 97)
            for nt in ((0, 1) if on_gpu and n <= FLOOR + E else (None,)):
                if nt is not None:
                    mdopt("nt", nt)
                _check_where(c, a, b, on_gpu, mdopt, True, (case, mode, n, nt))
            if on_gpu:
                mdopt("nt", -1)
    if dt == f16:                                   # every pattern, signalling NaNs included, on both branches
        n = 65536 + 8 * 3 + 5
        c, a, b = _where_operands(dt, "VV", (n,), 31)
        assert _signalling(a.view).any() and np.unique(a.view.view(u16)).size == 65536
        _check_where(c, a, b, on_gpu, mdopt, True, (case, "all patterns"))


test_where_stream, test_where_stream_gpu = _twins([d.name for d in N7])(_where_stream)


@pytest.mark.gpu
def test_where_default_grid_gpu(lib, on_gpu, mdopt):
    """One vector past a trip of the default grids: 4 blocks per CU for VEC/VEC, 8 with a scalar branch."""
    assert on_gpu
    for mode, per_cu in (("VV", 4), ("VS", 8)):
        n = (MD_NUM_CUS * per_cu * MD_BLOCK + 1) * 8 + 3
        _check_where(*_where_operands(f16, mode, (n,), 41), True, mdopt, True, ("default grid", mode))


# ---- 2b. the same routing through nd.* ----------------------------------------------------------------------------------------------
def _public(case, mdopt, on_gpu):
    want = 1 if on_gpu else 0
    x32 = np.random.default_rng(50).standard_normal(FLOOR).astype(f32)
    x16 = _f16_vals((37, 496), 51)
    d32, d16 = nd.asarray(x32), nd.asarray(x16)
    got, runs = _counted("convert_vec_runs", lambda: nd.astype(d32, np.float16).get())
    assert runs == want
    _same_bits(got, x32.astype(f16), ("nd.astype",))
    got, runs = _counted("convert_vec_runs", lambda: d32.astype(np.float16).get())
    assert runs == want
    got, runs = _counted("convert_vec_runs", lambda: nd.copy(d16[:, :480]).get())
    assert runs == want
    _same_bits(got, x16[:, :480].copy(), ("nd.copy of a slice",))
    got, runs = _counted("convert_vec_runs", lambda: d16[:, :480].astype(np.float32).get())
    assert runs == want
    _same_bits(got, x16[:, :480].astype(f32), ("astype of a slice",))
    got, runs = _counted("convert_vec_runs", lambda: d16.copy().get())
    assert runs == want
    _same_bits(got, x16, ("DeviceArray.copy",))
    got, runs = _counted("convert_vec_runs", lambda: nd.astype(nd.asarray(x32[:FLOOR - 1]), np.float16).get())
    assert runs == 0
    _same_bits(got, x32[:FLOOR - 1].astype(f16), ("nd.astype below the floor",))
    # where: relu-like selections of a float16 array, a row branch under a 2-D condition
    m = _mask((37, 496), 52)
    dm = nd.asarray(m)
    for a, b in ((x16, 0), (0, x16), (x16, -x16), (x16, 0.1)):
        da, db = (nd.asarray(v) if isinstance(v, np.ndarray) else v for v in (a, b))
        got, runs = _counted("where_vec_runs", lambda: nd.where(dm, da, db).get())
        assert runs == want
        _same_bits(got, np.where(m, a, b), ("nd.where", type(a).__name__, type(b).__name__))
    row = _f16_vals((496,), 53)
    got, runs = _counted("where_vec_runs", lambda: nd.where(dm, d16, nd.asarray(row)).get())
    assert runs == want
    _same_bits(got, np.where(m, x16, row), ("nd.where, row branch",))
    got, runs = _counted("where_vec_runs", lambda: nd.where(dm, d16, nd.asarray(x16.astype(f32))).get())
    assert runs == 0
    _same_bits(got, np.where(m, x16, x16.astype(f32)), ("nd.where, two dtypes",))


test_public, test_public_gpu = _twins(["nd"])(_public)


# ---- 7. determinism -----------------------------------------------------------------------------------------------------------------
def _determinism(case, mdopt, on_gpu):
    if on_gpu:
        mdopt("max_blocks", CAP)
    n = (2 * TRIP + 5) * 8 + 3
    x = Arr(_cast_values(f32, f16, n, np.random.default_rng(60), 8, TRIP))
    c, a, b = _where_operands(f16, "VV", (n,), 61)
    runs = []
    for _ in range(2):
        runs.append((_convert(x, f16)[0], _where(c, a, b)[0]))
    assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


test_determinism, test_determinism_gpu = _twins(["interleaved"])(_determinism)
