"""Thin and long-k float16 / int8 / uint8 products on the streaming kernels of csrc/skinny.hip, read in the operands' own type (planned by
gemm.hip plan_narrow: the long-k and the thin hand-off in front of the MFMA / generic / widened choice; option gemm_narrow_skinny = 0
restores the routes the products had; counter gemm_narrow_thin_runs: +1 per native launch the host issues, +2 for a long-k product).

Numerical contract (the project's own, tests/test_narrow_matmul.py and tests/test_matmul_dtype.py): int8 -> int8 and uint8 -> uint8 the
low byte of the exact sum, int8 -> int32 NumPy's wrapped sum, bit for bit; float16 -> float16 within
ulp16(exact) / 2 + K * 2**-23 * (|a| @ |b|) of the float64 product, float16 -> float32 within K * 2**-23 * (|a| @ |b|) + ulp32(exact) / 2
(every product of two float16 values is exact in float32: only the order of the float32 additions is free); integer-valued float16
operands with |a| @ |b| < 2**24 make every partial sum exact, so the result is `exact` itself (float32) or its one rounding (float16),
whatever the kernel's order; inf / NaN where np.matmul has them; the same bits run to run.

Shapes come from the launchers' constants (skinny.hip): a lane load is 16 B = V elements (8 float16, 16 bytes); row dot: KC = 4096 B of
k per LDS chunk, RW = 1 / 2 / 4 rows per wave from R = 512 / 4096 / 8192 (float16 at 8 columns: 2 from 4096 on), NCT = 1 / 2 / 4 / 8
column instantiations; column sum: a strip is 64 * V of r, NB = min(ceil(1024 / (strips * batch)), 64, K / 32) bands of k rows, eight
rows per wave and batch; long-k: patches 1x1 / 2x2 / 4x4 / 8x1 / 1x8 / 8x8, K >= 512, blocks of >= 4096 k. Floors of the hand-off:
thin side <= 8, R >= 512, K >= 64, R * K * batch >= 2**20, X 16-B aligned, its unit-stride extent a multiple of V."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu
# (operand dtype, wide output dtype or None)
KINDS = {"f16": (np.float16, None), "f16->f32": (np.float16, np.float32), "i8": (np.int8, None), "i8->i32": (np.int8, np.int32), "u8": (np.uint8, None)}
V = {np.float16: 8, np.int8: 16, np.uint8: 16}          # elements per 16-B lane load
KC = {np.float16: 2048, np.int8: 4096, np.uint8: 4096}  # row dot: elements of k per LDS chunk


def _nd():
    from minidiff_amd import ndarray as nd
    return nd


@pytest.fixture
def eager():
    nd = _nd()
    prev = nd.set_lazy(False)
    yield nd
    nd.set_lazy(prev)


def _opt(lib, name):
    v = C.c_int64()
    lib.debug_get_option(name.encode(), C.byref(v))
    return v.value


def _runs(lib):
    return _opt(lib, "gemm_narrow_thin_runs")


def _data(rng, shape, dt, small_ints=False):
    if dt == np.float16:
        if small_ints:
            return rng.integers(-8, 9, shape).astype(np.float16)
        return rng.standard_normal(shape).astype(np.float16)
    lo, hi = (-128, 128) if dt == np.int8 else (0, 256)
    x = rng.integers(lo, hi, shape).astype(dt)
    flat = x.reshape(-1)
    ext = np.array([lo, hi - 1, 0, hi - 1, lo], dtype=np.int64).astype(dt)
    flat[: min(5, flat.size)] = ext[: min(5, flat.size)]
    return x


def _mm(nd, a, b, wide, **kw):
    return nd.matmul(a, b, dtype=wide, **kw) if wide is not None else nd.matmul(a, b, **kw)


def _check(got, a, b, dt, wide, what=""):
    """got against the contract for operands a, b (NumPy arrays, any batch)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = np.matmul(a64, b64)
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    if dt != np.float16:
        out = wide or dt
        assert got.dtype == out, (what, got.dtype)
        # (|sum| < 2**53: exact in float64; then NumPy's wrap to int32 / low byte)
        exp = np.rint(exact).astype(np.int64).astype(out)
        assert np.array_equal(got, exp), (what, int((got != exp).sum()))
        return
    K = a.shape[-1]
    mag = np.matmul(np.abs(a64), np.abs(b64))
    if wide is None:
        assert got.dtype == np.float16, (what, got.dtype)
        with np.errstate(over="ignore"):
            ulp = np.spacing(np.abs(exact).astype(np.float16)).astype(np.float64)
        fin = np.isfinite(ulp)
        assert np.array_equal(np.isinf(got), ~fin), what          # past 65504: inf, as NumPy's cast
        bound = ulp / 2 + K * 2.0 ** -23 * mag
    else:
        assert got.dtype == np.float32, (what, got.dtype)
        fin = np.ones(exact.shape, bool)
        bound = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64) / 2 + K * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - exact)
    bad = fin & ~(err <= bound)
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(bound, 1e-300))[fin].max()))


def _check_exact_ints(got, a, b, wide, what=""):
    """integer-valued float16 operands, |a| @ |b| < 2**24: bit for bit, whatever the order of the sum"""
    exact = np.matmul(a.astype(np.float64), b.astype(np.float64))
    assert np.matmul(np.abs(a.astype(np.float64)), np.abs(b.astype(np.float64))).max() < 2 ** 24
    with np.errstate(over="ignore"):
        exp = exact.astype(np.float32 if wide is not None else np.float16)
    assert got.dtype == exp.dtype and np.array_equal(got, exp), (what, int((got != exp).sum()))


# ---- 1. the options (CPU double and GPU) -------------------------------------------------------------------------------------------
def test_options_are_in_the_shared_table(lib, mdopt):
    assert _opt(lib, "gemm_narrow_skinny") == 1
    mdopt("gemm_narrow_skinny", 0)
    assert _opt(lib, "gemm_narrow_skinny") == 0
    before = _runs(lib)
    mdopt("gemm_narrow_thin_runs", before + 5)
    assert _runs(lib) == before + 5


@gpu
def test_options_are_in_the_shared_table_on_the_gpu(lib, mdopt):
    test_options_are_in_the_shared_table(lib, mdopt)


# ---- 2. routing: the counter -------------------------------------------------------------------------------------------------------
# what each entry reaches, per kind K (f16 / f16->f32 / i8 / i8->i32 / u8 = MdThin<S, O>; u8 runs MdThin<int8, int8>):
#   "M @ v"   (512, K) @ (K,), K = 2**20 / 512        k_skinny_rowdot<K, 1, 1>, Y staged in 16-B pieces          1 launch
#   "v @ M"   (K,) @ (K, 1024), K = 1024               k_skinny_colsum<K, 1, 8>, NB = min(1024 / strips, K / 32)  1 launch
#   "dot"     (4096,) . (4096,)                        k_longk_partial<K, 1, 1> + k_longk_finish<K, 1, 1>         2 launches
def _route_products(nd, rng, dt, wide):
    out = []
    a, v = _data(rng, (512, 2048), dt), _data(rng, (2048,), dt)
    out.append(("M @ v", 1, a, v, lambda A=nd.asarray(a), B=nd.asarray(v): _mm(nd, A, B, wide)))
    v, m = _data(rng, (1024,), dt), _data(rng, (1024, 1024), dt)
    out.append(("v @ M", 1, v, m, lambda A=nd.asarray(v), B=nd.asarray(m): _mm(nd, A, B, wide)))
    v, w = _data(rng, (4096,), dt), _data(rng, (4096,), dt)
    if wide is None:
        out.append(("dot", 2, v, w, lambda A=nd.asarray(v), B=nd.asarray(w): nd.dot(A, B)))
    else:
        out.append(("dot", 2, v, w, lambda A=nd.asarray(v), B=nd.asarray(w): _mm(nd, A, B, wide)))
    return out


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_native_launches_are_counted(lib, mdopt, eager, kind):
    nd = eager
    dt, wide = KINDS[kind]
    for what, launches, a, b, run in _route_products(nd, np.random.default_rng(1), dt, wide):
        n0 = _runs(lib)
        got = np.asarray(run().get())
        assert _runs(lib) - n0 == launches, (kind, what, _runs(lib) - n0)
        _check(got.reshape(np.matmul(a.astype(np.float64), b.astype(np.float64)).shape), a, b, dt, wide, (kind, what))
        mdopt("gemm_narrow_skinny", 0)
        n0 = _runs(lib)
        old = np.asarray(run().get())
        assert _runs(lib) == n0, (kind, what)
        mdopt("gemm_narrow_skinny", 1)
        _check(old.reshape(got.shape), a, b, dt, wide, (kind, what, "option 0"))
        if dt != np.float16:
            assert np.array_equal(old, got), (kind, what)


# ---- 3. what the hand-offs decline keeps its route and its bits -----------------------------------------------------------------------
def _declined(dt):
    v = V[dt]
    # (M, K, N, offset of A in elements) — R = 504 < 512 (K a multiple of V with R * K >= 2**20); K no multiple of V; A one element off
    # 16-B alignment; a thin side of 9
    return [("R = 504", 504, 2096, 1, 0), ("K % V != 0", 512, 2048 + v // 2, 1, 0), ("A off by one element", 512, 2048, 1, 1), ("9 columns", 512, 2048, 9, 0)]


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_declined_products_keep_their_route(lib, mdopt, eager, kind):
    nd = eager
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(2)
    for what, M, K, N, off in _declined(dt):
        base = _data(rng, (M * K + off,), dt)
        a = base[off:].reshape(M, K)
        b = _data(rng, (K, N), dt)
        da, db = nd.asarray(base)[off:].reshape((M, K)), nd.asarray(b)
        n0 = _runs(lib)
        new = _mm(nd, da, db, wide).get()
        assert _runs(lib) == n0, (kind, what)
        mdopt("gemm_narrow_skinny", 0)
        old = _mm(nd, da, db, wide).get()
        mdopt("gemm_narrow_skinny", 1)
        assert np.array_equal(new.view(np.uint8), old.view(np.uint8)), (kind, what)
        _check(new, a, b, dt, wide, (kind, what))


# ---- 4. row dot (X unit-stride along k) ----------------------------------------------------------------------------------------------
# (R, K, nc) -> k_skinny_rowdot<kind, NCT, RW>: every RW at the smallest K with R * K >= 2**20, every NCT with fewer live columns than its
# width (3 of 4, 5 of 8), K inside one LDS chunk / over three chunks and no multiple of a chunk (2 KC + 3 V). Y as (K, nc) C order
# (staged element by element across the columns) and as the transpose of (nc, K) (staged in 16-B pieces along k).
def _rowdot_cases(dt):
    kc, v = KC[dt], V[dt]
    return [("RW 1, NCT 1, K in one chunk", 1024, kc // 2, 1), ("RW 2, NCT 2", 4096, 256, 2), ("RW 4, NCT 4 (3 live)", 8192, 128, 3),
            ("RW 1, NCT 8 (5 live), 3 ragged chunks", 512, 2 * kc + 3 * v, 5), ("RW 1, NCT 8, 3 ragged chunks", 512, 2 * kc + 3 * v, 8),
            ("RW 4 (float16: 2), NCT 8", 8192, 128, 8), ("RW 2, NCT 1", 4096, 256, 1)]


@gpu
@pytest.mark.parametrize("y_t", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rowdot(lib, eager, kind, y_t):
    nd = eager
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(3)
    for what, R, K, nc in _rowdot_cases(dt):
        for ints in ([False, True] if dt == np.float16 else [False]):
            a, b = _data(rng, (R, K), dt, ints), _data(rng, (K, nc), dt, ints)
            da, db = nd.asarray(a), (nd.asarray(np.ascontiguousarray(b.T)).T if y_t else nd.asarray(b))
            n0 = _runs(lib)
            r1 = _mm(nd, da, db, wide).get()
            assert _runs(lib) - n0 == 1, (kind, what)
            r2 = _mm(nd, da, db, wide).get()
            assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), (kind, what)
            if ints:
                _check_exact_ints(r1, a, b, wide, (kind, what))
            else:
                _check(r1, a, b, dt, wide, (kind, what))


# ---- 5. weighted column sum (X unit-stride along r) ------------------------------------------------------------------------------------
# (batch, R, K, nc) -> k_skinny_colsum<kind, NCT, 8>. R = one strip + V (a multiple of V, not of the strip); K = 2024: NB = 63 bands
# (the ticket merge), 2024 rows are no multiple of the 252 a round of the bands' waves takes, and waves end on a partial batch;
# batch 512 of K = 64 with a broadcast X: 1024 strips, NB = 1 (no partials, no ticket).
def _colsum_cases(dt):
    r = 64 * V[dt] + V[dt]
    return [("NB 63, NCT 1", 1, r, 2024, 1), ("NB 63, NCT 4 (3 live)", 1, r, 2024, 3), ("NB 63, NCT 8", 1, r, 2024, 8), ("NB 63, NCT 2", 1, r, 2024, 2),
            ("NB 1, batch 512, X broadcast, NCT 8 (5 live)", 512, r, 64, 5)]


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_colsum(lib, eager, kind):
    nd = eager
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(4)
    for what, batch, R, K, nc in _colsum_cases(dt):
        for ints in ([False, True] if dt == np.float16 else [False]):
            xt = _data(rng, (K, R), dt, ints)                    # X = xt.T: r is the unit-stride axis
            b = _data(rng, (batch, K, nc) if batch > 1 else (K, nc), dt, ints)
            da, db = nd.asarray(xt).T, nd.asarray(b)
            n0 = _runs(lib)
            r1 = _mm(nd, da, db, wide).get()
            assert _runs(lib) - n0 == 1, (kind, what)
            r2 = _mm(nd, da, db, wide).get()
            assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), (kind, what)
            if ints:
                _check_exact_ints(r1, xt.T, b, wide, (kind, what))
            else:
                _check(r1, xt.T, b, dt, wide, (kind, what))


# ---- 6. few outputs under a long k ---------------------------------------------------------------------------------------------------------
# (M, N) -> k_longk_partial / k_longk_finish<kind, TM, TN>: 1x1, 2x2, 4x4 (4 x 3 live), 8x1, 1x8, 8x8 (5 x 7 live); K = 512 (the floor:
# one block per patch) and 3 * 4096 + 40 (four blocks, the last one short).
LONGK = [(1, 1), (2, 2), (4, 3), (8, 1), (1, 8), (5, 7)]


@gpu
@pytest.mark.parametrize("K", [512, 3 * 4096 + 40])
@pytest.mark.parametrize("kind", list(KINDS))
def test_longk(lib, eager, kind, K):
    nd = eager
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(5)
    for M, N in LONGK:
        for ints in ([False, True] if dt == np.float16 else [False]):
            a, b = _data(rng, (M, K), dt, ints), _data(rng, (K, N), dt, ints)
            da, db = nd.asarray(a), nd.asarray(b)
            n0 = _runs(lib)
            r1 = _mm(nd, da, db, wide).get()
            assert _runs(lib) - n0 == 2, (kind, M, N)
            r2 = _mm(nd, da, db, wide).get()
            assert np.array_equal(r1.view(np.uint8), r2.view(np.uint8)), (kind, M, N)
            if ints:
                _check_exact_ints(r1, a, b, wide, (kind, M, N))
            else:
                _check(r1, a, b, dt, wide, (kind, M, N))


# ---- 7. layouts, vectors, batches, broadcast, out= -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_layouts_vectors_batches_out(lib, eager, kind):
    nd = eager
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(6)
    # thin N and thin M in the four layouts (views): row dot or column sum by the big operand's order
    for M, K, N in [(1024, 1024, 4), (4, 1024, 1024)]:
        a, b = _data(rng, (M, K), dt), _data(rng, (K, N), dt)
        for ta in (False, True):
            for tb in (False, True):
                da = nd.asarray(np.ascontiguousarray(a.T)).T if ta else nd.asarray(a)
                db = nd.asarray(np.ascontiguousarray(b.T)).T if tb else nd.asarray(b)
                n0 = _runs(lib)
                got = _mm(nd, da, db, wide).get()
                assert _runs(lib) - n0 == 1, (kind, M, N, ta, tb)
                _check(got, a, b, dt, wide, (kind, M, N, ta, tb))
    # 1-D operands
    m, v, w = _data(rng, (1024, 1024), dt), _data(rng, (1024,), dt), _data(rng, (1024,), dt)
    dm, dv, dw = nd.asarray(m), nd.asarray(v), nd.asarray(w)
    n0 = _runs(lib)
    _check(_mm(nd, dv, dm, wide).get()[None], v[None], m, dt, wide, (kind, "v @ M"))
    _check(_mm(nd, dm, dv, wide).get()[:, None], m, v[:, None], dt, wide, (kind, "M @ v"))
    _check(np.asarray(_mm(nd, dv, dw, wide).get())[None, None], v[None], w[:, None], dt, wide, (kind, "v @ w"))
    assert _runs(lib) - n0 == 4, kind
    if wide is None:
        _check(np.asarray(nd.dot(dv, dw).get())[None, None], v[None], w[:, None], dt, wide, (kind, "dot"))
    # a batch of 2; a stride-0 (broadcast) big operand
    a, b = _data(rng, (2, 512, 1024), dt), _data(rng, (2, 1024, 3), dt)
    n0 = _runs(lib)
    _check(_mm(nd, nd.asarray(a), nd.asarray(b), wide).get(), a, b, dt, wide, (kind, "batch 2"))
    _check(_mm(nd, nd.asarray(a[0]), nd.asarray(b), wide).get(), a[0], b, dt, wide, (kind, "broadcast X"))
    assert _runs(lib) - n0 == 2, kind
    # out= as a view: rows 8 .. 1031 of a taller array (C-contiguous, as matmul's out must be), the rows around it untouched
    a, b = _data(rng, (1024, 1024), dt), _data(rng, (1024, 4), dt)
    odt = wide or dt
    host = np.full((1040, 4), 7, dtype=odt)
    full = nd.asarray(host)
    view = full[8:1032]
    n0 = _runs(lib)
    r = _mm(nd, nd.asarray(a), nd.asarray(b), wide, out=view)
    assert r is view and _runs(lib) - n0 == 1
    res = full.get()
    assert np.array_equal(res[:8], host[:8]) and np.array_equal(res[1032:], host[1032:])
    _check(res[8:1032], a, b, dt, wide, (kind, "out="))


# ---- 8. values ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["i8", "i8->i32", "u8"])
def test_integer_extremes(lib, eager, kind):
    nd = eager
    dt, wide = KINDS[kind]
    lo, hi = (-128, 127) if dt == np.int8 else (0, 255)
    for R, K, t in [(512, 2048, False), (1040, 2048, True)]:      # row dot; column sum
        a = np.full((R, K), lo, dtype=dt)
        a[1::3] = hi
        a[2::3, ::2] = 0
        for fill in (lo, hi):
            b = np.full((K, 2), fill, dtype=dt)
            b[::5, 1] = hi if fill == lo else lo
            da = nd.asarray(np.ascontiguousarray(a.T)).T if t else nd.asarray(a)
            n0 = _runs(lib)
            got = _mm(nd, da, nd.asarray(b), wide).get()
            assert _runs(lib) - n0 == 1
            _check(got, a, b, dt, wide, (kind, R, K, t, fill))


@gpu
def test_int32_sums_wrap_as_numpy(lib, eager):
    """int8 -> int32 past 2**31: 139264 products of 127 * 127 are 2 246 189 056; every row a multiple of 127 * (its row sum)"""
    nd = eager
    R, K = 512, 139264
    a = np.full((R, K), 127, dtype=np.int8)
    a[1::2] = -127
    a[2, :1000] = 3
    a[3, 5::7] = -128
    v = np.full((K,), 127, dtype=np.int8)
    exp = (a.sum(axis=1, dtype=np.int64) * 127).astype(np.int32)      # NumPy's wrap
    assert abs(int(a[0].sum(dtype=np.int64)) * 127) > 2 ** 31
    da, dv = nd.asarray(a), nd.asarray(v)
    n0 = _runs(lib)
    got = nd.matmul(da, dv, dtype=np.int32).get()
    assert _runs(lib) - n0 == 1
    assert got.dtype == np.int32 and np.array_equal(got, exp)
    assert np.array_equal(nd.matmul(da, dv).get(), exp.astype(np.int8))
    # the same k through the long-k kernels: rows 0 .. 7 against the vector
    got = nd.matmul(nd.asarray(a[:8]), dv, dtype=np.int32).get()
    assert np.array_equal(got, exp[:8])


@gpu
@pytest.mark.parametrize("form", ["rowdot", "colsum", "longk"])
@pytest.mark.parametrize("wide", [None, np.float32])
def test_float16_specials_match_numpy(lib, eager, wide, form):
    nd = eager
    rng = np.random.default_rng(8)
    R, K, nc = (8, 4096, 4) if form == "longk" else (1024, 2048, 4)
    a = rng.standard_normal((R, K)).astype(np.float16)
    b = rng.standard_normal((K, nc)).astype(np.float16)
    a[1, :] = 300.0                       # 300 * 300 * K: past 65504 -> inf in float16, finite in float32
    b[:, 1] = 300.0
    a[2, 3] = np.inf
    a[3, 4] = -np.inf
    a[4, 7] = np.nan
    b[3, 2] = 0.0                         # inf * 0 -> NaN
    a[5, K - 1] = np.inf                  # the last element of a row
    a[6, :] = np.float16(6e-8)            # subnormal operands
    b[:, 3] = np.float16(-6e-8)
    b[9, 0] = np.inf
    da = nd.asarray(np.ascontiguousarray(a.T)).T if form == "colsum" else nd.asarray(a)
    n0 = _runs(lib)
    got = _mm(nd, da, nd.asarray(b), wide).get()
    assert _runs(lib) - n0 == (2 if form == "longk" else 1)
    with np.errstate(all="ignore"):
        exp = np.matmul(a, b, dtype=wide) if wide is not None else np.matmul(a, b)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        exact, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
    assert got.dtype == exp.dtype
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(np.isposinf(got), np.isposinf(exp)) and np.array_equal(np.isneginf(got), np.isneginf(exp))
    fin = np.isfinite(exp) & np.isfinite(exact)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(exact[fin]).astype(exp.dtype)).astype(np.float64)
    assert np.all(np.abs(got[fin].astype(np.float64) - exact[fin]) <= ulp / 2 + K * 2.0 ** -23 * mag[fin])
    assert got[6, 2] != 0                 # (subnormal operands are not flushed)


# ---- 9. graph capture -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["f16", "i8->i32"])
def test_captured_product_replays_the_eager_bits(lib, eager, kind):
    nd = eager
    from minidiff_amd import graph
    assert graph.can_capture(lib)
    dt, wide = KINDS[kind]
    rng = np.random.default_rng(9)
    xt, m, v = _data(rng, (2048, 1040), dt), _data(rng, (1024, 2048), dt), _data(rng, (2048,), dt)
    dxt, dm, dv = nd.asarray(xt), nd.asarray(m), nd.asarray(v)
    ref = [_mm(nd, dm, dv, wide).get(), _mm(nd, dxt.T, dv, wide).get()]      # row dot; column sum with band partials
    n0 = _runs(lib)
    sweep = graph.CapturedSweep(lambda: [_mm(nd, dm, dv, wide), _mm(nd, dxt.T, dv, wide)], warmup=0)
    assert _runs(lib) - n0 == 2
    try:
        for _ in range(2):
            out = sweep.replay()
            lib.sync()
            for o, r in zip(out, ref):
                assert np.array_equal(o.get().view(np.uint8), r.view(np.uint8)), kind
        assert _runs(lib) - n0 == 2          # (a replay issues nothing)
    finally:
        sweep.close()
