"""matmul(a, b, dtype=X): NumPy's keyword, honoured for every dtype of the table; float16 @ float16 -> float32 and int8 @ int8 -> int32 are
ONE native mdhip_matmul on the operands as they are (csrc/gemm_narrow.hip k_gemm_widen_*: the accumulators of the low-precision matrix
cores stored as they are; planned by gemm.hip plan_widen; plain loops in csrc/md_dispatch.h for the CPU double).

Numerical contract. int8 -> int32: bit for bit NumPy for any K (both sides wrap modulo 2**32). float16 -> float32: every product of two
float16 values is exact in float32, so only the order of the float32 additions differs: per element
|got - exact| <= K * 2**-23 * (|a| @ |b|) + ulp32(exact) / 2 with `exact` the float64 product. That bound is loose for large K (a result
wrongly rounded to float16 would pass at K = 512), so integer-valued float16 operands (-8 .. 8, K <= 1024: every partial sum an integer
below 2**24) must give the integer product bit for bit, odd values above 2048 included. NaN / inf pattern of NumPy; same bits run to run.

Unmarked tests run on whatever library the process bound (the CPU double without a device); the @gpu tests add the large shapes."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOOL, I32, I64, F32, F64, I8, I16, U8, U16, U32, U64, F16 = range(12)
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]   # NN, NT, TN, TT
# (M, K, N): the grids of tests/test_narrow_matmul.py. SMALL: what the CPU double's plain loops finish in seconds.
BIG_SHAPES = [(4096, 4096, 4096), (1024, 4096, 4096), (4097, 4100, 4096), (257, 515, 130), (300, 160, 208), (144, 256, 208), (1000, 1040, 520),
              (129, 48, 257), (3, 5, 7), (8, 4096, 1024), (2048, 4096, 5), (64, 96, 64)]
SMALL_SHAPES = [(257, 515, 130), (300, 160, 208), (144, 256, 208), (129, 48, 257), (3, 5, 7), (8, 1024, 256), (512, 1024, 5), (64, 96, 64)]
BIG_LAYOUT_SHAPES = [(512, 256, 384), (300, 160, 200), (144, 256, 208), (272, 160, 336), (1024, 1024, 1024)]
SMALL_LAYOUT_SHAPES = [(256, 128, 128), (300, 160, 200), (144, 256, 208), (272, 160, 336)]


def _nd():
    from minidiff_amd import ndarray as nd
    return nd


def _layout(x, t):
    """x (r, c) as a view with the given memory order: t = False C order, True the transpose of a C-order (c, r) array."""
    nd = _nd()
    return nd.asarray(np.ascontiguousarray(x.T)).T if t else nd.asarray(x)


def _i8(rng, shape):
    x = rng.integers(-128, 128, shape).astype(np.int8)
    flat = x.reshape(-1)
    flat[: min(4, flat.size)] = np.array([-128, 127, 0, -1], dtype=np.int8)[: min(4, flat.size)]
    return x


def _i32_ref(a, b):
    # the exact integer sum from float64 BLAS (|sum| <= K * 2**14, far below 2**53), wrapped to int32 as NumPy's loop wraps
    return np.rint(np.matmul(a.astype(np.float64), b.astype(np.float64))).astype(np.int64).astype(np.int32)


def _f32_bound_ok(got, a, b):
    assert got.dtype == np.float32
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = np.matmul(a64, b64)
    mag = np.matmul(np.abs(a64), np.abs(b64))
    K = a.shape[-1]
    ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    bound = ulp / 2 + K * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - exact)
    bad = ~(err <= bound)
    return not bad.any(), int(bad.sum())


def _h(rng, shape):
    return rng.standard_normal(shape).astype(np.float16)


def _mm32(a, b, **kw):
    nd = _nd()
    return nd.matmul(a if isinstance(a, nd.DeviceArray) else nd.asarray(a), b if isinstance(b, nd.DeviceArray) else nd.asarray(b), **kw)


# ---- 1. call log: one native call, no conversion ----------------------------------------------------------------------------------
SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from minidiff_amd import _capi
if %(double)r:
    _capi.use_library(%(double)r)
from minidiff_amd import ndarray as nd
rng = np.random.default_rng(0)
h = nd.asarray(rng.standard_normal((48, 40)).astype(np.float16))
g = nd.asarray(rng.standard_normal((40, 40)).astype(np.float16))
i = nd.asarray(rng.integers(-128, 128, (48, 40)).astype(np.int8))
print("BEGIN", flush=True)
r = [nd.matmul(h, g, dtype=np.float32), nd.matmul(i, i.T, dtype=np.int32)]
assert [x.dtype for x in r] == [np.float32, np.int32]
r = [x.get() for x in r]
"""


def _call_log(tmp_path, on_gpu, lazy="0"):
    from conftest import HOST_DOUBLE
    log = tmp_path / "calls.jsonl"
    env = dict(os.environ, MDHIP_TRACE=str(log), MDHIP_LAZY=lazy)
    p = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "double": "" if on_gpu else HOST_DOUBLE}],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [json.loads(line) for line in log.read_text().splitlines()]
    first = next(k for k, r in enumerate(recs) if r["call"] == "matmul")
    tail = recs[first:]
    mm = [tuple(a["dtype"] for a in r["args"] if isinstance(a, dict)) for r in tail if r["call"] == "matmul"]
    assert mm == [(F16, F16, F32), (I8, I8, I32)], mm
    assert [r for r in tail if r["call"] == "convert"] == []


@pytest.mark.parametrize("lazy", ["0", "1"])
def test_widening_products_issue_one_native_call(tmp_path, lib, on_gpu, lazy):
    _call_log(tmp_path, on_gpu, lazy)


@gpu
@pytest.mark.parametrize("lazy", ["0", "1"])
def test_widening_products_issue_one_native_call_on_the_gpu(tmp_path, lib, on_gpu, lazy):
    _call_log(tmp_path, on_gpu, lazy)


# ---- 2. int8 -> int32: bit for bit ------------------------------------------------------------------------------------------------
def _int_shape(M, K, N):
    rng = np.random.default_rng(M * 7 + K * 3 + N)
    a, b = _i8(rng, (M, K)), _i8(rng, (K, N))
    got = _mm32(a, b, dtype=np.int32).get()
    assert got.dtype == np.int32 and got.shape == (M, N) and np.array_equal(got, _i32_ref(a, b))


def _int_layout(ta, tb, M, K, N):
    rng = np.random.default_rng(11)
    a, b = _i8(rng, (M, K)), _i8(rng, (K, N))
    got = _mm32(_layout(a, ta), _layout(b, tb), dtype="int32").get()
    assert got.dtype == np.int32 and np.array_equal(got, _i32_ref(a, b)), (ta, tb)


@pytest.mark.parametrize("M,K,N", SMALL_SHAPES)
def test_int8_to_int32_is_exact(lib, M, K, N):
    _int_shape(M, K, N)


@gpu
@pytest.mark.parametrize("M,K,N", BIG_SHAPES)
def test_int8_to_int32_is_exact_on_the_gpu(lib, M, K, N):
    _int_shape(M, K, N)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,K,N", SMALL_LAYOUT_SHAPES)
def test_int8_to_int32_layouts(lib, ta, tb, M, K, N):
    _int_layout(ta, tb, M, K, N)


@gpu
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,K,N", BIG_LAYOUT_SHAPES)
def test_int8_to_int32_layouts_on_the_gpu(lib, ta, tb, M, K, N):
    _int_layout(ta, tb, M, K, N)


def _int_vectors_batches_views_out(n):
    nd = _nd()
    rng = np.random.default_rng(5)
    v, w = _i8(rng, (n,)), _i8(rng, (n,))
    r = _mm32(v, w, dtype=np.int32)
    assert r.shape == () and r.dtype == np.int32 and np.array_equal(r.get(), _i32_ref(v[None], w[:, None])[0, 0])
    m = _i8(rng, (n, 300))
    assert np.array_equal(_mm32(v, m, dtype=np.int32).get(), _i32_ref(v[None], m)[0])
    assert np.array_equal(_mm32(m.T.copy(), v, dtype=np.int32).get(), _i32_ref(m.T, v[:, None])[:, 0])
    a, b = _i8(rng, (6, 128, 256)), _i8(rng, (6, 256, 128))
    assert np.array_equal(_mm32(a, b, dtype=np.int32).get(), _i32_ref(a, b))
    a, b = _i8(rng, (4, 1, 128, 64)), _i8(rng, (3, 64, 96))
    got = _mm32(a, b, dtype=np.int32).get()
    assert got.shape == (4, 3, 128, 96) and np.array_equal(got, _i32_ref(a, b))
    a, b = _i8(rng, (5, 32, 64)), _i8(rng, (64, 48))                    # a batch against one matrix: one product of 5 * 32 rows
    assert np.array_equal(_mm32(a, b, dtype=np.int32).get(), _i32_ref(a, b))
    big = _i8(rng, (257, 261))
    da = nd.asarray(big)
    got = nd.matmul(da[1:, 1:], da[1:, 1:].T, dtype=np.int32).get()      # a view off every alignment
    assert np.array_equal(got, _i32_ref(big[1:, 1:], big[1:, 1:].T))
    got = nd.matmul(da[::2, :256], da[:256, ::3], dtype=np.int32).get()  # strided rows / columns
    assert np.array_equal(got, _i32_ref(big[::2, :256], big[:256, ::3]))
    a, b = _i8(rng, (256, 512)), _i8(rng, (512, 128))
    out = nd.zeros((256, 128), dtype=np.int32)
    r = nd.matmul(nd.asarray(a), nd.asarray(b), out=out, dtype=np.int32)
    assert r is out and np.array_equal(out.get(), _i32_ref(a, b))
    # empty products
    z = _mm32(np.zeros((5, 0), np.int8), np.zeros((0, 7), np.int8), dtype=np.int32)
    assert z.dtype == np.int32 and np.array_equal(z.get(), np.zeros((5, 7), np.int32))
    z = _mm32(np.zeros((0, 4), np.int8), np.zeros((4, 7), np.int8), dtype=np.int32)
    assert z.dtype == np.int32 and z.shape == (0, 7)


def test_int8_to_int32_vectors_batches_views_out(lib):
    _int_vectors_batches_views_out(1024)


@gpu
def test_int8_to_int32_vectors_batches_views_out_on_the_gpu(lib):
    _int_vectors_batches_views_out(4096)


def _int_overflow(K, rows):
    a = np.full((rows, K), 127, dtype=np.int8)
    b = np.full((K, rows), 127, dtype=np.int8)
    a[0, :7] = 3
    exp = np.matmul(a[:2], b[:, :1], dtype=np.int32)                    # NumPy's own int32 loop on two rows (b is constant)
    assert exp[1, 0] == np.int64(K * 127 * 127).astype(np.int32) and K * 127 * 127 >= 2 ** 31
    got = _mm32(a, b, dtype=np.int32).get()
    assert np.array_equal(got[0], np.full(rows, exp[0, 0])) and np.array_equal(got[1:], np.full((rows - 1, rows), exp[1, 0]))


def test_int8_to_int32_overflow_wraps_like_numpy(lib):
    _int_overflow(200000, 16)


@gpu
def test_int8_to_int32_overflow_wraps_like_numpy_on_the_gpu(lib):
    _int_overflow(200000, 16)       # few outputs under a long k
    _int_overflow(1 << 18, 256)     # the matrix cores


# ---- 3. float16 -> float32 --------------------------------------------------------------------------------------------------------
def _f16_shape(M, K, N):
    rng = np.random.default_rng(M + 5 * K + 7 * N)
    a, b = _h(rng, (M, K)), _h(rng, (K, N))
    got = _mm32(a, b, dtype=np.float32).get()
    ok, nbad = _f32_bound_ok(got, a, b)
    assert got.shape == (M, N) and ok, nbad


def _f16_layout(ta, tb, M, K, N):
    rng = np.random.default_rng(3)
    a, b = _h(rng, (M, K)), _h(rng, (K, N))
    ok, nbad = _f32_bound_ok(_mm32(_layout(a, ta), _layout(b, tb), dtype=np.dtype("float32")).get(), a, b)
    assert ok, (ta, tb, nbad)


@pytest.mark.parametrize("M,K,N", SMALL_SHAPES)
def test_float16_to_float32_within_bound(lib, M, K, N):
    _f16_shape(M, K, N)


@gpu
@pytest.mark.parametrize("M,K,N", [(s if s != (1000, 1040, 520) else (1000, 1032, 520)) for s in BIG_SHAPES])
def test_float16_to_float32_within_bound_on_the_gpu(lib, M, K, N):
    _f16_shape(M, K, N)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,K,N", SMALL_LAYOUT_SHAPES)
def test_float16_to_float32_layouts(lib, ta, tb, M, K, N):
    _f16_layout(ta, tb, M, K, N)


@gpu
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,K,N", BIG_LAYOUT_SHAPES)
def test_float16_to_float32_layouts_on_the_gpu(lib, ta, tb, M, K, N):
    _f16_layout(ta, tb, M, K, N)


def _f16_exact(shapes):
    """Integer-valued operands: every partial sum is an integer below 2**24 — exact in float32 in any order, not in float16."""
    for M, K, N in shapes:
        for ta, tb in LAYOUTS:
            rng = np.random.default_rng(M + K + N)
            a = rng.integers(-3, 9, (M, K)).astype(np.float16)      # (off centre: the sums reach the thousands)
            b = rng.integers(-3, 9, (K, N)).astype(np.float16)
            exp = np.matmul(a.astype(np.int64), b.astype(np.int64))
            assert np.abs(exp).max() < 2 ** 24 and K * 64 < 2 ** 24
            if K >= 512:
                assert ((np.abs(exp) > 2048) & (exp % 2 != 0)).any()        # values float16 cannot hold
            got = _mm32(_layout(a, ta), _layout(b, tb), dtype=np.float32).get()
            assert got.dtype == np.float32 and np.array_equal(got, exp.astype(np.float32)), (M, K, N, ta, tb)


def test_float16_to_float32_integer_operands_are_exact(lib):
    _f16_exact([(128, 1024, 128), (144, 512, 208), (33, 1000, 17), (7, 9, 5), (4, 1024, 64)])


@gpu
def test_float16_to_float32_integer_operands_are_exact_on_the_gpu(lib):
    _f16_exact([(1024, 1024, 1024), (512, 1024, 384), (300, 1000, 200), (128, 768, 128), (8, 1024, 512)])


def _f16_vectors_batches_views_out(n):
    nd = _nd()
    rng = np.random.default_rng(9)
    v, w = _h(rng, n), _h(rng, n)
    r = _mm32(v, w, dtype=np.float32)
    assert r.shape == () and _f32_bound_ok(np.asarray(r.get())[None, None], v[None], w[:, None])[0]
    m = _h(rng, (n, 300))
    assert _f32_bound_ok(_mm32(v, m, dtype=np.float32).get()[None], v[None], m)[0]
    assert _f32_bound_ok(_mm32(m.T.copy(), v, dtype=np.float32).get()[:, None], m.T, v[:, None])[0]
    a, b = _h(rng, (6, 128, 256)), _h(rng, (6, 256, 128))
    assert _f32_bound_ok(_mm32(a, b, dtype=np.float32).get(), a, b)[0]
    a, b = _h(rng, (4, 1, 128, 64)), _h(rng, (3, 64, 96))
    got = _mm32(a, b, dtype=np.float32).get()
    assert got.shape == (4, 3, 128, 96) and _f32_bound_ok(got, a, b)[0]
    a, b = _h(rng, (5, 32, 64)), _h(rng, (64, 48))
    assert _f32_bound_ok(_mm32(a, b, dtype=np.float32).get(), a, b)[0]
    big = _h(rng, (257, 261))
    da = nd.asarray(big)
    assert _f32_bound_ok(nd.matmul(da[1:, 1:], da[1:, 1:].T, dtype=np.float32).get(), big[1:, 1:], big[1:, 1:].T)[0]
    assert _f32_bound_ok(nd.matmul(da[::2, :256], da[:256, ::3], dtype=np.float32).get(), big[::2, :256], big[:256, ::3])[0]
    a, b = _h(rng, (256, 512)), _h(rng, (512, 256))
    out = nd.zeros((256, 256), dtype=np.float32)
    assert nd.matmul(nd.asarray(a), nd.asarray(b), out=out, dtype=np.float32) is out and _f32_bound_ok(out.get(), a, b)[0]
    z = _mm32(np.zeros((5, 0), np.float16), np.zeros((0, 7), np.float16), dtype=np.float32)
    assert z.dtype == np.float32 and np.array_equal(z.get(), np.zeros((5, 7), np.float32))


def test_float16_to_float32_vectors_batches_views_out(lib):
    _f16_vectors_batches_views_out(1024)


@gpu
def test_float16_to_float32_vectors_batches_views_out_on_the_gpu(lib):
    _f16_vectors_batches_views_out(4096)


def _f16_specials(M, K, N):
    rng = np.random.default_rng(1)
    a, b = _h(rng, (M, K)), _h(rng, (K, N))
    a[0, 0] = np.nan
    a[1, :] = 300.0                      # 300 * 300 * K: past float16's range, finite in float32
    b[:, 1] = 300.0
    a[2, 3] = np.inf
    b[3, :] = 0.0                        # inf * 0 -> NaN
    a[3, 4] = -np.inf
    a[4, :] = np.float16(6e-8)           # subnormal inputs
    b[:, 2] = np.float16(-6e-8)
    with np.errstate(all="ignore"):
        exp = np.matmul(a, b, dtype=np.float32)
    got = _mm32(a, b, dtype=np.float32).get()
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(np.isposinf(got), np.isposinf(exp)) and np.array_equal(np.isneginf(got), np.isneginf(exp))
    assert np.isfinite(got[1, 1]) and got[1, 1] > 65504
    with np.errstate(all="ignore"):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        exact, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
        fin = np.isfinite(exp) & np.isfinite(exact)
        bound = np.spacing(np.abs(exact[fin]).astype(np.float32)).astype(np.float64) / 2 + K * 2.0 ** -23 * mag[fin]
    assert np.all(np.abs(got[fin].astype(np.float64) - exact[fin]) <= bound)


@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (7, 9, 5)])
def test_float16_to_float32_specials_match_numpy(lib, M, K, N):
    _f16_specials(M, K, N)


@gpu
@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (7, 9, 5)])
def test_float16_to_float32_specials_match_numpy_on_the_gpu(lib, M, K, N):
    _f16_specials(M, K, N)


def _deterministic(n):
    nd = _nd()
    rng = np.random.default_rng(4)
    a, b = nd.asarray(_h(rng, (n, n))), nd.asarray(_h(rng, (n, n)))
    r1 = nd.matmul(a, b, dtype=np.float32).get()
    r2 = nd.matmul(a, b, dtype=np.float32).get()
    assert np.array_equal(r1.view(np.uint32), r2.view(np.uint32))


def test_float16_to_float32_is_deterministic(lib):
    _deterministic(256)


@gpu
def test_float16_to_float32_is_deterministic_on_the_gpu(lib):
    _deterministic(4096)


# ---- 4. the keyword against NumPy, every dtype of the table -----------------------------------------------------------------------
TABLE = [np.bool_, np.int8, np.uint8, np.int16, np.int32, np.int64, np.float16, np.float32, np.float64]


def _operand(rng, dt, shape):
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, shape).astype(dt)
    if dt.kind == "u":
        return rng.integers(0, 6, shape).astype(dt)
    if dt.kind == "i":
        return rng.integers(-5, 6, shape).astype(dt)
    return (rng.integers(-20, 21, shape) / 4).astype(dt)     # quarters: every product and sum here is exact in float16 and wider


def _keyword_grid(lazy):
    nd = _nd()
    rng = np.random.default_rng(8)
    n_ok = n_err = 0
    for da, db, dt in itertools.product(TABLE, TABLE, TABLE):
        a, b = _operand(rng, da, (6, 5)), _operand(rng, db, (5, 4))
        try:
            with np.errstate(all="ignore"):
                exp = np.matmul(a, b, dtype=dt)
        except TypeError as e:
            exp = e
        if isinstance(exp, Exception):
            with pytest.raises(TypeError):
                nd.matmul(nd.asarray(a), nd.asarray(b), dtype=dt)
            n_err += 1
            continue
        got = nd.matmul(nd.asarray(a), nd.asarray(b), dtype=dt)
        assert got.dtype == exp.dtype == np.dtype(dt), (da, db, dt, got.dtype)
        g = got.get()
        if exp.dtype.kind == "f":
            # the operands' values make every sum exact except where float16 overflows or rounds a wide integer operand: usual tolerances
            assert np.allclose(g, exp, rtol=1e-3 if exp.dtype == np.float16 else 1e-6, atol=0, equal_nan=True), (da, db, dt, g, exp)
        else:
            assert np.array_equal(g, exp), (da, db, dt, g, exp)
        n_ok += 1
    assert n_ok > 200 and n_err > 200, (n_ok, n_err)


@pytest.fixture
def lazy_mode():
    """Switch lazy mode for one test and put the process's setting back."""
    nd = _nd()
    saved = nd.lazy_enabled()

    def set_lazy(on):
        nd.set_lazy(bool(on))

    yield set_lazy
    nd.set_lazy(saved)


@pytest.mark.parametrize("lazy", [False, True])
def test_dtype_keyword_matches_numpy_over_the_table(lib, lazy_mode, lazy):
    lazy_mode(lazy)
    _keyword_grid(lazy)


@gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_dtype_keyword_matches_numpy_over_the_table_on_the_gpu(lib, lazy_mode, lazy):
    lazy_mode(lazy)
    _keyword_grid(lazy)


def _keyword_details():
    nd = _nd()
    rng = np.random.default_rng(12)
    a32, b32 = rng.standard_normal((16, 24)).astype(np.float32), rng.standard_normal((24, 8)).astype(np.float32)
    # a down-cast 'same_kind' allows: the float16 product of the ROUNDED operands
    got = nd.matmul(nd.asarray(a32), nd.asarray(b32), dtype=np.float16)
    exp = np.matmul(a32, b32, dtype=np.float16)
    assert got.dtype == np.float16 and np.allclose(got.get().astype(np.float64), exp.astype(np.float64), rtol=2e-3, atol=2e-3)
    # mixed operands
    h, i = _h(rng, (16, 24)), _i8(rng, (24, 8))
    got = nd.matmul(nd.asarray(h), nd.asarray(i), dtype=np.float32)
    assert got.dtype == np.float32 and np.allclose(got.get(), np.matmul(h, i, dtype=np.float32), rtol=1e-5, atol=1e-4)
    # spellings of the dtype; None is the plain call
    for spelling in ("int32", np.int32, np.dtype(np.int32), "i4"):
        assert np.array_equal(nd.matmul(nd.asarray(i.T.copy()), nd.asarray(i), dtype=spelling).get(), _i32_ref(i.T, i))
    for x, y in ((a32, b32), (h, h.T.copy()), (i.T.copy(), i)):
        p, q = nd.matmul(nd.asarray(x), nd.asarray(y)), nd.matmul(nd.asarray(x), nd.asarray(y), dtype=None)
        assert p.dtype == q.dtype and np.array_equal(p.get().view(np.uint8), q.get().view(np.uint8))
    # errors: NumPy's TypeError for a cast 'same_kind' refuses, with the operand and both dtypes named
    for x, y, dt in ((a32, b32, np.int32), (i.T.copy(), i, np.uint32), (i.T.copy(), i, np.bool_), (h, h.T.copy(), np.int64)):
        with pytest.raises(TypeError) as ours:
            nd.matmul(nd.asarray(x), nd.asarray(y), dtype=dt)
        with pytest.raises(TypeError) as theirs:
            np.matmul(x, y, dtype=dt)
        assert "input 0" in str(ours.value) and repr(np.dtype(dt)) in str(ours.value) and repr(x.dtype) in str(ours.value)
        assert "input 0" in str(theirs.value)
    with pytest.raises(TypeError):
        nd.matmul(nd.asarray(a32), nd.asarray(b32), dtype=np.complex64)
    # out=: with dtype= it has the keyword's dtype; without, the operands' result dtype as before
    i8a, i8b = _i8(rng, (16, 24)), _i8(rng, (24, 8))
    for dt in (np.int32, np.int64, np.float32, np.int16):
        out = nd.zeros((16, 8), dtype=dt)
        r = nd.matmul(nd.asarray(i8a), nd.asarray(i8b), out=out, dtype=dt)
        exp = np.matmul(i8a, i8b, out=np.zeros((16, 8), dt), dtype=dt)
        assert r is out and out.dtype == exp.dtype and np.array_equal(out.get(), exp)
    with pytest.raises(ValueError):
        nd.matmul(nd.asarray(i8a), nd.asarray(i8b), out=nd.zeros((16, 8), dtype=np.int64), dtype=np.int32)
    with pytest.raises(ValueError):
        nd.matmul(nd.asarray(i8a), nd.asarray(i8b), out=nd.zeros((16, 8), dtype=np.int32))      # no dtype=: the loop is int8's
    out = nd.zeros((16, 8), dtype=np.int8)
    assert nd.matmul(nd.asarray(i8a), nd.asarray(i8b), out=out) is out and np.array_equal(out.get(), np.matmul(i8a, i8b))
    # the backend table forwards the keyword; functions without it in NumPy have none here
    from minidiff_amd.hip_backend import HipBackendTable
    assert HipBackendTable.matmul(nd.asarray(i8a), nd.asarray(i8b), dtype=np.int32).dtype == np.int32
    with pytest.raises(TypeError):
        nd.dot(nd.asarray(i8a), nd.asarray(i8b), dtype=np.int32)
    with pytest.raises(TypeError):
        nd.add(nd.asarray(i8a), nd.asarray(i8a), dtype=np.int32)


@pytest.mark.parametrize("lazy", [False, True])
def test_dtype_keyword_casts_spellings_errors_and_out(lib, lazy_mode, lazy):
    lazy_mode(lazy)
    _keyword_details()


@gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_dtype_keyword_casts_spellings_errors_and_out_on_the_gpu(lib, lazy_mode, lazy):
    lazy_mode(lazy)
    _keyword_details()


def test_lazy_mode_never_defers_a_call_with_dtype(lib, lazy_mode):
    nd = _nd()
    lazy_mode(True)
    rng = np.random.default_rng(2)
    a, b = nd.asarray(_h(rng, (64, 64))), nd.asarray(_h(rng, (64, 64)))
    r = nd.matmul(a, b, dtype=np.float32)
    assert r._expr is None and r.dtype == np.float32
    f = nd.asarray(rng.standard_normal((64, 64)).astype(np.float32))
    r = nd.matmul(f, f, dtype=np.float32)
    assert r._expr is None
    assert np.allclose(r.get(), np.matmul(f.get(), f.get()), rtol=1e-4, atol=1e-4)


# ---- 5. route A/B through the option hook -----------------------------------------------------------------------------------------
def _routes(mdopt, shapes):
    rng = np.random.default_rng(21)
    for M, K, N in shapes:
        i, j = _i8(rng, (M, K)), _i8(rng, (K, N))
        h, g = _h(rng, (M, K)), _h(rng, (K, N))
        res = {}
        for route in (1, 0):
            mdopt("gemm_widen", route)
            res[route] = (_mm32(i, j, dtype=np.int32).get(), _mm32(h, g, dtype=np.float32).get())
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[1][0], _i32_ref(i, j)), (M, K, N)
        for route in (0, 1):
            ok, nbad = _f32_bound_ok(res[route][1], h, g)
            assert ok, (M, K, N, route, nbad)


def test_native_and_conversion_routes_agree(lib, mdopt):
    _routes(mdopt, [(128, 256, 128), (144, 160, 208), (33, 70, 17), (4, 1024, 64)])


@gpu
def test_native_and_conversion_routes_agree_on_the_gpu(lib, mdopt):
    _routes(mdopt, [(1024, 1024, 1024), (512, 4096, 384), (300, 160, 200), (128, 8192, 128), (8, 4096, 1024), (33, 70, 17)])


# ---- 6. C-ABI: the triples through descriptors ------------------------------------------------------------------------------------
def _capi_triples(lib):
    nd = _nd()
    rng = np.random.default_rng(6)
    np_of = {F16: np.float16, I8: np.int8, U8: np.uint8, F32: np.float32, F64: np.float64, I32: np.int32, I64: np.int64}

    def call(adt, bdt, cdt):
        a = nd.asarray(rng.integers(-4, 5, (1, 16, 32)).astype(np_of[adt]))
        b = nd.asarray(rng.integers(-4, 5, (1, 32, 16)).astype(np_of[bdt]))
        c = nd.zeros((1, 16, 16), dtype=np_of[cdt])
        lib.matmul(a.desc(), b.desc(), c.desc())
        return a.get(), b.get(), c.get()

    for triple in ((F16, F16, F32), (I8, I8, I32)):
        a, b, c = call(*triple)
        assert np.array_equal(c, np.matmul(a.astype(np.int64), b.astype(np.int64)).astype(c.dtype))
    for triple in ((F16, F16, F64), (I8, I8, I64), (U8, U8, I32), (F16, I8, F32), (F32, F32, F16)):
        with pytest.raises(TypeError):       # MDHIP_ETYPE
            call(*triple)


def test_capi_accepts_the_two_widening_triples_only(lib):
    _capi_triples(lib)


@gpu
def test_capi_accepts_the_two_widening_triples_only_on_the_gpu(lib):
    _capi_triples(lib)


# ---- 7. large shapes (GPU) ------------------------------------------------------------------------------------------------------------
def _sampled(kind, M, K, N, ta, tb, seed=0):
    """The product on the device, sampled rows against float64 on the host (int8: exact on the sample)."""
    rng = np.random.default_rng(seed + M + K + N)
    if kind == "i8":
        a, b = rng.integers(-128, 128, (M, K)).astype(np.int8), rng.integers(-128, 128, (K, N)).astype(np.int8)
    else:
        a, b = _h(rng, (M, K)), _h(rng, (K, N))
    got = _mm32(_layout(a, ta), _layout(b, tb), dtype=np.int32 if kind == "i8" else np.float32).get()
    assert got.shape == (M, N)
    rows = np.unique(np.concatenate([rng.integers(0, M, 6), [0, M - 1]]))
    if kind == "i8":
        assert np.array_equal(got[rows], _i32_ref(a[rows], b)), (M, K, N, ta, tb)
    else:
        ok, nbad = _f32_bound_ok(got[rows], a[rows], b)
        assert ok, (M, K, N, ta, tb, nbad)


@gpu
@pytest.mark.parametrize("kind", ["f16", "i8"])
@pytest.mark.parametrize("ta,tb", LAYOUTS[:3])
@pytest.mark.parametrize("M,K,N", [(4096, 4096, 4096), (8192, 4096, 4096)])
def test_large_products(lib, kind, ta, tb, M, K, N):
    _sampled(kind, M, K, N, ta, tb)


@gpu
@pytest.mark.parametrize("kind", ["f16", "i8"])
def test_large_ragged_product(lib, kind):
    _sampled(kind, 4097, 4096, 4100, False, False)


@gpu
@pytest.mark.parametrize("kind", ["f16", "i8"])
@pytest.mark.parametrize("M,K,N", [(128, 2048, 128), (128, 4096, 128), (256, 2048, 256), (256, 8192, 256), (384, 4096, 384), (384, 8192, 384),
                                   (512, 8192, 512), (1024, 8192, 1024)])
def test_few_tiles_under_a_long_k_on_both_sides_of_the_cut_over(lib, kind, M, K, N):
    # float16: 1 tile leaves the matrix cores from k ~ 2.7 K, 4 tiles from ~3.4 K, 9 from ~5 K, 18 tiles and more never (gemm.hip plan_widen)
    for ta, tb in LAYOUTS[:3]:
        _sampled(kind, M, K, N, ta, tb)


# ---- 8. ISA guard: the wide-output kernels as designed, read from the shipped library ---------------------------------------------
OBJ = os.path.join(ROOT, "minidiff_amd", "libmdhip.so")
KERNELS = {f"{'f16' if e == 2 else 'i8'} A_{'KC' if a else 'MN'} B_{'KC' if b else 'MN'}{' edge' if x else ''}":
           f"k_gemm_widen_mfmaILi{e}ELb{int(a)}ELb{int(b)}ELb{int(x)}EE"
           for e in (2, 1) for a in (False, True) for b in (False, True) for x in (False, True)}


@pytest.fixture(scope="module")
def widen_isa():
    if not os.path.exists(OBJ):
        pytest.skip("minidiff_amd/libmdhip.so not built (run __graft_entry__.build())")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_check
    ks = isa_check.raw_kernels(isa_check.disassemble(OBJ, ("k_gemm_widen_mfma",)))
    out = {}
    for label, frag in KERNELS.items():
        names = [n for n in ks if frag in n]
        assert len(names) == 1, (label, names)
        out[label] = (isa_check.analyse(names[0], ks[names[0]]), "\n".join(ks[names[0]]))
    return out


def _check_isa(widen_isa):
    assert len(widen_isa) == 16
    for label, (k, text) in widen_isa.items():
        f16 = label.startswith("f16")
        mnemonic = "v_mfma_f32_32x32x16_f16" if f16 else "v_mfma_i32_32x32x32_i8"
        assert k["mfma_total"] == 32 and k["mfma_loop"] == 32, (label, k)
        assert text.count(mnemonic) == 32, label
        assert k["dma_total"] == 24 and k["dma_loop"] >= 8, (label, k)
        if "edge" not in label:
            assert k["dma_loop_saddr"] == k["dma_loop"] and k["dma_loop_vaddr64"] == 0, (label, k)
        assert k["scratch"] == 0 and k["vmcnt0_between_barrier_and_first_read"] == 0, (label, k)
        assert k["ds_write"] == 0, (label, k)                                    # no LDS assembly of the output
        assert "v_cvt_f16_f32" not in text and "v_cvt_pk" not in text, label     # the accumulators leave as they are
        tr = "ds_read_b64_tr_b16" if f16 else "ds_read_b64_tr_b8"
        assert text.count(tr) == 32 * label.count("_MN"), (label, text.count(tr))


def test_widen_gemm_kernel_shape(widen_isa):
    _check_isa(widen_isa)


@gpu
def test_widen_gemm_kernel_shape_of_the_library_on_the_gpu_box(widen_isa):
    _check_isa(widen_isa)


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------------
def _quantised_linear(batch, d_in, d_out):
    """int8 activations and weights, the int32 sum, scaled to float32 — against the float64 computation of the same integers."""
    nd = _nd()
    rng = np.random.default_rng(31)
    x, w = rng.standard_normal((batch, d_in)), rng.standard_normal((d_in, d_out)) * 0.1
    sx, sw = np.abs(x).max() / 127, np.abs(w).max() / 127
    xq, wq = np.rint(x / sx).astype(np.int8), np.rint(w / sw).astype(np.int8)
    acc = nd.matmul(nd.asarray(xq), nd.asarray(wq), dtype=np.int32)
    y = nd.multiply(nd.astype(acc, np.float32), np.float32(sx * sw))
    exact = xq.astype(np.float64) @ wq.astype(np.float64)
    assert acc.dtype == np.int32 and np.array_equal(acc.get(), exact.astype(np.int32))
    assert y.dtype == np.float32 and np.array_equal(y.get(), exact.astype(np.int32).astype(np.float32) * np.float32(sx * sw))
    assert np.abs(y.get() - x @ w).max() < 0.05 * np.abs(x @ w).max()      # and it is the layer it quantises


def _mlp_float32_logits(batch, d, classes):
    nd = _nd()
    rng = np.random.default_rng(32)
    x, w1, w2 = _h(rng, (batch, d)), (rng.standard_normal((d, d)) * 0.1).astype(np.float16), (rng.standard_normal((d, classes)) * 0.1).astype(np.float16)
    z = nd.matmul(nd.asarray(x), nd.asarray(w1))
    hdn = nd.where(nd.greater(z, 0), z, 0)
    logits = nd.matmul(hdn, nd.asarray(w2), dtype=np.float32)
    assert hdn.dtype == np.float16 and logits.dtype == np.float32
    hn = hdn.get()
    ok, nbad = _f32_bound_ok(logits.get(), hn, w2)
    assert ok, nbad
    z64 = x.astype(np.float64) @ w1.astype(np.float64)
    assert np.allclose(hn.astype(np.float64), np.where(z64 > 0, z64, 0), rtol=2e-3, atol=2e-3)


def test_quantised_linear_layer_and_float32_logits(lib):
    _quantised_linear(64, 256, 128)
    _mlp_float32_logits(64, 128, 32)


@gpu
def test_quantised_linear_layer_and_float32_logits_on_the_gpu(lib):
    _quantised_linear(1024, 4096, 1024)
    _mlp_float32_logits(512, 1024, 256)
