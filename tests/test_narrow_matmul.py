"""float16 @ float16, int8 @ int8 and uint8 @ uint8 run natively (csrc/gemm_narrow.hip: the low-precision matrix cores, planned by
gemm.hip plan_narrow): one mdhip_matmul with the narrow dtype codes, no conversions around it.

Numerical contract. int8 / uint8: bit-for-bit NumPy (the low byte of the exact integer sum). float16: per element
|got - exact| <= ulp16(exact) / 2 + K * 2**-23 * (|a| @ |b|) with `exact` the float64 product — the float16 rounding plus a float32
accumulation error, a bound NumPy's own result meets — the NaN / inf pattern of NumPy, and the same bits run to run. The MFMA sums 16
products per instruction, so a few elements differ from NumPy's strictly sequential float32 loop (within the bound: the last bit, or
more near zero where the sum cancels); the fraction is printed by test_float16_against_numpy_loop.

References for the large cases come from float64 BLAS (exact for these integer sums, which stay far below 2**53) instead of NumPy's
own int8 / float16 loops, which have no BLAS and would take minutes at 4096^3."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
I8, U8, F16 = 5, 7, 11


# ---- call log: the product is one native call ----------------------------------------------------------------------------------
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
u = nd.asarray(rng.integers(0, 256, (40, 48)).astype(np.uint8))
print("BEGIN", flush=True)
r = [nd.matmul(h, g), nd.matmul(i, i.T), nd.matmul(u, u.T), nd.dot(h, g), nd.tensordot(h, g, axes=1)]
h @= g
r = [x.get() for x in r] + [h.get()]
"""


def _call_log(tmp_path, on_gpu):
    from conftest import HOST_DOUBLE
    log = tmp_path / "calls.jsonl"
    env = dict(os.environ, MDHIP_TRACE=str(log), MDHIP_LAZY="0")
    p = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "double": "" if on_gpu else HOST_DOUBLE}],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    recs = [json.loads(line) for line in log.read_text().splitlines()]
    # the arrays are created before the products: the log from the first product on
    first = next(k for k, r in enumerate(recs) if r["call"] == "matmul")
    tail = recs[first:]
    mm = [r for r in tail if r["call"] == "matmul"]
    assert len(mm) == 6, [r["call"] for r in tail]
    codes = [tuple(a["dtype"] for a in r["args"] if isinstance(a, dict)) for r in mm]
    assert codes == [(F16,) * 3, (I8,) * 3, (U8,) * 3, (F16,) * 3, (F16,) * 3, (F16,) * 3], codes
    # no conversion to a wide dtype and back (`@=` copies its result into the left operand: a float16 -> float16 copy)
    conv = [tuple(a["dtype"] for a in r["args"] if isinstance(a, dict)) for r in tail if r["call"] == "convert"]
    assert conv == [(F16, F16)], conv


def test_products_issue_one_native_call(tmp_path, lib, on_gpu):
    _call_log(tmp_path, on_gpu)


@gpu
def test_products_issue_one_native_call_on_the_gpu(tmp_path, lib, on_gpu):
    _call_log(tmp_path, on_gpu)


# ---- ISA guard: the kernels as designed, read from the shipped library ------------------------------------------------------------
OBJ = os.path.join(ROOT, "minidiff_amd", "libmdhip.so")
# k_gemm_narrow_mfma<ESZ, A_KC, B_KC, EDGE>, named by the operand images: for row-major arrays NN = (KC, MN), NT = (KC, KC),
# TN = (MN, MN), TT = (MN, KC)
KERNELS = {f"{'f16' if e == 2 else 'i8'} A_{'KC' if a else 'MN'} B_{'KC' if b else 'MN'}{' edge' if x else ''}":
           f"k_gemm_narrow_mfmaILi{e}ELb{int(a)}ELb{int(b)}ELb{int(x)}EE"
           for e in (2, 1) for a in (False, True) for b in (False, True) for x in (False, True)}


@pytest.fixture(scope="module")
def narrow_isa():
    if not os.path.exists(OBJ):
        pytest.skip("minidiff_amd/libmdhip.so not built (run __graft_entry__.build())")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_check
    ks = isa_check.raw_kernels(isa_check.disassemble(OBJ, ("k_gemm_narrow_mfma",)))
    out = {}
    for label, frag in KERNELS.items():
        names = [n for n in ks if frag in n]
        assert len(names) == 1, (label, names)
        out[label] = (isa_check.analyse(names[0], ks[names[0]]), "\n".join(ks[names[0]]))
    return out


def _check_isa(narrow_isa):
    for label, (k, text) in narrow_isa.items():
        mnemonic = "v_mfma_f32_32x32x16_f16" if label.startswith("f16") else "v_mfma_i32_32x32x32_i8"
        # 2 x 2 MFMA tiles x 4 k-steps per k-tile, the loop unrolled over two k-tiles; nothing outside the loop
        assert k["mfma_total"] == 32 and k["mfma_loop"] == 32, (label, k)
        assert text.count(mnemonic) == 32, label
        # 4 pieces of A and 4 of B per wave and k-tile: 8 in the prologue, 16 in the unrolled loop
        assert k["dma_total"] == 24 and k["dma_loop"] >= 8, (label, k)
        if "edge" not in label:
            assert k["dma_loop_saddr"] == k["dma_loop"] and k["dma_loop_vaddr64"] == 0, (label, k)   # scalar base + 32-bit lane offset
        assert k["scratch"] == 0 and k["vmcnt0_between_barrier_and_first_read"] == 0, (label, k)
        # float16 writes its results straight from the accumulators; int8 assembles its byte rows in LDS first
        assert (k["ds_write"] == 0) == label.startswith("f16"), (label, k)
        tr = "ds_read_b64_tr_b16" if label.startswith("f16") else "ds_read_b64_tr_b8"
        n_mn = label.count("_MN")
        # a transposed read pair per MN fragment: 2 fragments x 4 k-steps x 2 k-tiles x 2 reads per operand
        assert text.count(tr) == 32 * n_mn, (label, text.count(tr))


def test_narrow_gemm_kernel_shape(narrow_isa):
    _check_isa(narrow_isa)


@gpu
def test_narrow_gemm_kernel_shape_of_the_library_on_the_gpu_box(narrow_isa):
    _check_isa(narrow_isa)


# ---- helpers --------------------------------------------------------------------------------------------------------------------
def _nd():
    from minidiff_amd import ndarray as nd
    return nd


def _ints(rng, shape, dt):
    lo, hi = (-128, 128) if dt == np.int8 else (0, 256)
    x = rng.integers(lo, hi, shape).astype(dt)
    flat = x.reshape(-1)
    flat[: min(4, flat.size)] = np.array([lo, hi - 1, 0, hi - 1 if dt == np.uint8 else -1], dtype=np.int64)[: min(4, flat.size)].astype(dt)
    return x


def _int_ref(a, b, dt):
    # the exact integer sum (float64 BLAS: |sum| < 2**53 here), low byte — NumPy's int8 / uint8 loop result
    return np.rint(np.matmul(a.astype(np.float64), b.astype(np.float64))).astype(np.int64).astype(dt)


def _f16_bound_ok(got, a, b):
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    exact = np.matmul(a64, b64)
    mag = np.matmul(np.abs(a64), np.abs(b64))
    K = a.shape[-1]
    ulp = np.spacing(np.abs(exact).astype(np.float16)).astype(np.float64)
    bound = ulp / 2 + K * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - exact)
    bad = ~(err <= bound)
    return not bad.any(), int(bad.sum())


# (M, K, N), row-major operands. MFMA whole tiles: 4096^3, 1024x4096x4096. MFMA ragged (zero-filled DMA lanes): 300x160x208,
# 144x256x208 (M, N multiples of the 16-B chunk but not of the tile; K not a multiple of the k-tile). Rows whose length is not a
# multiple of 16 B (4097x4100x4096, 257x515x130, 1000x1040x520 for int8, 129x48x257): the generic kernel or, for large float16, the
# widened route. Tiny, thin: generic kernel / skinny hand-off.
INT_SHAPES = [(4096, 4096, 4096), (1024, 4096, 4096), (4097, 4100, 4096), (257, 515, 130), (300, 160, 208), (144, 256, 208), (1000, 1040, 520),
              (129, 48, 257), (3, 5, 7), (8, 4096, 1024), (2048, 4096, 5), (64, 96, 64)]
F16_SHAPES = [(4096, 4096, 4096), (1024, 4096, 4096), (4097, 4100, 4096), (257, 515, 130), (300, 160, 208), (144, 256, 208), (1000, 1032, 520),
              (129, 48, 257), (3, 5, 7), (8, 4096, 1024), (2048, 4096, 5), (64, 96, 64)]


def _layout(x, t):
    """x (r, c) as a view with the given memory order: t = False C order, True the transpose of a C-order (c, r) array."""
    nd = _nd()
    return nd.asarray(np.ascontiguousarray(x.T)).T if t else nd.asarray(x)


# ---- int8 / uint8: bit-for-bit ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", [np.int8, np.uint8])
@pytest.mark.parametrize("M,K,N", INT_SHAPES)
def test_int8_products_are_exact(lib, dt, M, K, N):
    nd = _nd()
    rng = np.random.default_rng(M * 7 + K * 3 + N)
    a, b = _ints(rng, (M, K), dt), _ints(rng, (K, N), dt)
    got = nd.matmul(nd.asarray(a), nd.asarray(b)).get()
    assert got.dtype == dt and np.array_equal(got, _int_ref(a, b, dt))


@gpu
@pytest.mark.parametrize("dt", [np.int8, np.uint8])
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,K,N", [(512, 256, 384), (300, 160, 200), (144, 256, 208), (272, 160, 336), (1024, 1024, 1024)])
def test_int8_layouts_are_exact(lib, dt, ta, tb, M, K, N):
    nd = _nd()
    rng = np.random.default_rng(11)
    a, b = _ints(rng, (M, K), dt), _ints(rng, (K, N), dt)
    got = nd.matmul(_layout(a, ta), _layout(b, tb)).get()
    assert np.array_equal(got, _int_ref(a, b, dt)), (ta, tb)


@gpu
@pytest.mark.parametrize("dt", [np.int8, np.uint8])
def test_int8_vectors_batches_views_out(lib, dt):
    nd = _nd()
    rng = np.random.default_rng(5)
    v, w = _ints(rng, (4096,), dt), _ints(rng, (4096,), dt)
    assert np.array_equal(nd.dot(nd.asarray(v), nd.asarray(w)).get(), _int_ref(v[None], w[:, None], dt)[0, 0])
    m = _ints(rng, (4096, 300), dt)
    assert np.array_equal(nd.matmul(nd.asarray(v), nd.asarray(m)).get(), _int_ref(v[None], m, dt)[0])
    a, b = _ints(rng, (16, 256, 256), dt), _ints(rng, (16, 256, 256), dt)
    assert np.array_equal(nd.matmul(nd.asarray(a), nd.asarray(b)).get(), _int_ref(a, b, dt))
    a, b = _ints(rng, (4, 1, 128, 64), dt), _ints(rng, (3, 64, 96), dt)
    assert np.array_equal(nd.matmul(nd.asarray(a), nd.asarray(b)).get(), _int_ref(a, b, dt))
    big = _ints(rng, (513, 517), dt)
    da = nd.asarray(big)
    got = nd.matmul(da[1:, 1:], da[1:, 1:].T).get()                  # a view off every alignment
    assert np.array_equal(got, _int_ref(big[1:, 1:], big[1:, 1:].T, dt))
    a, b = _ints(rng, (256, 512), dt), _ints(rng, (512, 128), dt)
    out = nd.zeros((256, 128), dtype=dt)
    r = nd.matmul(nd.asarray(a), nd.asarray(b), out=out)
    assert r is out and np.array_equal(out.get(), _int_ref(a, b, dt))
    x = nd.asarray(a[:, :256].copy())
    x @= nd.asarray(b[:256, :].repeat(2, axis=1))
    assert np.array_equal(x.get(), _int_ref(a[:, :256], b[:256, :].repeat(2, axis=1), dt))


@gpu
@pytest.mark.parametrize("dt", [np.int8, np.uint8])
def test_int8_int32_overflow_is_harmless(lib, dt):
    nd = _nd()
    K = 1 << 18
    ext = -128 if dt == np.int8 else 255
    a = np.full((256, K), ext, dtype=dt)
    b = np.full((K, 256), ext, dtype=dt)
    a[0, :7] = 3
    got = nd.matmul(nd.asarray(a), nd.asarray(b)).get()              # |sum| = 2**32 and more: wraps in int32
    exp = (a.astype(np.int64).sum(axis=1)[:, None] * np.full((1, 256), int(ext), dtype=np.int64)).astype(dt)   # b is constant
    assert np.array_equal(got, exp)
    small = nd.matmul(nd.asarray(a[:64]), nd.asarray(b[:, :64])).get()   # few outputs, long k: the long-k route
    assert np.array_equal(small, exp[:64, :64])


# ---- float16: the bound, NumPy's specials, determinism ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,K,N", F16_SHAPES)
def test_float16_products_within_bound(lib, M, K, N):
    nd = _nd()
    rng = np.random.default_rng(M + 5 * K + 7 * N)
    a = rng.standard_normal((M, K)).astype(np.float16)
    b = rng.standard_normal((K, N)).astype(np.float16)
    got = nd.matmul(nd.asarray(a), nd.asarray(b)).get()
    assert got.dtype == np.float16
    ok, nbad = _f16_bound_ok(got, a, b)
    assert ok, nbad


@gpu
@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("M,K,N", [(512, 256, 384), (300, 160, 200), (144, 256, 208), (272, 160, 336), (1024, 1024, 1024)])
def test_float16_layouts_within_bound(lib, ta, tb, M, K, N):
    nd = _nd()
    rng = np.random.default_rng(3)
    a = rng.standard_normal((M, K)).astype(np.float16)
    b = rng.standard_normal((K, N)).astype(np.float16)
    got = nd.matmul(_layout(a, ta), _layout(b, tb)).get()
    ok, nbad = _f16_bound_ok(got, a, b)
    assert ok, (ta, tb, nbad)


@gpu
def test_float16_vectors_batches_views_out(lib):
    nd = _nd()
    rng = np.random.default_rng(9)
    v, w = rng.standard_normal(4096).astype(np.float16), rng.standard_normal(4096).astype(np.float16)
    ok, _ = _f16_bound_ok(np.asarray(nd.dot(nd.asarray(v), nd.asarray(w)).get())[None, None], v[None], w[:, None])
    assert ok
    m = rng.standard_normal((4096, 300)).astype(np.float16)
    assert _f16_bound_ok(nd.matmul(nd.asarray(v), nd.asarray(m)).get()[None], v[None], m)[0]
    a, b = rng.standard_normal((16, 256, 256)).astype(np.float16), rng.standard_normal((16, 256, 256)).astype(np.float16)
    assert _f16_bound_ok(nd.matmul(nd.asarray(a), nd.asarray(b)).get(), a, b)[0]
    a, b = rng.standard_normal((4, 1, 128, 64)).astype(np.float16), rng.standard_normal((3, 64, 96)).astype(np.float16)
    assert _f16_bound_ok(nd.matmul(nd.asarray(a), nd.asarray(b)).get(), a, b)[0]
    big = rng.standard_normal((513, 517)).astype(np.float16)
    da = nd.asarray(big)
    assert _f16_bound_ok(nd.matmul(da[1:, 1:], da[1:, 1:].T).get(), big[1:, 1:], big[1:, 1:].T)[0]
    t = rng.standard_normal((6, 40, 48)).astype(np.float16)
    u = rng.standard_normal((48, 6, 32)).astype(np.float16)
    got = nd.tensordot(nd.asarray(t), nd.asarray(u), axes=([0, 2], [1, 0])).get()
    a2 = np.transpose(t, (1, 0, 2)).reshape(40, 6 * 48)
    b2 = np.transpose(u, (1, 0, 2)).reshape(6 * 48, 32)
    assert got.dtype == np.float16 and _f16_bound_ok(got, a2, b2)[0]
    a, b = rng.standard_normal((256, 512)).astype(np.float16), rng.standard_normal((512, 256)).astype(np.float16)
    out = nd.zeros((256, 256), dtype=np.float16)
    assert nd.matmul(nd.asarray(a), nd.asarray(b), out=out) is out and _f16_bound_ok(out.get(), a, b)[0]
    x = nd.asarray(a[:, :256].copy())
    x @= nd.asarray(b[:256])
    assert _f16_bound_ok(x.get(), a[:, :256], b[:256])[0]


@gpu
@pytest.mark.parametrize("M,K,N", [(256, 256, 256), (7, 9, 5)])
def test_float16_specials_match_numpy(lib, M, K, N):
    nd = _nd()
    rng = np.random.default_rng(1)
    a = rng.standard_normal((M, K)).astype(np.float16)
    b = rng.standard_normal((K, N)).astype(np.float16)
    a[0, 0] = np.nan
    a[1, :] = 300.0                      # rows of 300 * 300 * K: past 65504 -> inf
    b[:, 1] = 300.0
    a[2, 3] = np.inf
    b[3, :] = 0.0                        # inf * 0 -> NaN
    a[3, 4] = -np.inf
    a[4, :] = np.float16(6e-8)           # subnormal inputs
    b[:, 2] = np.float16(-6e-8)
    with np.errstate(all="ignore"):
        exp = np.matmul(a, b)
    got = nd.matmul(nd.asarray(a), nd.asarray(b)).get()
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    assert np.array_equal(np.isposinf(got), np.isposinf(exp)) and np.array_equal(np.isneginf(got), np.isneginf(exp))
    with np.errstate(all="ignore"):
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        exact, mag = a64 @ b64, np.abs(a64) @ np.abs(b64)
        fin = np.isfinite(exp) & np.isfinite(exact)
        bound = np.spacing(np.abs(exact[fin]).astype(np.float16)).astype(np.float64) / 2 + K * 2.0 ** -23 * mag[fin]
    assert np.all(np.abs(got[fin].astype(np.float64) - exact[fin]) <= bound)


@gpu
def test_float16_against_numpy_loop(lib, capsys):
    """The fraction of elements that differ from NumPy's own float16 loop (a sequential float32 sum); both within the bound."""
    nd = _nd()
    rng = np.random.default_rng(2)
    a = rng.standard_normal((256, 512)).astype(np.float16)
    b = rng.standard_normal((512, 256)).astype(np.float16)
    exp = np.matmul(a, b)
    got = nd.matmul(nd.asarray(a), nd.asarray(b)).get()
    diff = got != exp
    with capsys.disabled():
        print(f"\nfloat16 256x512x256: {diff.mean():.4%} of elements differ from NumPy's loop")
    assert diff.mean() < 0.01 and _f16_bound_ok(got, a, b)[0]


@gpu
def test_float16_is_deterministic(lib):
    nd = _nd()
    rng = np.random.default_rng(4)
    a = nd.asarray(rng.standard_normal((4096, 4096)).astype(np.float16))
    b = nd.asarray(rng.standard_normal((4096, 4096)).astype(np.float16))
    r1 = nd.matmul(a, b).get()
    r2 = nd.matmul(a, b).get()
    assert np.array_equal(r1.view(np.uint16), r2.view(np.uint16))


# ---- autodiff in float16 ---------------------------------------------------------------------------------------------------------
def _mlp(md):
    rng = np.random.default_rng(17)
    x = md.Tensor(rng.standard_normal((64, 64)).astype(np.float16))
    W1 = md.Tensor((rng.standard_normal((64, 128)) * 0.2).astype(np.float16), allow_grad=True)
    b1 = md.Tensor((rng.standard_normal(128) * 0.1).astype(np.float16), allow_grad=True)
    W2 = md.Tensor((rng.standard_normal((128, 32)) * 0.2).astype(np.float16), allow_grad=True)
    z = x @ W1 + b1
    h = md.where(z > 0, z, 0)
    loss = md.sum(h @ W2)
    loss.backward()
    return [loss] + [p.grad for p in (W1, b1, W2)]


@gpu
def test_float16_mlp_forward_backward(lib):
    sys.path.insert(0, HERE)
    from golden_util import rel_err
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    from oracle.numpy_table import NumpyOracleTable
    got = _mlp(build_engine(HipBackendTable, "dev"))
    exp = _mlp(build_engine(NumpyOracleTable, "np"))
    for g, e in zip(got, exp):
        g, e = np.asarray(g.as_numpy()), np.asarray(e.as_numpy())
        assert g.dtype == e.dtype == np.float16 and g.shape == e.shape
        assert rel_err(g, e) <= 4e-3
