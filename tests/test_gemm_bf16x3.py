"""float32 products as six bfloat16 products of pre-split planes (csrc/gemm_bf16x3.hip, md_bf16x3.h; planned by gemm.hip).

CPU: the split itself, compiled into a stand-alone host program. GPU: the product kernel forced onto every eligible shape
(option gemm_bf16x3 = 2) at the smallest shapes that exercise it — block tile 256 x 128, k-tile 32: one, two and three tiles along
m and n, one, two, three and five k-tiles (the prologue alone, odd and even buffer turns) — in all four operand layouts."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SPLIT_MAIN = r"""
#include <math.h>
#include <stdio.h>
#include "md_bf16x3.h"
static unsigned long long fails = 0, seen = 0;
static void check(uint32_t u) {
  const float x = md_bf16x3_float(u);
  uint32_t p[3];
  const bool special = md_bf16x3_split(x, &p[0], &p[1], &p[2]);
  ++seen;
  bool ok = !(p[0] & 0xFFFFu) && !(p[1] & 0xFFFFu) && !(p[2] & 0xFFFFu);
  const bool nonfinite = (u & 0x7F800000u) == 0x7F800000u;
  ok = ok && special == nonfinite;
  if (nonfinite) {
    const float q = md_bf16x3_float(p[0]);
    ok = ok && p[1] == 0 && p[2] == 0 && ((u & 0x007FFFFFu) ? q != q : q == x);
  } else {
    const float s = (md_bf16x3_float(p[0]) + md_bf16x3_float(p[1])) + md_bf16x3_float(p[2]);
    if (fabsf(x) >= ldexpf(1.0f, -102)) ok = ok && s == x;   /* every plane a normal number: exact */
    else ok = ok && fabs((double)s - (double)x) < ldexp(1.0, -133);   /* a subnormal tail under bfloat16's smallest step is dropped */
    if (x == 0.0f) ok = ok && p[0] == u && p[1] == 0 && p[2] == 0;
  }
  if (!ok && fails++ < 10) printf("bad %08x -> %08x %08x %08x\n", u, p[0], p[1], p[2]);
}
int main(void) {
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < (1 << 22); ++i) {   /* 2^22 random bit patterns (xorshift64) */
    s ^= s << 13; s ^= s >> 7; s ^= s << 17;
    check((uint32_t)(s >> 16));
  }
  for (uint32_t e = 0; e < 256; ++e)      /* the edges of every binade, both signs (e = 0: zeros and subnormals, 255: inf and NaNs) */
    for (uint32_t sign = 0; sign < 2; ++sign) {
      const uint32_t m[] = {0u, 1u, 2u, 0xFFFFu, 0x10000u, 0x10001u, 0x7FFFu, 0x8000u, 0x3FFFFFu, 0x400000u, 0x7F0000u, 0x7FFFFEu, 0x7FFFFFu};
      for (unsigned j = 0; j < sizeof m / sizeof m[0]; ++j) check((sign << 31) | (e << 23) | m[j]);
    }
  const uint32_t named[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F800001u, 0xFFC00001u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                            0x00000001u, 0x807FFFFFu, 0x00800000u};   /* +-0, +-inf, NaNs, +-FLT_MAX, subnormals, FLT_MIN */
  for (unsigned j = 0; j < sizeof named / sizeof named[0]; ++j) check(named[j]);
  printf("checked %llu failed %llu\n", seen, fails);
  return fails != 0;
}
"""


def test_split_is_exact_on_the_host(tmp_path):
    """md_bf16x3_split in a stand-alone program built with the host compiler: low halves clear, the planes sum exactly to x
    wherever all three are normal numbers (|x| >= 2^-102; below, within bfloat16's smallest step 2^-133), specials give (x, 0, 0)."""
    cxx = shutil.which("gcc")   # the host compiler of csrc/Makefile (the program needs the C library only)
    assert cxx, "no host compiler"
    src = tmp_path / "split_main.cpp"
    src.write_text(_SPLIT_MAIN)
    exe = tmp_path / "split_main"
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "minidiff_amd", "csrc"), "-o", str(exe), str(src), "-lm"])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout
    assert "failed 0" in run.stdout and "checked 42" in run.stdout, run.stdout   # 2^22 + 256 * 2 * 13 + 12 = 4 200 972


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
TM, TN, TK = 256, 128, 32
LAYOUTS = ("NN", "NT", "TN", "TT")
SHAPES = [(m * TM, k * TK, n * TN) for m in (1, 2, 3) for n in (1, 2, 3) for k in (1, 2, 3, 5)]


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _runs(lib):
    v = C.c_int64()
    lib.debug_get_option(b"gemm_bf16x3_runs", C.byref(v))
    return v.value


def _operands(nd, A, B, lay):
    """device views of A (M x K) and B (K x N) in the layout: 'T' = stored transposed, passed as the transposed view"""
    a = nd.asarray(np.ascontiguousarray(A.T)).T if lay[0] == "T" else nd.asarray(A)
    b = nd.asarray(np.ascontiguousarray(B.T)).T if lay[1] == "T" else nd.asarray(B)
    return a, b


@pytest.fixture
def eager():
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(False)
    yield nd
    nd.set_lazy(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_integers_identity_and_randn_on_every_shape(lib, on_gpu, mdopt, eager, lay):
    """Integer operands in -2000 .. 2000 (two planes) against small ones, sums below 2^24: EQUAL to NumPy. Identity on either side:
    exact. randn: within 2e-6 (max-norm, as test_direct_to_lds_gemm_random_aligned_shapes) of float64. One launch of the product
    kernel per call."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(31)
    for (M, K, N) in SHAPES:
        small = (1 << 24) // (2000 * K)
        for big_a in (True, False):
            A = rng.integers(-2000, 2001, (M, K)) if big_a else rng.integers(-small, small + 1, (M, K))
            B = rng.integers(-small, small + 1, (K, N)) if big_a else rng.integers(-2000, 2001, (K, N))
            a, b = _operands(nd, A.astype(np.float32), B.astype(np.float32), lay)
            r0 = _runs(lib)
            got = nd.matmul(a, b).get()
            assert _runs(lib) == r0 + 1, (lay, M, K, N)
            assert np.array_equal(got, (A @ B).astype(np.float64)), (lay, M, K, N, big_a)
        fa, fb = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
        a, b = _operands(nd, fa, fb, lay)
        got = nd.matmul(a, b).get()
        assert _rel(got, fa.astype(np.float64) @ fb) < 2e-6, (lay, M, K, N)
        assert np.array_equal(nd.matmul(a, b).get(), got), (lay, M, K, N)   # two calls: bit-equal
    # identity on either side (square shapes: K = M or K = N is a multiple of the k-tile)
    for n in (256, 768):
        x = rng.standard_normal((n, n), dtype=np.float32) * np.exp2(rng.integers(-20, 20, (n, n))).astype(np.float32)
        eye = np.eye(n, dtype=np.float32)
        for A, B in ((eye, x), (x, eye)):
            a, b = _operands(nd, A, B, lay)
            r0 = _runs(lib)
            assert np.array_equal(nd.matmul(a, b).get(), x), (lay, n)
            assert _runs(lib) == r0 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_row_panels_are_bit_equal_to_the_whole_product(lib, on_gpu, mdopt, eager, lay):
    """The first tile-row panel of A, and a panel written through out= into a row-panel view of a larger array, carry the bits of
    the same rows of the whole product."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(32)
    M, K, N = 768, 160, 384
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    whole = nd.matmul(a, b).get()
    r0 = _runs(lib)
    assert np.array_equal(nd.matmul(a[:TM], b).get(), whole[:TM])
    bucket = nd.asarray(np.zeros((M, N), np.float32))
    nd.matmul(a[TM:3 * TM], b, out=bucket[TM:3 * TM])
    assert _runs(lib) == r0 + 2
    got = bucket.get()
    assert np.array_equal(got[TM:], whole[TM:]) and not got[:TM].any()


@pytest.mark.gpu
def test_shapes_the_kernel_does_not_take_keep_the_fp32_route(lib, on_gpu, mdopt, eager):
    """A ragged shape, a batch, a misaligned view and option 0: no launch of the product kernel, and the bits of option 0."""
    assert on_gpu
    nd = eager
    rng = np.random.default_rng(33)
    M, K, N = 512, 96, 256

    def randn(*shape):
        return rng.standard_normal(shape, dtype=np.float32)

    big = nd.asarray(randn(M, K + 4))
    cases = {
        "ragged m": (nd.asarray(randn(M + 4, K)), nd.asarray(randn(K, N))),
        "ragged k": (nd.asarray(randn(M, K + 4)), nd.asarray(randn(K + 4, N))),
        "batch": (nd.asarray(randn(2, M, K)), nd.asarray(randn(2, K, N))),
        "misaligned view": (big[:, 1:K + 1], nd.asarray(randn(K, N))),
        # few 64 x 64 tiles under K >= 1024: the fp32 plan is a split-K launch and a sum, which cannot stand in behind the product
        # (plan_bf16x3 takes plain launches only) — the product stays fp32. Above option 1's floors no shape is planned that way.
        "split-k fp32 plan": (nd.asarray(randn(512, 1024)), nd.asarray(randn(1024, 512))),
        "eligible": (nd.asarray(randn(M, K)), nd.asarray(randn(K, N))),
    }
    for name, (a, b) in cases.items():
        mdopt("gemm_bf16x3", 0)
        r0 = _runs(lib)
        ref = nd.matmul(a, b).get()
        assert _runs(lib) == r0, name
        mdopt("gemm_bf16x3", 2)
        got = nd.matmul(a, b).get()
        if name == "eligible":
            assert _runs(lib) == r0 + 1
            assert _rel(got, ref) < 2e-6
        else:
            assert _runs(lib) == r0, name
            assert np.array_equal(got, ref), name
    # the default (option 1) keeps small products off the route whatever their structure
    mdopt("gemm_bf16x3", 1)
    r0 = _runs(lib)
    nd.matmul(*cases["eligible"]).get()
    assert _runs(lib) == r0


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_non_finite_operands_give_the_fma_chain_result(lib, on_gpu, mdopt, eager, lay):
    """An inf, a NaN, and an inf opposite an exact zero (whose lower planes would give inf x 0): the split passes raise the flag, the
    fp32 kernel behind the product runs instead — the NaN / inf pattern and the finite values of option 0, bit for bit."""
    assert on_gpu
    nd = eager
    rng = np.random.default_rng(34)
    M, K, N = 512, 96, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    plant = {
        "inf in a": ((3, 5, np.inf), None),
        "nan in b": (None, (7, 9, np.nan)),
        "inf opposite zero": ((300, 40, -np.inf), (40, 200, 0.0)),
        "inf opposite one": ((300, 40, -np.inf), (40, 200, 1.0)),   # (1.0 = (1, 0, 0): inf x its zero planes would be NaN)
        "both": ((511, 95, np.inf), (0, 0, np.nan)),
    }
    for name, (pa, pb) in plant.items():
        A2, B2 = A.copy(), B.copy()
        if pa: A2[pa[0], pa[1]] = pa[2]
        if pb: B2[pb[0], pb[1]] = pb[2]
        a, b = _operands(nd, A2, B2, lay)
        mdopt("gemm_bf16x3", 0)
        ref = nd.matmul(a, b).get()
        mdopt("gemm_bf16x3", 2)
        r0 = _runs(lib)
        got = nd.matmul(a, b).get()
        assert _runs(lib) == r0 + 1, name
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name
        assert np.array_equal(got.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)]), name
        assert not np.isfinite(ref).all(), name
    # and the flag does not stick: the next finite product runs on the planes
    a, b = _operands(nd, A, B, lay)
    assert _rel(nd.matmul(a, b).get(), A.astype(np.float64) @ B) < 2e-6


@pytest.mark.gpu
def test_all_positive_operands_at_depth_keep_the_fp32_bound(lib, on_gpu, mdopt, eager):
    """Same-sign operands at K = 4096: the matrix instruction's accumulation truncates, so one accumulator over all of K comes out
    low, linearly in K (8.6e-6 of the largest element at this depth); the kernel starts a fresh accumulator per k-tile and adds the
    k-tiles with round-to-nearest adds. Both routes are held to the same bounds against float64: 2e-6 norm-wise (the randn bound of
    this file; the fma chain measures 1e-6 here), and a mean error under 12 * 2^-23 of the largest element — the worst case of the
    12 truncations of one k-tile, which no K adds to. 512 x 4096 x 2304: the smallest full grid the k ranges do not take."""
    assert on_gpu
    nd = eager
    rng = np.random.default_rng(36)
    M, K, N = 512, 4096, 2304
    A, B = np.abs(rng.standard_normal((M, K), dtype=np.float32)), np.abs(rng.standard_normal((K, N), dtype=np.float32))
    ref = A.astype(np.float64) @ B
    a, b = nd.asarray(A), nd.asarray(B)
    for opt in (0, 2):
        mdopt("gemm_bf16x3", opt)
        r0 = _runs(lib)
        got = nd.matmul(a, b).get().astype(np.float64)
        assert _runs(lib) - r0 == (1 if opt else 0)
        fro = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        bias = float(np.mean(got - ref) / np.abs(ref).max())
        print(f"option {opt}: norm-wise {fro:.3e}, mean error / max {bias:+.3e}")
        assert fro < 2e-6, (opt, fro)
        assert abs(bias) < 12 * 2.0 ** -23, (opt, bias)


@pytest.mark.gpu
def test_default_option_routes_products_above_the_floors(lib, on_gpu, eager):
    """Option 1, untouched: a 1024 x 4096 x 4096 product and its 512-row panel both launch the product kernel once (no split-K or
    peeled fp32 plan above the floors keeps them off it) and agree bit for bit; 1024 x 4096 x 2048 (N under the floor) does not."""
    assert on_gpu
    nd = eager
    v = C.c_int64()
    lib.debug_get_option(b"gemm_bf16x3", C.byref(v))
    assert v.value == 1
    rng = np.random.default_rng(37)
    a, b = nd.asarray(rng.standard_normal((1024, 4096), dtype=np.float32)), nd.asarray(rng.standard_normal((4096, 4096), dtype=np.float32))
    r0 = _runs(lib)
    whole = nd.matmul(a, b).get()
    assert _runs(lib) == r0 + 1
    assert np.array_equal(nd.matmul(a[:512], b).get(), whole[:512])
    assert _runs(lib) == r0 + 2
    nd.matmul(a, b[:, :2048]).get()
    assert _runs(lib) == r0 + 2


@pytest.mark.gpu
def test_fused_epilogue_declines_and_lazy_relu_sum_stays_right(lib, on_gpu, mdopt):
    """On a shape whose plain product runs as bf16x3 the fused bias + relu + sum GEMM reports "not fused"; lazy
    sum(where(X @ W + b > 0, X @ W + b, 0)) then runs the plain product and the fused tail: right loss, and the mask of the plain
    product bit for bit."""
    assert on_gpu
    from minidiff_amd import ndarray as nd
    rng = np.random.default_rng(35)
    M, K, N = 512, 64, 256
    X = rng.integers(-3, 4, (M, K)).astype(np.float32)
    W = rng.integers(-3, 4, (K, N)).astype(np.float32)
    b = (rng.integers(-3, 4, N) + 0.5).astype(np.float32)     # (never exactly 0 after the add)
    zr = X.astype(np.float64) @ W + b
    prev = nd.set_lazy(True)
    try:
        for opt, fused in ((0, 1), (2, 0)):
            mdopt("gemm_bf16x3", opt)
            s0, r0 = nd.FUSION_STATS["gemm_epilogue"], _runs(lib)
            z = nd.add(nd.matmul(nd.asarray(X), nd.asarray(W)), nd.asarray(b))
            m = nd.greater(z, 0)
            loss = nd.sum(nd.where(m, z, 0))
            got = float(loss.get())
            assert nd.FUSION_STATS["gemm_epilogue"] - s0 == fused, opt
            assert _runs(lib) - r0 == 1 - fused, opt
            assert np.array_equal(m.get(), zr > 0), opt
            assert abs(got - np.where(zr > 0, zr, 0).sum()) <= 1e-6 * np.abs(zr).sum(), opt
        # randn: the mask is the plain product's own
        Xf, Wf, bf = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32), rng.standard_normal(N, dtype=np.float32)
        z = nd.add(nd.matmul(nd.asarray(Xf), nd.asarray(Wf)), nd.asarray(bf))
        m = nd.greater(z, 0)
        loss = nd.sum(nd.where(m, z, 0))
        got, mask = float(loss.get()), m.get()
        nd.set_lazy(False)
        plain = nd.matmul(nd.asarray(Xf), nd.asarray(Wf)).get() + bf
        assert np.array_equal(mask, plain > 0)
        assert abs(got - np.where(plain > 0, plain.astype(np.float64), 0).sum()) <= 1e-6 * np.abs(plain).sum()
    finally:
        nd.set_lazy(prev)
