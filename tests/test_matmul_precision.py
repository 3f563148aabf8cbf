"""The matmul precision switch: float32 products as three or one bfloat16 product (ndarray.set_matmul_precision, library option
gemm_products; csrc/md_bf16x3.h md_bf16x3_split_rn, csrc/gemm_bf16x3.hip k_gemm_bf16xp, planned by gemm.hip).

CPU: the option, the Python switch, the rounding split as a stand-alone host program, the sweep cache's key. GPU: the reduced kernels
forced onto every eligible shape (option gemm_bf16x3 = 2) at the shapes of tests/test_gemm_bf16x3.py — block tile 256 x 128, k-tile
32: one, two and three tiles along m and n, one, two, three and five k-tiles — in all four operand layouts.

The contract, entry-wise against the float64 product, with u8 = 2^-8 and mass = |a| @ |b|:
    medium  |err| <= (2 u8 + u8^2) mass + acc          (one rounded plane per operand)
    high    |err| <= (3 u8^2 + 2^-23) mass + acc       (two plane remainders and the dropped a2b2)
and acc = _acc(K, products) * mass, derived from the kernel as built (bx_mma<NP, NPROD> in gemm_bf16x3.hip): a k-tile of 32 k is two
k16 steps; each step issues `products` matrix instructions per output element (a1b1[, a1b2, a2b1]) that accumulate into ONE fresh
float32 accumulator, and the matrix instruction's accumulation truncates: 2 * products truncating accumulations per k-tile, each off
by at most 2^-23 of the accumulator's value, which the k-tile's share of mass bounds — summed over the k-tiles, 2 * products * 2^-23
* mass. The k-tile's sum is then added into the running sum with ONE round-to-nearest add (2^-24 of the running sum, which mass
bounds): K / 32 * 2^-24 * mass. First-order terms only; the products of these terms are below 2^-30 mass and the bounds are held
with the margins printed by the tests (the emulation stays within 0.18 of the medium and 0.07 of the high bound)."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8 = 2.0 ** -8
PRODUCTS = {"highest": 6, "high": 3, "medium": 1}
MODES = ("medium", "high")


def _acc(K, products):
    """the accumulation term per unit of mass: see the module docstring"""
    return 2 * products * 2.0 ** -23 + (K // 32) * 2.0 ** -24


def _bound(mode, mass, K):
    model = 2 * U8 + U8 * U8 if mode == "medium" else 3 * U8 * U8 + 2.0 ** -23
    return (model + _acc(K, PRODUCTS[mode])) * mass


def _rn(x):
    """round-to-nearest-even to bfloat16, as a float32 array (finite values that do not overflow)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def _planes(x):
    x = np.asarray(x, dtype=np.float32)
    p1 = _rn(x)
    return p1, _rn(x - p1)


def _emulated(A, B, mode):
    """the product of the emulated planes in float64: medium RN(A) @ RN(B); high A1 @ B1 + A1 @ B2 + A2 @ B1"""
    a1, a2 = (p.astype(np.float64) for p in _planes(A))
    b1, b2 = (p.astype(np.float64) for p in _planes(B))
    if mode == "medium":
        return a1 @ b1
    return a1 @ b1 + a1 @ b2 + a2 @ b1


def _get(lib, name):
    v = C.c_int64()
    lib.debug_get_option(name.encode(), C.byref(v))
    return v.value


def _runs(lib):
    return _get(lib, "gemm_bf16x3_runs")


@pytest.fixture
def precision():
    """the public setter, put back when the test ends"""
    from minidiff_amd import ndarray as nd
    before = nd.get_matmul_precision()
    yield nd.set_matmul_precision
    nd.set_matmul_precision(before)


@pytest.fixture
def eager():
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(False)
    yield nd
    nd.set_lazy(prev)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------
def test_option_gemm_products_is_in_the_shared_table(lib, mdopt):
    """settable and readable through the test hook on whichever build of the C-ABI is bound (the double ignores its value)"""
    assert _get(lib, "gemm_products") == 6
    for v in (3, 1, 6):
        mdopt("gemm_products", v)
        assert _get(lib, "gemm_products") == v


def test_python_switch_names_previous_value_and_errors(lib, precision):
    from minidiff_amd import ndarray as nd
    assert nd.get_matmul_precision() == "highest"
    assert precision("medium") == "highest" and nd.get_matmul_precision() == "medium" and _get(lib, "gemm_products") == 1
    assert precision("high") == "medium" and nd.get_matmul_precision() == "high" and _get(lib, "gemm_products") == 3
    for bad in ("low", "HIGH", "", 3, None):
        with pytest.raises(ValueError):
            nd.set_matmul_precision(bad)
        assert nd.get_matmul_precision() == "high" and _get(lib, "gemm_products") == 3
    assert precision("highest") == "high" and _get(lib, "gemm_products") == 6


def test_environment_variable_is_read_once_and_pushed_to_the_library(on_gpu):
    """MDHIP_MATMUL_PRECISION in a fresh child: the setting is there before any library is, and reaches the library when it is bound"""
    double = os.environ.get("MDHIP_HOST_DOUBLE") or os.path.join(ROOT, "oracle", "_build", "libmdhip_host.so")   # (as tests/conftest.py)
    child = ("import sys, ctypes as C\n"
             "from minidiff_amd import ndarray as nd, _capi\n"
             "assert _capi.current() is None\n"
             "print(nd.get_matmul_precision())\n"
             "lib = _capi.load() if sys.argv[1] == 'gpu' else _capi.use_library(sys.argv[1])\n"
             "v = C.c_int64(); lib.debug_get_option(b'gemm_products', C.byref(v)); print(v.value)\n")
    for name, products in (("high", 3), ("medium", 1), ("highest", 6), (None, 6)):
        env = {k: v for k, v in os.environ.items() if k != "MDHIP_MATMUL_PRECISION"}
        if name:
            env["MDHIP_MATMUL_PRECISION"] = name
        run = subprocess.run([sys.executable, "-c", child, "gpu" if on_gpu else double], cwd=ROOT, env=env, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr
        assert run.stdout.split() == [name or "highest", str(products)], run.stdout
    env = dict(os.environ, MDHIP_MATMUL_PRECISION="fastest")
    run = subprocess.run([sys.executable, "-c", "import minidiff_amd.ndarray"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert run.returncode != 0 and "ValueError" in run.stderr and "fastest" in run.stderr


def test_products_the_kernels_do_not_take_are_bit_equal_under_medium(lib, eager, precision):
    """64 x 48 x 40: under every floor and no whole tile — the fp32 route on the GPU; the double ignores the option altogether"""
    nd = eager
    rng = np.random.default_rng(50)
    A, B = rng.standard_normal((64, 48), dtype=np.float32), rng.standard_normal((48, 40), dtype=np.float32)
    a, b = nd.asarray(A), nd.asarray(B)
    ref = nd.matmul(a, b).get()
    precision("medium")
    r0 = _runs(lib)
    got = nd.matmul(a, b).get()
    assert _runs(lib) == r0
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


_SPLIT_RN_MAIN = r"""
#include <math.h>
#include <stdio.h>
#include "md_bf16x3.h"
static unsigned long long fails = 0, seen = 0;
/* round to nearest even on the integer halves, written independently of md_bf16x3_rn's add-and-mask */
static uint32_t rne(uint32_t u) {
  uint32_t keep = u >> 16;
  const uint32_t low = u & 0xFFFFu;
  if (low > 0x8000u || (low == 0x8000u && (keep & 1u))) ++keep;
  return keep << 16;
}
static void check(uint32_t u, int nplanes) {
  const float x = md_bf16x3_float(u);
  uint32_t p1 = 0xDEADBEEFu, p2 = 0xDEADBEEFu;
  const bool special = md_bf16x3_split_rn(x, nplanes, &p1, &p2);
  ++seen;
  bool ok = !(p1 & 0xFFFFu) && !(p2 & 0xFFFFu);
  const bool nonfinite = (u & 0x7F800000u) == 0x7F800000u;
  if (nonfinite) {
    const float q = md_bf16x3_float(p1);
    ok = ok && special && p2 == 0 && ((u & 0x007FFFFFu) ? q != q : q == x);
  } else {
    ok = ok && p1 == rne(u);
    const bool overflow = (rne(u) & 0x7F800000u) == 0x7F800000u;   /* |x| >= 0x7F7F8000 rounds up to inf */
    ok = ok && special == overflow;
    if (overflow) ok = ok && p2 == 0 && (u & 0x7FFFFFFFu) >= 0x7F7F8000u;
    else {
      const float a = md_bf16x3_float(p1), r = x - a;
      ok = ok && (double)r == (double)x - (double)a;               /* x - p1 is exact in float32 */
      if (fabsf(x) >= ldexpf(1.0f, -126)) ok = ok && fabs((double)r) <= ldexp(fabs((double)x), -8);   /* normal x: at most half a step of an 8-bit significand */
      if (nplanes == 1) ok = ok && p2 == 0;
      else {
        ok = ok && p2 == rne(md_bf16x3_bits(r));
        const double rest = fabs((double)r - (double)md_bf16x3_float(p2));
        /* 2^-16 |x| down to |x| = 2^-118; below, half of bfloat16's smallest step 2^-133, which no 16-bit plane does better */
        if (fabsf(x) >= ldexpf(1.0f, -118)) ok = ok && rest <= ldexp(fabs((double)x), -16);
        else ok = ok && rest <= ldexp(1.0, -134);
      }
      if (x == 0.0f) ok = ok && p1 == u && p2 == 0;
    }
  }
  if (!ok && fails++ < 10) printf("bad %08x (%d planes) -> %08x %08x %d\n", u, nplanes, p1, p2, (int)special);
}
int main(void) {
  for (int nplanes = 1; nplanes <= 2; ++nplanes) {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < (1 << 22); ++i) {   /* 2^22 random bit patterns (xorshift64) */
      s ^= s << 13; s ^= s >> 7; s ^= s << 17;
      check((uint32_t)(s >> 16), nplanes);
    }
    for (uint32_t e = 0; e < 256; ++e)      /* the edges of every binade, both signs: ties to even and to odd, one off a tie, the last pattern */
      for (uint32_t sign = 0; sign < 2; ++sign) {
        const uint32_t m[] = {0u, 1u, 2u, 0xFFFFu, 0x10000u, 0x10001u, 0x7FFFu, 0x8000u, 0x8001u, 0x18000u, 0x17FFFu, 0x3FFFFFu, 0x400000u,
                              0x7F0000u, 0x7F7FFFu, 0x7F8000u, 0x7FFFFEu, 0x7FFFFFu};
        for (unsigned j = 0; j < sizeof m / sizeof m[0]; ++j) check((sign << 31) | (e << 23) | m[j], nplanes);
      }
    const uint32_t named[] = {0x00000000u, 0x80000000u, 0x7F800000u, 0xFF800000u, 0x7FC00000u, 0x7F800001u, 0xFFC00001u, 0x7F7FFFFFu, 0xFF7FFFFFu,
                              0x7F7F7FFFu, 0x7F7F8000u, 0xFF7F8000u, 0x00000001u, 0x807FFFFFu, 0x00800000u};
    /* +-0, +-inf, NaNs, +-FLT_MAX, the last value that rounds to a finite plane and the first that rounds to inf, subnormals, FLT_MIN */
    for (unsigned j = 0; j < sizeof named / sizeof named[0]; ++j) check(named[j], nplanes);
  }
  printf("checked %llu failed %llu\n", seen, fails);
  return fails != 0;
}
"""


def test_rounding_split_on_the_host(tmp_path):
    """md_bf16x3_split_rn for one and two planes in a stand-alone program built with the host compiler: low halves clear, p1 the
    round-to-nearest-even of an independent integer rounding, x - p1 exact, |x - p1 - p2| <= 2^-16 |x| for |x| >= 2^-118 (below, the
    normal numbers down to 2^-126 included, half of bfloat16's smallest step 2^-133 is all a 16-bit plane can give), `true` exactly for inf, NaN and what rounds up to inf."""
    cxx = shutil.which("gcc")
    assert cxx, "no host compiler"
    src = tmp_path / "split_rn_main.cpp"
    src.write_text(_SPLIT_RN_MAIN)
    exe = tmp_path / "split_rn_main"
    subprocess.check_call([cxx, "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "minidiff_amd", "csrc"), "-o", str(exe), str(src), "-lm"])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout
    assert "failed 0" in run.stdout and "checked 8407070 " in run.stdout, run.stdout   # 2 * (2^22 + 256 * 2 * 18 + 15)


def test_sweep_cache_does_not_replay_across_a_change_of_precision(engines, precision, monkeypatch):
    """The replay bookkeeping with a stand-in for the captured graph (the double cannot capture): eager, captured, replayed under
    "highest"; the first call under "medium" runs the sweep in Python again and captures a graph of its own; back under "highest"
    the call runs in Python once more and then the graph recorded under "highest" is the one replayed."""
    from minidiff_amd import graph
    made = []

    class Recorded:
        def __init__(self, step, warmup=0):
            from minidiff_amd import ndarray as nd
            self.precision, self.replays = nd.get_matmul_precision(), 0
            self.outputs = step()
            made.append(self)

        def replay(self):
            from minidiff_amd import ndarray as nd
            assert nd.get_matmul_precision() == self.precision, "a graph recorded under another precision was replayed"
            self.replays += 1
            return self.outputs

        def close(self):
            pass

    monkeypatch.setattr(graph, "CapturedSweep", Recorded)
    monkeypatch.setattr(graph.SweepCache, "_lib_sync", staticmethod(lambda: None))
    md = engines[0]
    x = md.Tensor(np.arange(12.0, dtype=np.float32).reshape(3, 4) / 8, allow_grad=True)
    w = md.Tensor(np.arange(8.0, dtype=np.float32).reshape(4, 2) / 4, allow_grad=True)

    def step():
        x.grad = None
        w.grad = None
        md.sum(x @ w).backward()
        return {"gx": x.grad}

    with graph.SweepCache(md, validate_every=0) as cache:
        for _ in range(4):
            cache.run(step)
        assert cache.stats == {"eager": 1, "captured": 1, "replayed": 2, "invalidated": 0, "uncapturable": 0}
        precision("medium")
        cache.run(step)
        assert cache.stats["replayed"] == 2 and cache.stats["eager"] == 2
        cache.run(step)
        cache.run(step)
        assert cache.stats["captured"] == 2 and cache.stats["replayed"] == 3
        assert [r.precision for r in made] == ["highest", "medium"] and made[1].replays == 2
        precision("highest")
        cache.run(step)
        assert cache.stats["eager"] == 3 and cache.stats["replayed"] == 3
        cache.run(step)
        assert cache.stats["replayed"] == 4 and made[0].replays == 4 and len(made) == 2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
TM, TN, TK = 256, 128, 32
LAYOUTS = ("NN", "NT", "TN", "TT")
SHAPES = [(m * TM, k * TK, n * TN) for m in (1, 2, 3) for n in (1, 2, 3) for k in (1, 2, 3, 5)]


def _operands(nd, A, B, lay):
    """device views of A (M x K) and B (K x N) in the layout: 'T' = stored transposed, passed as the transposed view"""
    a = nd.asarray(np.ascontiguousarray(A.T)).T if lay[0] == "T" else nd.asarray(A)
    b = nd.asarray(np.ascontiguousarray(B.T)).T if lay[1] == "T" else nd.asarray(B)
    return a, b


def _sparse_big(rng, K, N):
    """K x N integers in -2000 .. 2000, three non-zeros per column at random k: against a dense operand of the same range every sum of
    the plane products stays below 3 * 2000 * 2008 < 2^24"""
    B = np.zeros((K, N), dtype=np.int64)
    for _ in range(3):
        B[rng.integers(0, K, N), np.arange(N)] = rng.integers(-2000, 2001, N)
    return B


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_integers_identity_and_bf16_exact_operands_are_exact(lib, on_gpu, mdopt, eager, precision, mode, lay):
    """Integer operands in -2000 .. 2000 (two planes in about two thirds of the elements, never a third) on both sides, sums below 2^24
    — a dense operand against one with three non-zeros per column or row, and against a dense one of small integers: EQUAL to the
    product of the emulated planes, which is not A @ B. Operands that are bfloat16 numbers: NumPy's product. Identity on either
    side: RN(x) under medium, RN(x) + RN(x - RN(x)) under high. One counted launch per call."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    precision(mode)
    rng = np.random.default_rng(51)
    differs = 0
    for (M, K, N) in SHAPES:
        small = (1 << 23) // (2000 * K)
        cases = (
            (rng.integers(-2000, 2001, (M, K)), _sparse_big(rng, K, N)),
            (_sparse_big(rng, K, M).T, rng.integers(-2000, 2001, (K, N))),
            (rng.integers(-2000, 2001, (M, K)), rng.integers(-small, small + 1, (K, N))),
            (rng.integers(-small, small + 1, (M, K)), rng.integers(-2000, 2001, (K, N))),
        )
        for A, B in cases:
            a, b = _operands(nd, A.astype(np.float32), B.astype(np.float32), lay)
            r0 = _runs(lib)
            got = nd.matmul(a, b).get()
            assert _runs(lib) == r0 + 1, (lay, M, K, N)
            want = _emulated(A, B, mode)
            assert np.array_equal(got, want), (lay, M, K, N)
            differs += not np.array_equal(want, (A @ B).astype(np.float64))
        # bfloat16 numbers: integers of at most 8 bits times a power of two
        A = rng.integers(-255, 256, (M, K)) * 2.0 ** rng.integers(-3, 4)
        B = rng.integers(-255, 256, (K, N)) * 2.0 ** rng.integers(-3, 4)
        a, b = _operands(nd, A.astype(np.float32), B.astype(np.float32), lay)
        assert np.array_equal(nd.matmul(a, b).get(), A @ B), (lay, M, K, N)
    assert differs >= 2 * len(SHAPES), "the cases must tell the reduced products from A @ B"
    for n in (256, 768):
        x = rng.standard_normal((n, n), dtype=np.float32) * np.exp2(rng.integers(-20, 20, (n, n))).astype(np.float32)
        p1, p2 = _planes(x)
        want = p1 if mode == "medium" else p1 + p2   # (exact in float32: at most 17 significant bits)
        eye = np.eye(n, dtype=np.float32)
        for A, B in ((eye, x), (x, eye)):
            a, b = _operands(nd, A, B, lay)
            r0 = _runs(lib)
            assert np.array_equal(nd.matmul(a, b).get(), want), (lay, n)
            assert _runs(lib) == r0 + 1


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_randn_and_positive_operands_stay_within_the_contract(lib, on_gpu, mdopt, eager, precision, mode, lay):
    """entry-wise |got - float64| <= _bound (module docstring) at every shape, and two calls agree bit for bit"""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    precision(mode)
    rng = np.random.default_rng(52)
    worst = 0.0
    for (M, K, N) in SHAPES:
        for positive in (False, True):
            A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
            if positive:
                A, B = np.abs(A), np.abs(B)
            a, b = _operands(nd, A, B, lay)
            r0 = _runs(lib)
            got = nd.matmul(a, b).get()
            assert _runs(lib) == r0 + 1
            A64, B64 = A.astype(np.float64), B.astype(np.float64)
            ratio = float((np.abs(got - A64 @ B64) / _bound(mode, np.abs(A64) @ np.abs(B64), K)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (lay, M, K, N, positive, ratio)
            assert np.array_equal(nd.matmul(a, b).get().view(np.uint32), got.view(np.uint32)), (lay, M, K, N)
    print(f"{mode} {lay}: worst |err| / bound {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_positive_operands_at_depth_stay_within_the_contract(lib, on_gpu, mdopt, eager, precision, mode):
    """256 x 4096 x 128, all-positive: the case in which one truncating accumulator over all of K comes out low in proportion to K
    (-1.5e-5 at K = 8192: as large as the three-product form's own error). A fresh accumulator per k-tile keeps it out."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    mdopt("gemm_splitk", 0)   # (few tiles under a long k: the fp32 stand-in must be one plain launch for the plan to take the product)
    precision(mode)
    rng = np.random.default_rng(53)
    M, K, N = 256, 4096, 128
    A, B = np.abs(rng.standard_normal((M, K), dtype=np.float32)), np.abs(rng.standard_normal((K, N), dtype=np.float32))
    ref = A.astype(np.float64) @ B
    r0 = _runs(lib)
    got = nd.matmul(nd.asarray(A), nd.asarray(B)).get()
    assert _runs(lib) == r0 + 1
    ratio = float((np.abs(got - ref) / _bound(mode, ref, K)).max())   # (mass = the product itself)
    print(f"{mode}: worst |err| / bound {ratio:.3f}, norm-wise {np.linalg.norm(got - ref) / np.linalg.norm(ref):.3e}, "
          f"mean error / max {np.mean(got - ref) / ref.max():+.3e}")
    assert ratio <= 1.0, ratio


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_non_finite_operands_give_the_fma_chain_result(lib, on_gpu, mdopt, eager, precision, mode, lay):
    """An inf, a NaN, an inf opposite a zero, and FINITE elements that round up to inf as a plane (FLT_MAX, 0x7F7F8000): the split
    passes raise the flag and the fp32 kernel behind the product runs instead — the pattern and the values of option 0, bit for bit."""
    assert on_gpu
    nd = eager
    rng = np.random.default_rng(54)
    M, K, N = 512, 96, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    fmax = np.float32(np.finfo(np.float32).max)
    edge = np.array([0x7F7F8000], dtype=np.uint32).view(np.float32)[0]
    plant = {
        "inf in a": ((3, 5, np.inf), None, False),
        "nan in b": (None, (7, 9, np.nan), False),
        "inf opposite zero": ((300, 40, -np.inf), (40, 200, 0.0), False),
        "both": ((511, 95, np.inf), (0, 0, np.nan), False),
        "FLT_MAX in a": ((2, 3, fmax), None, True),
        "-FLT_MAX in b": (None, (95, 255, -fmax), True),
        "first value that rounds to inf": ((255, 31, edge), None, True),
    }
    for name, (pa, pb, finite) in plant.items():
        A2, B2 = A.copy(), B.copy()
        if pa: A2[pa[0], pa[1]] = pa[2]
        if pb: B2[pb[0], pb[1]] = pb[2]
        a, b = _operands(nd, A2, B2, lay)
        mdopt("gemm_bf16x3", 0)
        ref = nd.matmul(a, b).get()
        mdopt("gemm_bf16x3", 2)
        precision(mode)
        r0 = _runs(lib)
        got = nd.matmul(a, b).get()
        assert _runs(lib) == r0 + 1, name
        assert np.array_equal(np.isnan(got), np.isnan(ref)), name
        assert np.array_equal(got.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)]), name
        assert finite or not np.isfinite(ref).all(), name
    # the last value that rounds to a finite plane runs on the planes, and the flag does not stick
    A2 = A.copy()
    A2[1, 1] = np.array([0x7F7F7FFF], dtype=np.uint32).view(np.float32)[0]
    A2[1, 2:] = 0
    A2[1, 0] = 0
    a, b = _operands(nd, A2, B * np.float32(2.0 ** -20), lay)
    got = nd.matmul(a, b).get()
    want = _emulated(A2, B * np.float32(2.0 ** -20), mode)
    assert np.isfinite(got).all() and np.allclose(got[1], want[1], rtol=2e-6, atol=0)   # (one term per element: six truncations at most)
    a, b = _operands(nd, A, B, lay)
    A64 = A.astype(np.float64)
    assert (np.abs(nd.matmul(a, b).get() - A64 @ B) <= _bound(mode, np.abs(A64) @ np.abs(B), K)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_row_panels_are_bit_equal_to_the_whole_product(lib, on_gpu, mdopt, eager, precision, mode, lay):
    """the three 256-row panels of a 768-row product, one of them written through out= into a panel of a larger array"""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    precision(mode)
    rng = np.random.default_rng(55)
    M, K, N = 768, 160, 384
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    whole = nd.matmul(a, b).get()
    r0 = _runs(lib)
    for i in range(2):
        assert np.array_equal(nd.matmul(a[i * TM:(i + 1) * TM], b).get().view(np.uint32), whole[i * TM:(i + 1) * TM].view(np.uint32))
    bucket = nd.asarray(np.zeros((M, N), np.float32))
    nd.matmul(a[2 * TM:], b, out=bucket[2 * TM:])
    assert _runs(lib) == r0 + 3
    got = bucket.get()
    assert np.array_equal(got[2 * TM:].view(np.uint32), whole[2 * TM:].view(np.uint32)) and not got[:2 * TM].any()


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("mode", MODES)
def test_plane_image_and_tile_walk_change_no_bit(lib, on_gpu, mdopt, eager, precision, mode, lay):
    """options gemm_bf16x3_planes 0 / 1 and gemm_bf16x3_band 1 / forced 2 apply to the reduced kernels and leave every bit"""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    precision(mode)
    rng = np.random.default_rng(56)
    M, K, N = 768, 160, 384
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    ref = nd.matmul(a, b).get()
    for planes in (0, 1):
        for band in (1, 2, 0):
            mdopt("gemm_bf16x3_planes", planes)
            mdopt("gemm_bf16x3_band", band)
            r0 = _runs(lib)
            got = nd.matmul(a, b).get()
            assert _runs(lib) == r0 + 1
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (planes, band)


@pytest.mark.gpu
def test_default_is_untouched_and_untaken_shapes_keep_their_bits(lib, on_gpu, mdopt, eager, precision):
    """"highest" before and after a visit to "medium": the same bits (the six-product kernel, counted); a ragged shape and a batch
    under "medium": the bits of "highest", no launch of the product kernels."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(57)
    M, K, N = 512, 96, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = nd.asarray(A), nd.asarray(B)
    assert nd.get_matmul_precision() == "highest" and _get(lib, "gemm_products") == 6
    before = nd.matmul(a, b).get()
    precision("medium")
    reduced = nd.matmul(a, b).get()
    precision("highest")
    r0 = _runs(lib)
    after = nd.matmul(a, b).get()
    assert _runs(lib) == r0 + 1
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert not np.array_equal(before, reduced)

    def randn(*shape):
        return nd.asarray(rng.standard_normal(shape, dtype=np.float32))

    cases = {"ragged m": (randn(M + 4, K), randn(K, N)), "ragged k": (randn(M, K + 4), randn(K + 4, N)), "batch": (randn(2, M, K), randn(2, K, N))}
    for name, (x, y) in cases.items():
        precision("highest")
        ref = nd.matmul(x, y).get()
        precision("medium")
        r0 = _runs(lib)
        got = nd.matmul(x, y).get()
        assert _runs(lib) == r0, name
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), name


@pytest.mark.gpu
def test_default_option_routes_by_the_floors_of_the_mode(lib, on_gpu, eager, precision):
    """Option gemm_bf16x3 untouched (1). M x K x N = 512 x 1024 x 2048 runs on the planes under "medium" (floors N 2048, K 1024) and
    not under "high" (K 2048) or "highest" (4096 both); N = 1024 under none. 2048 x 4096 x 2048 and its 512- and 1024-row panels —
    shapes the k ranges of the fp32 plan would take for M <= 1024 alone — keep one route and agree bit for bit under "high"."""
    assert on_gpu
    nd = eager
    assert _get(lib, "gemm_bf16x3") == 1
    rng = np.random.default_rng(59)
    a = nd.asarray(rng.standard_normal((512, 1024), dtype=np.float32))
    b = nd.asarray(rng.standard_normal((1024, 2048), dtype=np.float32))
    for mode, counted in (("highest", 0), ("high", 0), ("medium", 1)):
        precision(mode)
        r0 = _runs(lib)
        nd.matmul(a, b).get()
        assert _runs(lib) - r0 == counted, mode
        nd.matmul(a, b[:, :1024]).get()
        assert _runs(lib) - r0 == counted, mode
    a = nd.asarray(rng.standard_normal((2048, 4096), dtype=np.float32))
    b = nd.asarray(rng.standard_normal((4096, 2048), dtype=np.float32))
    precision("high")
    r0 = _runs(lib)
    whole = nd.matmul(a, b).get()
    for rows in (512, 1024):
        assert np.array_equal(nd.matmul(a[:rows], b).get().view(np.uint32), whole[:rows].view(np.uint32)), rows
    assert _runs(lib) == r0 + 3


@pytest.mark.gpu
def test_forward_and_backward_sweep_under_high(lib, on_gpu, mdopt, precision):
    """sum((X @ W) * G).backward() through tape.build_engine at 512 x 1024 x 1024: the forward product (NN) and the two gradients
    G @ W^T (NT) and X^T @ G (TN) each launch the product kernel once and are norm-wise within the high bound of float64."""
    assert on_gpu
    from minidiff_amd.hip_backend import HipBackendTable
    from minidiff_amd.tape import build_engine
    md = build_engine(HipBackendTable, "precision")
    mdopt("gemm_bf16x3", 2)
    mdopt("gemm_splitk", 0)   # (128 64 x 64 tiles under k = 1024: the fp32 stand-in must be one plain launch, see plan_bf16x3)
    precision("high")
    rng = np.random.default_rng(58)
    M, K, N = 512, 1024, 1024
    Xh, Wh, Gh = (rng.standard_normal(s, dtype=np.float32) for s in ((M, K), (K, N), (M, N)))
    X, W, G = md.Tensor(Xh, allow_grad=True), md.Tensor(Wh, allow_grad=True), md.Tensor(Gh)
    r0 = _runs(lib)
    Y = X @ W
    md.sum(Y * G).backward()
    got = {"Y": Y.as_numpy(), "dX": X.grad.as_numpy(), "dW": W.grad.as_numpy()}
    assert _runs(lib) == r0 + 3
    X64, W64, G64 = Xh.astype(np.float64), Wh.astype(np.float64), Gh.astype(np.float64)
    want = {"Y": (X64, W64), "dX": (G64, W64.T), "dW": (X64.T, G64)}
    for name, (p, q) in want.items():
        err = np.linalg.norm(got[name] - p @ q)
        bound = np.linalg.norm(_bound("high", np.abs(p) @ np.abs(q), p.shape[1]))
        print(f"{name}: |err| / bound {err / bound:.3f}, norm-wise error {err / np.linalg.norm(p @ q):.3e}")
        assert err <= bound, name
