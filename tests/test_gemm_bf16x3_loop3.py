"""Loop 3 of the bf16x3 product kernel (csrc/gemm_bf16x3.hip, option gemm_bf16x3_loop = 3): loop 2's two halves one segment apart
on v_mfma_f32_16x16x32_bf16 — one instruction per k-tile, the wave tile formed as two 32 x 64 halves, an LDS swizzle of its own.
Its bits are its own (six truncating accumulations of 32 terms per k-tile where loops 0 - 2 take twelve of 16), so nothing here is
compared with another loop: the operand and accumulator maps (identity products, bit for bit), exactness on integers, the float64
contract, determinism, panels, the stand-in and the bias at depth are asserted for loop 3 by itself, set explicitly whatever the
default is.

Shapes (M x K x N): 256 x 32 x 128 (one tile, one k-tile: the unstaged tail tile alone), 256 x 64 x 128 (the pair tail),
256 x 96 x 128 (one trip of the loop and the single tail), 512 x 128 x 256 (four tiles, four k-tiles: the tile walk),
768 x 160 x 384 (five k-tiles; the panel shape). The kernel facts are read from the shipped library (scripts/isa_check.py
report_bf16x3_loop3; no GPU needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OBJ = os.path.join(ROOT, "minidiff_amd", "libmdhip.so")

TM = 256
SHAPES = ((256, 32, 128), (256, 64, 128), (256, 96, 128), (512, 128, 256), (768, 160, 384))
LAYOUTS = ("NN", "NT", "TN", "TT")


def _runs(lib):
    v = C.c_int64()
    lib.debug_get_option(b"gemm_bf16x3_runs", C.byref(v))
    return v.value


def _operands(nd, A, B, lay):
    """device views of A (M x K) and B (K x N) in the layout: 'T' = stored transposed, passed as the transposed view"""
    a = nd.asarray(np.ascontiguousarray(A.T)).T if lay[0] == "T" else nd.asarray(A)
    b = nd.asarray(np.ascontiguousarray(B.T)).T if lay[1] == "T" else nd.asarray(B)
    return a, b


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.fixture
def loop3(lib, on_gpu, mdopt):
    """(nd, product): eager mode, the six products on every eligible shape, loop 3; product() is one counted launch of the kernel"""
    assert on_gpu
    from minidiff_amd import ndarray as nd
    prev = nd.set_lazy(False)
    mdopt("gemm_bf16x3", 2)
    mdopt("gemm_bf16x3_loop", 3)

    def product(a, b, what, **kw):
        r0 = _runs(lib)
        got = nd.matmul(a, b, **kw)
        assert _runs(lib) == r0 + 1, what
        return got

    yield nd, product
    nd.set_lazy(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_3_maps_identity_on_either_side_is_bit_exact(loop3, lay):
    """A = I with an asymmetric B, B = I with an asymmetric A (n = 256; scaled by 2^-20 .. 2^20 so that all three planes carry data):
    a wrong operand or accumulator map, or a wrong swizzle, moves or mixes elements."""
    nd, product = loop3
    rng = np.random.default_rng(51)
    n = 256
    x = rng.standard_normal((n, n), dtype=np.float32) * np.exp2(rng.integers(-20, 21, (n, n))).astype(np.float32)
    eye = np.eye(n, dtype=np.float32)
    for name, A, B in (("I X", eye, x), ("X I", x, eye)):
        a, b = _operands(nd, A, B, lay)
        assert np.array_equal(_bits(product(a, b, (lay, name)).get()), _bits(x)), (lay, name)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_3_integers_randn_and_two_calls_on_every_shape(loop3, lay):
    """Integers in -2000 .. 2000 (two planes) against small ones, sums below 2^24, either way round: EQUAL to NumPy's integer
    product. randn: within 2e-6 (max-norm) of float64, and a second call gives the same bits."""
    nd, product = loop3
    rng = np.random.default_rng(52)
    for (M, K, N) in SHAPES:
        small = (1 << 24) // (2000 * K)
        for big_a in (True, False):
            A = rng.integers(-2000, 2001, (M, K)) if big_a else rng.integers(-small, small + 1, (M, K))
            B = rng.integers(-small, small + 1, (K, N)) if big_a else rng.integers(-2000, 2001, (K, N))
            a, b = _operands(nd, A.astype(np.float32), B.astype(np.float32), lay)
            assert np.array_equal(product(a, b, (lay, M, K, N)).get(), (A @ B).astype(np.float64)), (lay, M, K, N, big_a)
        fa, fb = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
        a, b = _operands(nd, fa, fb, lay)
        got = product(a, b, (lay, M, K, N)).get()
        err = _rel(got, fa.astype(np.float64) @ fb)
        print(f"{lay} {M} x {K} x {N}: randn max-norm error {err:.3e}")
        assert err < 2e-6, (lay, M, K, N, err)
        assert np.array_equal(_bits(product(a, b, (lay, M, K, N)).get()), _bits(got)), (lay, M, K, N)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_3_row_panels_carry_the_bits_of_the_whole_product(loop3, lay):
    """768 x 160 x 384: the first 256-row panel, and a two-tile-row panel written through out= into a row-panel view of a larger
    array, are bit-equal to the same rows of the whole product; the rows outside the panel keep their fill."""
    nd, product = loop3
    rng = np.random.default_rng(53)
    M, K, N = 768, 160, 384
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    whole = product(a, b, lay).get()
    assert np.array_equal(_bits(product(a[:TM], b, lay).get()), _bits(whole[:TM])), lay
    bucket = nd.asarray(np.full((M, N), 7.0, np.float32))
    product(a[TM:3 * TM], b, lay, out=bucket[TM:3 * TM])
    got = bucket.get()
    assert np.array_equal(_bits(got[TM:]), _bits(whole[TM:])), lay
    assert (got[:TM] == 7.0).all(), lay


@pytest.mark.gpu
def test_loop_3_leaves_an_operand_with_an_inf_to_the_stand_in(loop3, mdopt):
    """An inf planted in A at 512 x 96 x 256: the NaN / inf pattern and the finite bits of gemm_bf16x3 = 0, and the flag does not
    stick — the next finite product runs on the planes again."""
    nd, product = loop3
    rng = np.random.default_rng(54)
    M, K, N = 512, 96, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    A2 = A.copy()
    A2[300, 77] = np.inf
    a, b = nd.asarray(A2), nd.asarray(B)
    mdopt("gemm_bf16x3", 0)
    ref = nd.matmul(a, b).get()
    mdopt("gemm_bf16x3", 2)
    got = product(a, b, "inf").get()
    assert not np.isfinite(ref).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(_bits(got)[~np.isnan(ref)], _bits(ref)[~np.isnan(ref)])
    assert _rel(product(nd.asarray(A), nd.asarray(B), "finite again").get(), A.astype(np.float64) @ B) < 2e-6


@pytest.mark.gpu
def test_loop_3_all_positive_operands_at_depth(loop3):
    """Same-sign operands at 512 x 4096 x 2304 (the smallest full grid the k ranges leave alone): 2e-6 norm-wise against float64, and
    a mean error under 6 * 2^-23 of the largest element — the worst case of the six truncating accumulations of one k-tile into a
    fresh accumulator, which no K adds to (the k-tiles are added with round-to-nearest adds)."""
    nd, product = loop3
    rng = np.random.default_rng(36)
    M, K, N = 512, 4096, 2304
    A, B = np.abs(rng.standard_normal((M, K), dtype=np.float32)), np.abs(rng.standard_normal((K, N), dtype=np.float32))
    ref = A.astype(np.float64) @ B
    got = product(nd.asarray(A), nd.asarray(B), "depth").get().astype(np.float64)
    fro = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    bias = float(np.mean(got - ref) / np.abs(ref).max())
    print(f"loop 3: norm-wise {fro:.3e}, mean error / max {bias:+.3e} (bound {6 * 2.0 ** -23:.3e})")
    assert fro < 2e-6, fro
    assert abs(bias) < 6 * 2.0 ** -23, bias


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(OBJ):
        pytest.skip("minidiff_amd/libmdhip.so not built (run __graft_entry__.build())")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    import isa_check
    return isa_check.report_bf16x3_loop3(OBJ)


def test_bf16x3_loop_3_kernel_shape(isa):
    k = isa
    # two k-tiles per trip, 96 MFMAs of the 16x16x32 shape each and none of the 32x32x16 one; no scratch, two waves per SIMD
    assert k["mfma_16x16x32_loop"] == 2 * 96 and k["mfma_32x32x16_loop"] == 0 and k["mfma_loop"] == 2 * 96, k
    assert k["scratch"] == 0 and k["vgprs"] <= 256 and k["ds_write"] == 0, k
    # 18 pieces per trip in the scalar-base + 32-bit lane offset form; the fold: 64 scalar adds per k-tile, none packed
    assert k["dma_loop"] == 18 and k["dma_loop_saddr"] == 18 and k["dma_loop_vaddr64"] == 0 and k["s_mul_loop"] == 0, k
    assert k["v_add_f32_loop"] == 128 and k["v_pk_add_f32_loop"] == 0, k
    # four segments per k-tile — L(2 kt): all of B and A rows 0 .. 31 (18 reads), three pieces, the fold of the half before;
    # C(2 kt): 48 MFMAs with the other six pieces between them; L(2 kt + 1): A rows 32 .. 63 (6 reads) and the fold of rows
    # 0 .. 31, no piece in front of its vmcnt(0); C(2 kt + 1): 48 MFMAs and nothing else
    assert k["barrier_loop"] == 8 and len(k["segments"]) == 8, k
    tile = [{"mfma": 0, "ds_read": 18, "dma": 3, "v_add_f32": 32}, {"mfma": 48, "ds_read": 0, "dma": 6, "v_add_f32": 0},
            {"mfma": 0, "ds_read": 6, "dma": 0, "v_add_f32": 32}, {"mfma": 48, "ds_read": 0, "dma": 0, "v_add_f32": 0}]
    assert k["segments"] == tile + tile, k
    assert k["tail_after_last_barrier"] == {"mfma": 0, "ds_read": 0, "dma": 0, "v_add_f32": 0}, k
    assert k["vmcnt0_between_barrier_and_first_read"] == 0, k
