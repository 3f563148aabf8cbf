"""Loop 2 of the bf16x3 product kernel (csrc/gemm_bf16x3.hip, option gemm_bf16x3_loop = 2): the two halves of the block — waves
0 .. 3 and 4 .. 7, one wave of each per SIMD — run one segment apart, so that on every SIMD one wave issues MFMAs while its partner
reads fragments, stages the next tile and folds. Who does what when changes and nothing else: the tile, the planes, the LDS image,
the product order and the fold per k-tile are loop 1's, so the BITS must be loop 1's.

Shapes (M x K x N): 256 x 32 x 128 (one tile, one k-tile: prologue and epilogue only), 256 x 64 x 128 (two k-tiles), 256 x 96 x 128
(an odd count: the unrolled pair breaks in the middle), 512 x 160 x 256 (four tiles), 768 x 128 x 640 (15 tiles: the XCD order with
a remainder, and bands). The kernel facts — what each segment between two barriers holds, the barrier count — are read from the
shipped library (scripts/isa_check.py report_bf16x3_loop2; no GPU needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
OBJ = os.path.join(ROOT, "minidiff_amd", "libmdhip.so")

SHAPES = ((256, 32, 128), (256, 64, 128), (256, 96, 128), (512, 160, 256), (768, 128, 640))
LAYOUTS = ("NN", "NT", "TN")


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


def _product(lib, mdopt, nd, a, b, loop, what):
    """one launch of the product kernel under the loop"""
    mdopt("gemm_bf16x3_loop", loop)
    r0 = _runs(lib)
    got = nd.matmul(a, b).get()
    assert _runs(lib) == r0 + 1, (what, loop)
    return got


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("planes", (0, 1))
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_2_gives_the_bits_of_loop_1(lib, on_gpu, mdopt, eager, lay, planes):
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    mdopt("gemm_bf16x3_planes", planes)
    rng = np.random.default_rng(43)
    for (M, K, N) in SHAPES:
        data = (("randn", rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)),
                # all-positive: the data on which a changed accumulation order shows (the matrix instruction truncates)
                ("uniform(0.5, 1.5)", rng.uniform(0.5, 1.5, (M, K)).astype(np.float32), rng.uniform(0.5, 1.5, (K, N)).astype(np.float32)))
        for name, A, B in data:
            what = (lay, planes, M, K, N, name)
            a, b = _operands(nd, A, B, lay)
            one = _product(lib, mdopt, nd, a, b, 1, what)
            two = _product(lib, mdopt, nd, a, b, 2, what)
            assert np.array_equal(_bits(one), _bits(two)), what


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_2_is_exact_on_integers_and_the_identity(lib, on_gpu, mdopt, eager, lay):
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(44)
    for (M, K, N) in SHAPES:
        small = (1 << 24) // (2000 * K)   # sums stay below 2^24: the product is exact
        A, B = rng.integers(-2000, 2001, (M, K)), rng.integers(-small, small + 1, (K, N))
        a, b = _operands(nd, A.astype(np.float32), B.astype(np.float32), lay)
        assert np.array_equal(_product(lib, mdopt, nd, a, b, 2, (lay, M, K, N)), (A @ B).astype(np.float32)), (lay, M, K, N, "integers")
    # identity x random: M = K = 256, and the identity on the right with K = N = 128
    X = rng.standard_normal((256, 128), dtype=np.float32) * np.exp2(rng.integers(-20, 20, (256, 128))).astype(np.float32)
    a, b = _operands(nd, np.eye(256, dtype=np.float32), X, lay)
    assert np.array_equal(_bits(_product(lib, mdopt, nd, a, b, 2, (lay, "I X"))), _bits(X)), (lay, "I X")
    a, b = _operands(nd, X, np.eye(128, dtype=np.float32), lay)
    assert np.array_equal(_bits(_product(lib, mdopt, nd, a, b, 2, (lay, "X I"))), _bits(X)), (lay, "X I")


@pytest.mark.gpu
def test_loop_2_row_panel_in_a_wider_array_keeps_the_padding(lib, on_gpu, mdopt, eager):
    """The product written into a row panel of a wider array (rows c_ms = 640 > N = 256 floats apart): loop 2 writes loop 1's bits
    there and leaves the fill pattern beside them."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(45)
    M, K, N, W = 512, 160, 256, 640
    a, b = nd.asarray(rng.standard_normal((M, K), dtype=np.float32)), nd.asarray(rng.standard_normal((K, N), dtype=np.float32))
    got = {}
    for loop in (1, 2):
        mdopt("gemm_bf16x3_loop", loop)
        bucket = nd.asarray(np.full((M + 256, W), 7.0, np.float32))
        c = bucket[256:, 128:128 + N]
        assert c.shape == (M, N) and c._strides == (W, 1)
        r0 = _runs(lib)
        nd._lib().matmul(a._view(a._offset, (1, M, K), (0,) + a._strides).desc(), b._view(b._offset, (1, K, N), (0,) + b._strides).desc(),
                         c._view(c._offset, (1, M, N), (0,) + c._strides).desc())
        assert _runs(lib) == r0 + 1, loop
        got[loop] = bucket.get()
    assert np.array_equal(_bits(got[1]), _bits(got[2]))
    inside = np.zeros((M + 256, W), bool)
    inside[256:, 128:128 + N] = True
    assert (got[2][~inside] == 7.0).all() and not (got[2][inside] == 7.0).all()


@pytest.mark.gpu
def test_loop_2_leaves_an_operand_with_an_inf_to_the_stand_in(lib, on_gpu, mdopt, eager):
    """One inf in an operand: the split pass raises the flag word, the product kernel returns before its first barrier and the fp32
    kernel behind it computes the product — the same result under either loop."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(46)
    M, K, N = 512, 160, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    A[300, 77] = np.inf
    a, b = nd.asarray(A), nd.asarray(B)
    one = _product(lib, mdopt, nd, a, b, 1, "inf")
    two = _product(lib, mdopt, nd, a, b, 2, "inf")
    assert np.array_equal(_bits(one), _bits(two))
    assert not np.isfinite(two[300]).any() and np.isfinite(np.delete(two, 300, axis=0)).all()


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(OBJ):
        pytest.skip("minidiff_amd/libmdhip.so not built (run __graft_entry__.build())")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("llvm-objdump not available")
    import isa_check
    return isa_check.report_bf16x3_loop2(OBJ)


def test_bf16x3_loop_2_kernel_shape(isa):
    k = isa
    # two k-tiles per trip: 96 MFMAs, 18 pieces in the scalar-base + 32-bit lane offset form, their bases stepped without a multiply
    assert k["mfma_loop"] == 96, k
    assert k["dma_loop"] == 18 and k["dma_loop_saddr"] == 18 and k["dma_loop_vaddr64"] == 0 and k["lshl_add_u64_loop"] == 0, k
    assert k["s_mul_loop"] == 0, k
    # the fold: 64 scalar adds per k-tile, none packed; nothing staged through registers, no scratch, two waves per SIMD
    assert k["v_add_f32_loop"] == 128 and k["v_pk_add_f32_loop"] == 0, k
    assert k["ds_write"] == 0 and k["scratch"] == 0 and k["vgprs"] <= 256, k
    # four segments per k-tile, each ended by a barrier — L(2 kt): 12 reads, three pieces, the fold; C(2 kt): 24 MFMAs with the
    # other six pieces between them; L(2 kt + 1): 12 reads and the wait alone; C(2 kt + 1): 24 MFMAs and nothing else
    assert k["barrier_loop"] == 8 and len(k["segments"]) == 8, k
    tile = [{"mfma": 0, "ds_read": 12, "dma": 3, "v_add_f32": 64}, {"mfma": 24, "ds_read": 0, "dma": 6, "v_add_f32": 0},
            {"mfma": 0, "ds_read": 12, "dma": 0, "v_add_f32": 0}, {"mfma": 24, "ds_read": 0, "dma": 0, "v_add_f32": 0}]
    assert k["segments"] == tile + tile, k
    assert k["tail_after_last_barrier"] == {"mfma": 0, "ds_read": 0, "dma": 0, "v_add_f32": 0}, k
    # no drain between a barrier and the first fragment read behind it
    assert k["vmcnt0_between_barrier_and_first_read"] == 0, k
    assert k["loop1_present"], k
