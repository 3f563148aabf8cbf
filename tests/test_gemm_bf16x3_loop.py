"""The two k loops of the bf16x3 product kernel (csrc/gemm_bf16x3.hip, option gemm_bf16x3_loop): loop 1 — staging addresses formed
once, the next tile's DMAs, the fragment reads of the second k16 step and the fold placed under the MFMAs, the last sub-tile's sum
carried over the barrier — must give the BITS of loop 0, the loop the kernel was merged with. Only the interleaving between
different accumulators moved; every element keeps its 12 accumulations per k-tile in their order and its one add per k-tile.

Shapes: 2, 8 and 9 blocks (9: the XCD mapping has a remainder); k-tiles 1 (the prologue alone), 2, 3, 4, 5 (odd and even counts, a
break in the middle of the unrolled pair), 8 and 9 (the carried fold and the read pipeline reach steady state and drain)."""
import ctypes as C

import numpy as np
import pytest

TK = 32
LAYOUTS = ("NN", "NT", "TN", "TT")
MN = ((256, 128), (512, 256), (768, 384))
KS = tuple(TK * k for k in (1, 2, 3, 4, 5, 8, 9))


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


def _both_arms(lib, mdopt, nd, a, b, what):
    """the product under loop 0 and under loop 1: one launch of the product kernel each"""
    got = []
    for arm in (0, 1):
        mdopt("gemm_bf16x3_loop", arm)
        r0 = _runs(lib)
        got.append(nd.matmul(a, b).get())
        assert _runs(lib) == r0 + 1, (what, arm)
    assert np.array_equal(got[0], got[1]), what
    return got[1]


def _cases(rng, M, K, N):
    """(name, A, B, exact product or None)"""
    scale = lambda *s: np.exp2(rng.integers(-20, 20, s)).astype(np.float32)   # noqa: E731
    yield "randn x 2^e", rng.standard_normal((M, K), dtype=np.float32) * scale(M, K), rng.standard_normal((K, N), dtype=np.float32) * scale(K, N), None
    # all-positive: the data the matrix instruction's truncating accumulation shows on
    yield "uniform(0.5, 1.5)", rng.uniform(0.5, 1.5, (M, K)).astype(np.float32), rng.uniform(0.5, 1.5, (K, N)).astype(np.float32), None
    small = (1 << 24) // (2000 * K)   # sums stay below 2^24: the product is exact
    A, B = rng.integers(-2000, 2001, (M, K)), rng.integers(-small, small + 1, (K, N))
    yield "integers", A.astype(np.float32), B.astype(np.float32), (A @ B).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_loop_1_gives_the_bits_of_loop_0(lib, on_gpu, mdopt, eager, lay):
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(41)
    for (M, N) in MN:
        for K in KS:
            for name, A, B, exact in _cases(rng, M, K, N):
                a, b = _operands(nd, A, B, lay)
                got = _both_arms(lib, mdopt, nd, a, b, (lay, M, K, N, name))
                if exact is not None:
                    assert np.array_equal(got, exact), (lay, M, K, N, name)


@pytest.mark.gpu
def test_row_panel_output_in_a_wider_array(lib, on_gpu, mdopt, eager):
    """The product written into a row panel of a wider array (rows c_ms = 640 > N = 256 floats apart): through out= where the panel
    spans whole rows of a taller array, and — matmul's out= wants a contiguous array — through the library call matmul itself makes
    where it does not. Both loops write the same bits there and nothing beside them."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(42)
    M, K, N, W = 512, 288, 256, 640
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = nd.asarray(A), nd.asarray(B)
    got, tall = [], []
    for arm in (0, 1):
        mdopt("gemm_bf16x3_loop", arm)
        bucket = nd.asarray(np.full((M + 256, W), 7.0, np.float32))
        c = bucket[256:, 128:128 + N]
        assert c.shape == (M, N) and c._strides == (W, 1)
        r0 = _runs(lib)
        nd._lib().matmul(a._view(a._offset, (1, M, K), (0,) + a._strides).desc(), b._view(b._offset, (1, K, N), (0,) + b._strides).desc(),
                         c._view(c._offset, (1, M, N), (0,) + c._strides).desc())
        assert _runs(lib) == r0 + 1, arm
        got.append(bucket.get())
        rows = nd.asarray(np.full((M + 256, N), 7.0, np.float32))
        nd.matmul(a, b, out=rows[256:])
        assert _runs(lib) == r0 + 2, arm
        tall.append(rows.get())
    assert np.array_equal(tall[0], tall[1]) and (tall[1][:256] == 7.0).all()
    assert np.array_equal(tall[1][256:], got[1][256:, 128:128 + N])
    assert np.array_equal(got[0], got[1])
    inside = np.zeros((M + 256, W), bool)
    inside[256:, 128:128 + N] = True
    assert (got[1][~inside] == 7.0).all()
    ref = A.astype(np.float64) @ B
    assert np.abs(got[1][256:, 128:128 + N] - ref).max() / np.abs(ref).max() < 2e-6   # (the randn bound of test_gemm_bf16x3.py)
