"""Where the bf16x3 product's bytes lie and in which order its tiles run (csrc/md_bf16x3_layout.h, csrc/gemm_bf16x3.hip): the plane
image (option gemm_bf16x3_planes: 0 [rows][K] | 1 k-tile-major [K / 32][rows][64 B]) and the band height of the tile walk (option
gemm_bf16x3_band: 0 by the CU count | 1 row-major | n forced). Neither touches an accumulation — an output element's bits depend on
the k order alone — so every arm must give the BITS of planes 0 + band 1, the arm the kernel was merged with.

On the host: the two maps of the header in a stand-alone program (also under the address and undefined-behaviour sanitizers). On the
GPU: tile grids of 1 .. 32 blocks with M != N wherever the grid allows it (1 x 2 tiles of 256 x 128 are square), so that A's and
B's k steps, which differ under planes 1, cannot be swapped unseen; 1, 2, 3, 5 and 9 k-tiles; the four operand layouts (both split
kernels on either side)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- host --------------------------------------------------------------------------------------------------------------------------
_MAPS_MAIN = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "md_bf16x3_layout.h"

static unsigned long long fails = 0, seen = 0;
#define CHECK(c) do { ++seen; if (!(c)) { if (++fails <= 10) printf("line %d: %s\n", __LINE__, #c); } } while (0)

/* the tile walk: every wg of the grid lands on a tile of the grid, no tile twice; gm = 1 is the row-major walk; a group's tiles run
   tile_m fastest over min(gm, tiles_m - first_m) rows */
static void walk(int tiles_m, int tiles_n, int gm) {
  const int n = tiles_m * tiles_n;
  unsigned char *hit = (unsigned char *)calloc((size_t)n, 1);
  for (int wg = 0; wg < n; ++wg) {
    int tm = -1, tn = -1;
    md_bf16x3_tile(wg, tiles_m, tiles_n, gm, &tm, &tn);
    const bool inside = tm >= 0 && tm < tiles_m && tn >= 0 && tn < tiles_n;
    CHECK(inside);
    if (!inside) continue;
    CHECK(!hit[tm * tiles_n + tn]);
    hit[tm * tiles_n + tn] = 1;
    if (gm == 1) CHECK(tm == wg / tiles_n && tn == wg % tiles_n);
    const int first_m = tm / gm * gm, h = tiles_m - first_m < gm ? tiles_m - first_m : gm, in = wg - first_m * tiles_n;
    CHECK(in >= 0 && in < h * tiles_n && tm == first_m + in % h && tn == in / h);
  }
  for (int i = 0; i < n; ++i) CHECK(hit[i]);
  free(hit);
}

/* the plane image: (row, k) -> byte offset is a bijection onto [0, rows K 2) in 2-byte steps, and under layout 1 every 16-row piece
   of a k-tile is 1 KiB contiguous and 16-B aligned, the four 16-B chunks of a row in k order */
static void image(int planes, long long rows, long long K) {
  const long long rs = md_bf16x3_row_stride(planes, K), ks = md_bf16x3_k_step(planes, rows), bytes = rows * K * 2;
  unsigned char *hit = (unsigned char *)calloc((size_t)(bytes / 2), 1);
  for (long long r = 0; r < rows; ++r)
    for (long long k = 0; k < K; ++k) {
      const long long o = md_bf16x3_plane_off(r, k, rs, ks);
      const bool inside = o >= 0 && o + 2 <= bytes && o % 2 == 0;
      CHECK(inside);
      if (!inside) continue;
      CHECK(!hit[o / 2]);
      hit[o / 2] = 1;
      if (planes == 0) CHECK(o == (r * K + k) * 2);
    }
  for (long long i = 0; i < bytes / 2; ++i) CHECK(hit[i]);
  free(hit);
  if (planes == 1)
    for (long long kt = 0; kt < K / 32; ++kt)
      for (long long r0 = 0; r0 < rows; r0 += 16) {
        const long long base = md_bf16x3_plane_off(r0, kt * 32, rs, ks);
        CHECK(base % 1024 == 0);
        for (long long r = 0; r < 16; ++r)
          for (long long k = 0; k < 32; ++k) CHECK(md_bf16x3_plane_off(r0 + r, kt * 32 + k, rs, ks) == base + r * 64 + k * 2);
      }
}

int main(void) {
  for (int tm = 1; tm <= 40; ++tm)
    for (int tn = 1; tn <= 40; ++tn)
      for (int gm = 1; gm <= 8; ++gm) walk(tm, tn, gm);
  const long long R[] = {16, 48, 256, 768}, Ks[] = {32, 64, 160, 288};
  for (int p = 0; p < 2; ++p)
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) image(p, R[i], Ks[j]);
  /* the band for 32 resident blocks: 256 gm + 128 ceil(32 / gm) is least at 4; clipped to the grid; a forced height is clipped too */
  CHECK(md_bf16x3_band(16, 32, 0) == 4 && md_bf16x3_band(32, 32, 0) == 4 && md_bf16x3_band(4, 32, 0) == 4);
  CHECK(md_bf16x3_band(2, 32, 0) == 2 && md_bf16x3_band(1, 32, 0) == 1 && md_bf16x3_band(3, 32, 0) == 3);
  CHECK(md_bf16x3_band(16, 32, 1) == 1 && md_bf16x3_band(16, 32, 8) == 8 && md_bf16x3_band(5, 32, 8) == 5);
  printf("checked %llu failed %llu\n", seen, fails);
  return fails != 0;
}
"""


def _build_and_run(tmp_path, name, flags):
    cxx = shutil.which("g++") or shutil.which("gcc")
    assert cxx, "no host compiler"
    src = tmp_path / (name + ".cpp")
    src.write_text(_MAPS_MAIN)
    exe = tmp_path / name
    subprocess.check_call([cxx, "-O1", "-g", *flags, "-I", os.path.join(ROOT, "minidiff_amd", "csrc"), "-o", str(exe), str(src)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "failed 0" in run.stdout and "checked " in run.stdout, run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr


def test_tile_walk_and_plane_image_on_the_host(tmp_path):
    """md_bf16x3_tile is a bijection onto the grid for every tiles_m, tiles_n in 1 .. 40 and gm in 1 .. 8 (block counts with a
    remainder over the eight XCDs, a ragged last group, gm > tiles_m); md_bf16x3_plane_off is a bijection onto the plane for rows in
    16 {1, 3, 16, 48} and K in 32 {1, 2, 5, 9}, and puts a 16-row piece of a k-tile into one aligned KiB under layout 1."""
    _build_and_run(tmp_path, "maps_main", [])


def test_tile_walk_and_plane_image_on_the_host_under_sanitizers(tmp_path):
    """The same stand-alone program built with the address and undefined-behaviour sanitizers of the host compiler."""
    _build_and_run(tmp_path, "maps_main_san", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
TM, TN, TK = 256, 128, 32
LAYOUTS = ("NN", "NT", "TN", "TT")
GRIDS = ((1, 1), (1, 2), (2, 1), (3, 3), (5, 2), (2, 5), (8, 4), (9, 3))   # tiles_m x tiles_n
KS = tuple(TK * k for k in (1, 2, 3, 5, 9))
PARENT = (0, 1, 1)   # (planes, band, loop): the arm the kernel was merged with


def _arms(grid):
    """every arm but the parent's: planes 0 / 1 x band 1 / automatic / forced (3: ragged groups on 5, 8 and 9 tile rows; 2 and 8
    on the 8 x 4 grid, one full round of the XCDs), and the first loop under both images"""
    forced = (3,) + ((2, 8) if grid == (8, 4) else ())
    arms = [(p, b, 1) for p in (0, 1) for b in (1, 0) + forced if (p, b, 1) != PARENT]
    return arms + [(0, 0, 0), (1, 0, 0), (1, 1, 0)]


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


def _set(mdopt, arm):
    mdopt("gemm_bf16x3_planes", arm[0])
    mdopt("gemm_bf16x3_band", arm[1])
    mdopt("gemm_bf16x3_loop", arm[2])


def _product(lib, mdopt, nd, a, b, arm, what):
    """one product under the arm: exactly one launch of the product kernel"""
    _set(mdopt, arm)
    r0 = _runs(lib)
    got = nd.matmul(a, b).get()
    assert _runs(lib) == r0 + 1, (what, arm)
    return got


def _cases(rng, M, K, N):
    """(name, A, B, exact product or None): the data of test_gemm_bf16x3_loop.py"""
    scale = lambda *s: np.exp2(rng.integers(-20, 20, s)).astype(np.float32)   # noqa: E731
    yield "randn x 2^e", rng.standard_normal((M, K), dtype=np.float32) * scale(M, K), rng.standard_normal((K, N), dtype=np.float32) * scale(K, N), None
    yield "uniform(0.5, 1.5)", rng.uniform(0.5, 1.5, (M, K)).astype(np.float32), rng.uniform(0.5, 1.5, (K, N)).astype(np.float32), None
    small = (1 << 24) // (2000 * K)   # sums stay below 2^24: the product is exact
    A, B = rng.integers(-2000, 2001, (M, K)), rng.integers(-small, small + 1, (K, N))
    yield "integers", A.astype(np.float32), B.astype(np.float32), (A @ B).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("lay", LAYOUTS)
def test_every_arm_gives_the_bits_of_the_parent_arm(lib, on_gpu, mdopt, eager, lay, grid):
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(51)
    M, N = grid[0] * TM, grid[1] * TN
    for K in KS:
        for name, A, B, exact in _cases(rng, M, K, N):
            what = (lay, M, K, N, name)
            a, b = _operands(nd, A, B, lay)
            ref = _product(lib, mdopt, nd, a, b, PARENT, what)
            if exact is not None:
                assert np.array_equal(ref, exact), what
            for arm in _arms(grid):
                got = _product(lib, mdopt, nd, a, b, arm, what)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, arm)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_strided_panel_of_a_wider_array_keeps_its_padding(lib, on_gpu, mdopt, eager, lay):
    """C as a column panel (rows 640 floats apart, N = 256) of a wider array filled with a pattern: every arm writes the parent
    arm's bits into the panel and nothing beside it. 5 x 2 tiles: a ragged last group under the automatic band."""
    assert on_gpu
    nd = eager
    mdopt("gemm_bf16x3", 2)
    rng = np.random.default_rng(52)
    M, K, N, W = 1280, 288, 256, 640
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    fill = (np.arange((M + 256) * W, dtype=np.float32) % 1021.0).reshape(M + 256, W)
    inside = np.zeros((M + 256, W), bool)
    inside[256:, 128:128 + N] = True
    ref = None
    for arm in [PARENT] + _arms((5, 2)):
        _set(mdopt, arm)
        bucket = nd.asarray(fill)
        c = bucket[256:, 128:128 + N]
        assert c.shape == (M, N) and c._strides == (W, 1)
        r0 = _runs(lib)
        nd._lib().matmul(a._view(a._offset, (1, M, K), (0,) + a._strides).desc(), b._view(b._offset, (1, K, N), (0,) + b._strides).desc(),
                         c._view(c._offset, (1, M, N), (0,) + c._strides).desc())
        assert _runs(lib) == r0 + 1, arm
        got = bucket.get()
        assert np.array_equal(got[~inside], fill[~inside]), arm
        if ref is None:
            ref = got
            exact = A.astype(np.float64) @ B
            assert np.abs(got[256:, 128:128 + N] - exact).max() / np.abs(exact).max() < 2e-6   # (the randn bound of test_gemm_bf16x3.py)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), arm


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYOUTS)
def test_an_inf_in_a_corner_raises_the_flag_under_k_tile_major_planes(lib, on_gpu, mdopt, eager, lay):
    """An inf in the first or the last element of either operand, under planes 1 (both split kernels, by the layout): the flag is
    raised and the fp32 kernels' result comes out, the inf / NaN pattern and the finite values of option 0 bit for bit; the next
    finite product runs on the planes again."""
    assert on_gpu
    nd = eager
    rng = np.random.default_rng(53)
    M, K, N = 512, 96, 256
    A, B = rng.standard_normal((M, K), dtype=np.float32), rng.standard_normal((K, N), dtype=np.float32)
    a, b = _operands(nd, A, B, lay)
    mdopt("gemm_bf16x3", 2)
    finite = _product(lib, mdopt, nd, a, b, PARENT, "finite")
    for band in (1, 0):
        for side in "ab":
            for first in (True, False):
                what = (lay, band, side, first)
                A2, B2 = A.copy(), B.copy()
                if side == "a":
                    A2[(0, 0) if first else (M - 1, K - 1)] = np.inf      # [row, k] of A
                else:
                    B2[(0, 0) if first else (K - 1, N - 1)] = np.inf      # B is K x N: [k, row] of its plane rows
                a2, b2 = _operands(nd, A2, B2, lay)
                mdopt("gemm_bf16x3", 0)
                ref = nd.matmul(a2, b2).get()
                assert not np.isfinite(ref).all(), what
                mdopt("gemm_bf16x3", 2)
                got = _product(lib, mdopt, nd, a2, b2, (1, band, 1), what)
                assert np.array_equal(np.isnan(got), np.isnan(ref)), what
                assert np.array_equal(got.view(np.uint32)[~np.isnan(ref)], ref.view(np.uint32)[~np.isnan(ref)]), what
                # the flag does not stick
                again = _product(lib, mdopt, nd, a, b, (1, band, 1), what)
                assert np.array_equal(again.view(np.uint32), finite.view(np.uint32)), what
