// gemm_bf16x3.hip — a float32 product as six bfloat16 products of pre-split planes, accumulated in float32.
//
// What it computes. Every float32 operand element splits EXACTLY into three bfloat16 planes x = p1 + p2 + p3 (md_bf16x3.h). Of
// the nine plane products the six with i + j <= 4 — a1b1, a1b2, a2b1, a1b3, a2b2, a3b1, in that order (BX_PA / BX_PB) — are
// formed on the bf16 matrix cores; the three dropped ones are below 2^-23 |a||b|. The plane products themselves are exact (8 x 8
// significand bits), so integer operands whose sums stay below 2^24 and products with an identity come out exact. The matrix
// instruction's float32 accumulation TRUNCATES, so a k-tile (32 k) is summed in a fresh accumulator and the k-tiles' sums are
// added with VALU adds, round to nearest (bx_mma). Planned by gemm.hip (plan_bf16x3): split A, split B, the product, and behind
// it the fp32 kernel that runs instead when a split saw an inf or a NaN (the flag word).
//
// Plane image (md_bf16x3_layout.h; option gemm_bf16x3_planes, chosen by plan_bf16x3 for the split passes and the product alike):
// k-tile-major [K / 32][rows][64 B] by default — the 32 k of one k-tile of one row are 64 contiguous bytes and the rows of a
// k-tile follow each other, so one 1-KiB DMA piece (16 rows) is eight whole 128-B lines that no other k-tile shares — or
// [rows][K] (0), where the same piece is 16 half-used lines 2 K bytes apart. One addressing serves both: rows `rs` bytes apart,
// k-tiles `a_kstep` / `b_kstep` bytes apart (64 B x the operand's rows under the default: A and B step differently).
// Tile walk (md_bf16x3_tile; option gemm_bf16x3_band): an XCD's blocks take consecutive tiles of a grouped order with bands of
// gm tile rows (band 0, the default: gm chosen from the CU count); gm = 1 is the row-major walk.
//
// Split pass (one per operand, streaming): reads the float32 operand once and writes its planes in the plan's image whatever the
// operand's layout — BX_SPLIT_ROWS ([rows][K]) / BX_SPLIT_ROWS_KT (k-tile-major) for an operand whose k axis is contiguous,
// BX_SPLIT_COLS (64 rows x 32 k patches transposed through LDS) for one that is contiguous along its rows (A of TN, B of NN, both
// of TT). 16-B loads and stores. A block that saw a non-finite element ORs 1 into the flag word (an ordinary vector atomic).
// Each pass is written once over the plane count NP: k_bf16x3_split_* are the three TRUNCATED planes of the six-product kernel,
// k_bf16xp_split_*<NP> the NP = 2 / 1 ROUNDED planes of the reduced kernels.
//
// Product kernel k_gemm_bf16x3: block tile 256 x 128, eight waves 4 x 2 (wave tile 64 x 64), k-tile 32 = 64-B rows: six plane
// tiles (3 x 256 + 3 x 128 rows) = 72 KiB per k-tile, two buffers = 144 KiB of the 160 KiB LDS, one block per CU and two waves per
// SIMD. Each plane tile is staged ONCE per k-tile (global_load_lds_dwordx4: scalar base + 32-bit lane offset, a 1-KiB piece = 16
// rows per wave instruction, nine pieces per wave and k-tile) and serves all its products: 24 ds_read_b128 and 48 MFMAs (96 on the
// 16x16x32 shape) per wave and k-tile, 64 adds per wave to fold a k-tile's sum into the running sum.
// LDS image (as gemm_narrow.hip's KC image, for 64-B rows): [row][64 B], 16-B chunk c of row r in slot c ^ ((r >> 2) & 3),
// swizzled through the per-lane SOURCE address of the DMA (bx_lane_off); the 16 lanes of a 32-row read group hit 16 distinct bank
// slots. Loop 3 reads 16-row operands, which are 2-way on that image, and has a swizzle of its own: slot c ^ h((r >> 2) & 3) with
// h = 0, 2, 3, 1 (bx3_swz). The buffers are separate __shared__ objects and every k loop is unrolled by two.
//
// Four k loops in one build (template argument LOOP, option gemm_bf16x3_loop). Loops 0 - 2 agree bit for bit; loop 3 has bits
// of its own under the same contract.
//   0  bx_stage / bx_mma under BX_LOOP0: all nine DMAs in front of the k-tile's reads, their addresses formed anew per k-tile,
//      the fold behind the last MFMA, one __syncthreads() per k-tile. The loop the kernel was first measured with.
//   1  bx_tile: the piece bases formed once, the k-tile's program order written out, every MFMA behind a scheduling fence with
//      what issues in its shadow (a DMA, two reads, four adds); one __syncthreads() per k-tile.
//   2  bx2_tile: the two halves of the block one segment apart, so that on every SIMD one wave issues MFMAs while its partner
//      reads, stages and folds; four raw barriers per k-tile.
//   3  bx3_tile under bx3_run, THE DEFAULT: loop 2 on v_mfma_f32_16x16x32_bf16 (SIX truncating accumulations of 32 terms per
//      k-tile and element where the others take twelve of 16), the wave tile as two 32 x 64 halves, 240 VGPRs against 252.
// What loops 1 - 3 share stands once: the piece bases (BX_BASES), bx_dma_n, the fold (bx_fold4), the twelve-read order
// (bx_read12) and the driver (BX_PAIRS_AND_TAIL). The barrier and counter invariants of a loop (WAR / RAW by slot count) stand
// in front of its tile body; whoever moves a DMA, a wait or a barrier re-derives them there. tests/test_isa_bf16x3.py and the
// ISA halves of tests/test_gemm_bf16x3_loop2.py / _loop3.py pin what the compiler makes of loops 1 - 3.
// What stands in a kernel's own body — tile origin, zeroing, stamps, bases, drivers, write-out — is a MACRO: as inlined functions
// each of them changed the machine code of some kernel (another register assignment or scalar prologue), and this file's speed
// hangs on that; expanded in place the text compiles to what the copies it replaced compiled to (scripts/isa_diff.py,
// profiles/gemm_bf16x3_one_copy_isa.txt). What runs inside a tile body is a function.
//
// Reduced products (option gemm_products 3 / 1 = ndarray.set_matmul_precision "high" / "medium"; the default 6 is everything
// above). The product list is ordered so that its prefixes are the cheaper forms: k_gemm_bf16xp<3> forms a1b1 + a1b2 + a2b1 over
// two planes per operand, k_gemm_bf16xp<1> a1b1 over one. Their planes are ROUNDED (md_bf16x3_split_rn: p1 = RN(x), p2 =
// RN(x - p1)), not truncated: a truncated plane leans every term towards zero. Their split passes write only the planes in use,
// same images (4 + 2 NP bytes per operand element instead of 10), and also raise the flag for a finite element that rounds up to
// inf. The kernels are loop 0 over the plane count and the product prefix, with its tile, swizzle, tile walk, flag word and
// write-out, and only the LDS they use (96 / 48 KiB). Contract, against float64 with mass = |a| @ |b| and u8 = 2^-8: medium
// (2 u8 + u8^2) mass, high (3 u8^2 + 2^-23) mass, plus the accumulation term (2 NPROD 2^-23 + K / 32 x 2^-24) mass; integer
// operands whose sums stay below 2^24 give the integer product of the rounded planes exactly (tests/test_matmul_precision.py). A
// permission, not a promise: what plan_bf16x3 does not take runs as under 6.
//
// Fixed order. Whole tiles only. The k order and the product order are fixed: an output element's bits do not depend on M, N,
// the plane image, the tile walk or where its tile lies. No float atomics.
// How each loop, image and walk was arrived at, what was built and dropped, and every measured figure: DESIGN.md ("Above the
// floors: six bf16 products of pre-split planes") with its files under profiles/.
#include "md_hip.h"
#include "md_bf16x3.h"
#include "md_bf16x3_layout.h"

namespace {

typedef __attribute__((address_space(3))) void bx_lds_void;
typedef __attribute__((address_space(1))) const void bx_gbl_void;
typedef __bf16 bx_bf16x8 __attribute__((ext_vector_type(8)));
typedef int bx_i32x4 __attribute__((ext_vector_type(4)));
typedef float bx_f32x4 __attribute__((ext_vector_type(4)));
typedef float bx_f32x16 __attribute__((ext_vector_type(16)));

constexpr int BX_BM = 256, BX_BN = 128, BX_BK = 32;   // block tile; BX_BK bfloat16 = 64 B per row and k-tile
constexpr int BX_NT = 512;                            // threads (eight waves)
constexpr int BX_ROWB = BX_BK * 2;                    // bytes of a row in the LDS image

// ---- split pass ------------------------------------------------------------------------------------------------------------------
// eight consecutive k of one row -> 16 B of each of NP planes. NP = 3: the exact truncating split (md_bf16x3_split); NP = 2 / 1:
// the rounding split of the reduced products (md_bf16x3_split_rn), where `bad` also rises for a finite element that rounds to inf.
// (The two flavours keep their own temporaries, scalars and an array: with one form for both, one of them compiled differently.)
template <int NP>
__device__ __forceinline__ bool bx_split8(const float (&x)[8], bx_i32x4 *q1, bx_i32x4 *q2, bx_i32x4 *q3) {
  bool bad = false;
  uint32_t h[NP][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if constexpr (NP == 3) {
      uint32_t p1, p2, p3;
      bad |= md_bf16x3_split(x[j], &p1, &p2, &p3);
      h[0][j] = p1 >> 16; h[1][j] = p2 >> 16; h[2][j] = p3 >> 16;
    } else {
      uint32_t p[2];
      bad |= md_bf16x3_split_rn(x[j], NP, &p[0], &p[1]);
#pragma unroll
      for (int i = 0; i < NP; ++i) h[i][j] = p[i] >> 16;
    }
  }
  bx_i32x4 *q[3] = {q1, q2, q3};
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int w = 0; w < 4; ++w) (*q[p])[w] = (int)(h[p][2 * w] | (h[p][2 * w + 1] << 16));
  return bad;
}
// the first NP of them to d, `plane` BYTES apart
template <int NP>
__device__ __forceinline__ void bx_put(char *d, int64_t plane, const bx_i32x4 &q1, const bx_i32x4 &q2, const bx_i32x4 &q3) {
  *(bx_i32x4 *)d = q1;
  if (NP > 1) *(bx_i32x4 *)(d + plane) = q2;
  if (NP > 2) *(bx_i32x4 *)(d + 2 * plane) = q3;
}

// The three passes, each written once over the plane count; the nine kernels below are their instantiations. (Macros: as inlined
// functions the bodies came out with another register assignment in eight of the nine.)
// src: rows x K float32, k unit-stride, `rs` floats between rows. dst: NP planes of rows x K bfloat16 in layout 0 ([rows][K]),
// `plane` BYTES apart.
#define BX_SPLIT_ROWS(NP)                                                                                        \
  bool bad = false;                                                                                              \
  const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;                                               \
  if (k < K) {                                                                                                   \
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {                                                     \
      const bx_f32x4 lo = *(const bx_f32x4 *)(src + r * rs + k), hi = *(const bx_f32x4 *)(src + r * rs + k + 4); \
      const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                               \
      bx_i32x4 q1, q2, q3;                                                                                       \
      bad |= bx_split8<NP>(x, &q1, &q2, &q3);                                                                    \
      bx_put<NP>(dst + md_bf16x3_plane_off(r, k, K * 2, 64), plane, q1, q2, q3);                                 \
    }                                                                                                            \
  }                                                                                                              \
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1u);
// The same pass into layout 1 ([K / 32][rows][64 B]), where a k-tile's 64 B of one row are followed by the next ROW's: a wave takes
// two adjacent rows (rows is even: a multiple of the block tile) x eight k-tiles — lane l row 2 j + ((l >> 2) & 1), k-tile l >> 3,
// 16-B chunk l & 3 — so that eight lanes store one whole 128-B line and the lanes of one row still load 1 KiB of it in a piece.
#define BX_SPLIT_ROWS_KT(NP)                                                                                     \
  bool bad = false;                                                                                              \
  const int l = threadIdx.x & 63, w = threadIdx.x >> 6;                                                          \
  const int64_t k = (((int64_t)blockIdx.x * 4 + w) * 8 + (l >> 3)) * 32 + (l & 3) * 8;                           \
  if (k < K) {                                                                                                   \
    for (int64_t r = (int64_t)blockIdx.y * 2 + ((l >> 2) & 1); r < rows; r += (int64_t)gridDim.y * 2) {          \
      const bx_f32x4 lo = *(const bx_f32x4 *)(src + r * rs + k), hi = *(const bx_f32x4 *)(src + r * rs + k + 4); \
      const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                               \
      bx_i32x4 q1, q2, q3;                                                                                       \
      bad |= bx_split8<NP>(x, &q1, &q2, &q3);                                                                    \
      bx_put<NP>(dst + md_bf16x3_plane_off(r, k, 64, rows * 64), plane, q1, q2, q3);                             \
    }                                                                                                            \
  }                                                                                                              \
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(flag, 1u);
// src: K x rows float32, the rows unit-stride, `ks` floats between k-rows. One block: 64 rows x 32 k, stored at `prs` bytes between
// rows and `pks` between k-tiles (either layout; under layout 1 the block's 4 KiB per plane are contiguous).
#define BX_SPLIT_COLS(NP)                                                                                        \
  __shared__ float T[32][66]; /* [k][row]; 66: the transposed reads below hit 64 distinct banks */               \
  const int t = threadIdx.x;                                                                                     \
  for (int64_t kb = blockIdx.y; kb < K / 32; kb += gridDim.y) {                                                  \
    const int64_t r0 = (int64_t)blockIdx.x * 64, k0 = kb * 32;                                                   \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                              \
      const int idx = t + 256 * i, kk = idx >> 4, r4 = (idx & 15) * 4;                                           \
      const bx_f32x4 v = *(const bx_f32x4 *)(src + (k0 + kk) * ks + r0 + r4);                                    \
      T[kk][r4] = v[0]; T[kk][r4 + 1] = v[1]; T[kk][r4 + 2] = v[2]; T[kk][r4 + 3] = v[3];                        \
    }                                                                                                            \
    __syncthreads();                                                                                             \
    const int kg = t & 3, r = t >> 2;                                                                            \
    float x[8];                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) x[j] = T[kg * 8 + j][r];                                       \
    bx_i32x4 q1, q2, q3;                                                                                         \
    const bool bad = bx_split8<NP>(x, &q1, &q2, &q3);                                                            \
    bx_put<NP>(dst + md_bf16x3_plane_off(r0 + r, k0 + kg * 8, prs, pks), plane, q1, q2, q3);                     \
    if (__syncthreads_or(bad) && t == 0) atomicOr(flag, 1u); /* (also: every lane is done with T) */             \
  }

#define BX_SPLIT_ROWS_ARGS const float *__restrict__ src, int64_t rows, int64_t K, int64_t rs, char *__restrict__ dst, int64_t plane, unsigned *flag
#define BX_SPLIT_COLS_ARGS \
  const float *__restrict__ src, int64_t rows, int64_t K, int64_t ks, char *__restrict__ dst, int64_t plane, int64_t prs, int64_t pks, unsigned *flag
// three planes, truncated: the six-product kernel's
__global__ void __launch_bounds__(256) k_bf16x3_split_rows(BX_SPLIT_ROWS_ARGS) { BX_SPLIT_ROWS(3) }
__global__ void __launch_bounds__(256) k_bf16x3_split_rows_kt(BX_SPLIT_ROWS_ARGS) { BX_SPLIT_ROWS_KT(3) }
__global__ void __launch_bounds__(256) k_bf16x3_split_cols(BX_SPLIT_COLS_ARGS) { BX_SPLIT_COLS(3) }
// NP = 2 / 1 planes, rounded: the reduced products' (option gemm_products 3 / 1); the same images, grids and flag word
template <int NP> __global__ void __launch_bounds__(256) k_bf16xp_split_rows(BX_SPLIT_ROWS_ARGS) { BX_SPLIT_ROWS(NP) }
template <int NP> __global__ void __launch_bounds__(256) k_bf16xp_split_rows_kt(BX_SPLIT_ROWS_ARGS) { BX_SPLIT_ROWS_KT(NP) }
template <int NP> __global__ void __launch_bounds__(256) k_bf16xp_split_cols(BX_SPLIT_COLS_ARGS) { BX_SPLIT_COLS(NP) }

// ---- product: what the kernels share -------------------------------------------------------------------------------------------------
struct Bx3Args {
  const char *A, *B;        // plane 1 of each operand; planes 2 and 3 follow a_plane / b_plane BYTES apart
  float *C;
  int64_t K, c_ms;          // c_ms in floats
  int64_t a_plane, b_plane;
  int64_t rs, a_kstep, b_kstep;   // the plane images (md_bf16x3_layout.h): bytes between rows, and between k-tiles of A / of B
  int tiles_m, tiles_n, gm; // gm: band height of the tile walk (md_bf16x3_tile)
  const unsigned *flag;     // the split passes' verdict: a non-zero word = nothing to do here (the fp32 kernel behind runs instead)
  unsigned long long *stamp;   // diagnostic instantiation only (option gemm_stamp): per block {shader cycles, 100 MHz ticks} of its k loop
};
struct Bx3Bufs { char *a[3], *b[3]; };   // the plane tiles of one LDS buffer

// the products a1b1, a1b2, a2b1, a1b3, a2b2, a3b1 as plane indices of A / of B; the reduced kernels take the first 3 / 1
constexpr int BX_PA[6] = {0, 0, 1, 0, 1, 2}, BX_PB[6] = {0, 1, 0, 2, 1, 0};

// The block's tile: XCD-aware order, as gemm_narrow.hip (the blocks that share an XCD take a contiguous run of output tiles),
// then the banded walk. Declares m0, n0.
#define BX_ORIGIN(g, m0, n0)                                                                               \
  int64_t m0, n0;                                                                                          \
  {                                                                                                        \
    const int nwg = (g).tiles_m * (g).tiles_n, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7; \
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);                   \
    int tm, tn;                                                                                            \
    md_bf16x3_tile(wg, (g).tiles_m, (g).tiles_n, (g).gm, &tm, &tn);                                        \
    m0 = (int64_t)tm * BX_BM; n0 = (int64_t)tn * BX_BN;                                                    \
  }
// acc[I][J] of vectors of R floats = 0
#define BX_ZERO(acc, I, J, R)                       \
  _Pragma("unroll") for (int i = 0; i < (I); ++i)   \
    _Pragma("unroll") for (int j = 0; j < (J); ++j) \
      _Pragma("unroll") for (int e = 0; e < (R); ++e) acc[i][j][e] = 0;

// The per-lane source offset of a DMA piece (16 rows x 64 B, 1 KiB): lane l lands in LDS at piece + 16 l = row l >> 2, slot l & 3,
// so it fetches chunk (l & 3) ^ h of its row, h the image's swizzle of the row group (row >> 2) & 3 = (l >> 4) & 3.
__device__ __forceinline__ uint32_t bx_lane_off(int64_t rs, int l, int h) { return (uint32_t)((l >> 2) * rs + (((l & 3) ^ h) << 4)); }

// STAMP: the diagnostic instantiations (option gemm_stamp, never launched otherwise) read s_memtime / s_memrealtime before the
// first DMA and behind the last fold and write the differences to g.stamp, a buffer of their own that nothing else reads. The
// instantiations without it hold no stamp.
struct Bx3Stamp { unsigned long long c = 0, r = 0; };
#define BX_STAMP_BEGIN(STAMP, st)                                                                           \
  Bx3Stamp st;                                                                                              \
  if constexpr (STAMP) {                                                                                    \
    st.c = __builtin_amdgcn_s_memtime(); st.r = __builtin_amdgcn_s_memrealtime();                           \
    __builtin_amdgcn_s_waitcnt(0xC07F); /* (lgkmcnt(0) alone: the loop's counted LDS waits stay counted) */ \
  }
#define BX_STAMP_END(STAMP, g, st)                                             \
  if constexpr (STAMP) {                                                       \
    if (threadIdx.x == 0) {                                                    \
      (g).stamp[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st.c;         \
      (g).stamp[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st.r; \
    }                                                                          \
  }

// The write-out of the 32 x 32 accumulators (loops 0 - 2 and the reduced kernels). Accumulator element e of lane l: row (e & 3) +
// 8 (e >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 tile; one wave store writes 32 consecutive floats of two rows (whole 128-B
// lines), as k_gemm_widen_mfma
#define BX_WRITE_C(g, m0, n0, wm, wn, l, acc)                                                                                  \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                                \
    _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                              \
      _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                                         \
        const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (l >> 5), n = n0 + wn * 64 + j * 32 + (l & 31); \
        (g).C[m * (g).c_ms + n] = acc[i][j][e];                                                                                \
      }
// (the reduced kernels call it as a function, the six-product kernel expands it in its body: the other form changes the machine
// code of either)
__device__ __forceinline__ void bx_write_c(const Bx3Args &g, int64_t m0, int64_t n0, int wm, int wn, int l, const bx_f32x16 (&acc)[2][2]) {
  BX_WRITE_C(g, m0, n0, wm, wn, l, acc)
}

__device__ __forceinline__ const char *bx_uniform(const char *p) {
  uint32_t lo = (uint32_t)(uintptr_t)p, hi = (uint32_t)((uintptr_t)p >> 32);
  asm("" : "+s"(lo), "+s"(hi));
  return reinterpret_cast<const char *>(((uintptr_t)hi << 32) | lo);
}

// ---- loop 0 (and the reduced kernels) ---------------------------------------------------------------------------------------------
// One piece of a plane tile, its address formed anew: P + row rs + kt kstep, and the lane's offset (bx_lane_off).
__device__ __forceinline__ void bx_piece(const char *P, int64_t rs, int64_t row, int64_t kstep, int kt, uint32_t lane_off, char *S) {
  uint32_t off = lane_off;
  asm("" : "+v"(off) : "s"(kt));
  const char *src = bx_uniform(P + row * rs + kt * kstep) + off;
  __builtin_amdgcn_global_load_lds((bx_gbl_void *)src, (bx_lds_void *)S, 16, 0, 0);
}

// the NP plane tiles of k-tile kt (NP = 3: the six-product kernel; 2 / 1: the reduced ones)
template <int NP>
__device__ __forceinline__ void bx_stage(const Bx3Args &g, int64_t m0, int64_t n0, int kt, const Bx3Bufs &S, uint32_t lane_off) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
#pragma unroll
    for (int i = 0; i < 2; ++i) bx_piece(g.A + p * g.a_plane, g.rs, m0 + 16 * (wave + 8 * i), g.a_kstep, kt, lane_off, S.a[p] + (wave + 8 * i) * 1024);
    bx_piece(g.B + p * g.b_plane, g.rs, n0 + 16 * wave, g.b_kstep, kt, lane_off, S.b[p] + wave * 1024);
  }
}

// the MFMA operand of lane l for k16 step s (0, 1) and the 32 rows from rb: row rb + (l & 31), k 16 s + 8 (l >> 5) ..
__device__ __forceinline__ bx_bf16x8 bx_frag(const char *S, int rb, int s) {
  const int l = threadIdx.x & 63, r = rb + (l & 31), c = 2 * s + (l >> 5);
  return __builtin_bit_cast(bx_bf16x8, *(const bx_i32x4 *)(S + r * BX_ROWB + ((c ^ ((r >> 2) & 3)) << 4)));
}

// One k-tile. The matrix instruction's float32 accumulation TRUNCATES (measured: all-positive operands came out low by 2e-9 K of their
// value with one accumulator over all of K), so the k-tile's 12 accumulations per element start from zero in a fresh accumulator and
// the k-tile's sum is folded into the running sum with VALU adds (round to nearest), outside the k16 steps: the bias is that of 12
// truncations whatever K is. The chunk is the k-tile, so the bits of an element still depend on k alone.
// NPROD: the first 6 / 3 / 1 products of the list over NP = 3 / 2 / 1 planes (2 NPROD accumulations per k-tile).
template <int NP, int NPROD>
__device__ __forceinline__ void bx_mma(const Bx3Bufs &S, int wm, int wn, bx_f32x16 (&acc)[2][2]) {
  bx_f32x16 part[2][2];
  BX_ZERO(part, 2, 2, 16)
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bx_bf16x8 a[NP][2], b[NP][2];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[p][i] = bx_frag(S.a[p], wm * 64 + i * 32, s);
        b[p][i] = bx_frag(S.b[p], wn * 64 + i * 32, s);
      }
    // each product over the four sub-tiles, so that consecutive MFMAs write different accumulators
#pragma unroll
    for (int q = 0; q < NPROD; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[BX_PA[q]][i], b[BX_PB[q]][j], part[i][j], 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
}

// Loop 0's driver, two buffers: behind each __syncthreads() tile kt is in its buffer (the barrier's vmcnt(0) retires the DMAs) and
// every wave is done with the other one, which the next tile's DMAs then fill while this one is multiplied. Uses g, S0, S1, m0, n0,
// nk, lane_off, wm, wn and acc of the kernel it stands in.
#define BX_LOOP0(NP, NPROD)                                         \
  bx_stage<NP>(g, m0, n0, 0, S0, lane_off);                         \
  for (int kt = 0; kt < nk; kt += 2) {                              \
    __syncthreads();                                                \
    if (kt + 1 < nk) bx_stage<NP>(g, m0, n0, kt + 1, S1, lane_off); \
    bx_mma<NP, NPROD>(S0, wm, wn, acc);                             \
    if (kt + 1 >= nk) break;                                        \
    __syncthreads();                                                \
    if (kt + 2 < nk) bx_stage<NP>(g, m0, n0, kt + 2, S0, lane_off); \
    bx_mma<NP, NPROD>(S1, wm, wn, acc);                             \
  }

// ---- what loops 1 - 3 share --------------------------------------------------------------------------------------------------------
// The nine wave-uniform piece bases of a wave are formed ONCE; a DMA adds the k offset with scalar adds, no multiply.
struct Bx3Src { const char *a[3][2], *b[3]; };   // piece bases of the k-tile staged last, in SGPRs
struct Bx3Dst { char *a[3][2], *b[3]; };         // and where they land
// Declares rs, ka, kb, the bases `src` of tile 0 and the destinations d0 / d1 in buffers S0 / S1, for wave uw (in an SGPR).
#define BX_BASES(g, S0, S1, m0, n0, uw, src, d0, d1)                                     \
  const int64_t rs = (g).rs, ka = (g).a_kstep, kb = (g).b_kstep;                         \
  Bx3Src src;                                                                            \
  Bx3Dst d0, d1;                                                                         \
  _Pragma("unroll") for (int p = 0; p < 3; ++p) {                                        \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                      \
      src.a[p][i] = bx_uniform((g).A + p * (g).a_plane + (m0 + 16 * (uw + 8 * i)) * rs); \
      d0.a[p][i] = S0.a[p] + (uw + 8 * i) * 1024;                                        \
      d1.a[p][i] = S1.a[p] + (uw + 8 * i) * 1024;                                        \
    }                                                                                    \
    src.b[p] = bx_uniform((g).B + p * (g).b_plane + (n0 + 16 * uw) * rs);                \
    d0.b[p] = S0.b[p] + uw * 1024;                                                       \
    d1.b[p] = S1.b[p] + uw * 1024;                                                       \
  }

__device__ __forceinline__ void bx_fence() { __builtin_amdgcn_sched_barrier(0); }

// The piece base steps to the next k-tile (a 64-bit scalar add: the step is 64 B under layout 0, 64 B x the operand's rows under
// layout 1, which fits no 32-bit offset) and the piece is fetched from there.
__device__ __forceinline__ void bx_dma(const char *&base, int64_t step, uint32_t lane_off, char *S) {
  base = bx_uniform(base + step);
  uint32_t off = lane_off;
  asm("" : "+v"(off));
  __builtin_amdgcn_global_load_lds((bx_gbl_void *)(base + off), (bx_lds_void *)S, 16, 0, 0);
}

// piece n (0 .. 8) of the next tile; ka / kb: the k step of A's / of B's pieces (0, 0: of tile 0, from the bases as they stand)
__device__ __forceinline__ void bx_dma_n(Bx3Src &src, const Bx3Dst &dst, int n, int64_t ka, int64_t kb, uint32_t lane_off) {
  const int p = n / 3, i = n % 3;
  if (i < 2) bx_dma(src.a[p][i], ka, lane_off, dst.a[p][i]);
  else bx_dma(src.b[p], kb, lane_off, dst.b[p]);
}

// acc[e0 .. e0 + 4) += part[e0 .. e0 + 4) as four scalar adds, pinned where they stand: the empty statement holds the four sums, so
// that the adds neither move nor pair up into packed ones (measured slower beside MFMAs: DESIGN.md)
__device__ __forceinline__ void bx_fold4(bx_f32x16 &acc, const bx_f32x16 &part, int e0) {
  float r0 = acc[e0] + part[e0], r1 = acc[e0 + 1] + part[e0 + 1], r2 = acc[e0 + 2] + part[e0 + 2], r3 = acc[e0 + 3] + part[e0 + 3];
  asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));
  acc[e0] = r0; acc[e0 + 1] = r1; acc[e0 + 2] = r2; acc[e0 + 3] = r3;
}

// the operand of bx_frag from the lane's offset (bx_read_off) and the half (0, 1: rows 0 .. 31, 32 .. 63 of the wave's 64)
__device__ __forceinline__ bx_bf16x8 bx_frag_at(const char *S, uint32_t off, int half) {
  return __builtin_bit_cast(bx_bf16x8, *(const bx_i32x4 *)(S + off + half * 32 * BX_ROWB));
}
__device__ __forceinline__ uint32_t bx_read_off(int rb, int s) {
  const int l = threadIdx.x & 63, r = rb + (l & 31), c = 2 * s + (l >> 5);
  return (uint32_t)(r * BX_ROWB + ((c ^ ((r >> 2) & 3)) << 4));
}
// A k16 step's twelve fragments (loops 1 and 2) in the order the products a1b1, a1b2, a2b1, a1b3, (a2b2,) a3b1 first need them, so
// that the waits the compiler inserts are counted (the first MFMA waits for three reads, not twelve)
__device__ __forceinline__ void bx_read12(const Bx3Bufs &S, uint32_t ra, uint32_t rb, bx_bf16x8 (&a)[3][2], bx_bf16x8 (&b)[3][2]) {
  a[0][0] = bx_frag_at(S.a[0], ra, 0); b[0][0] = bx_frag_at(S.b[0], rb, 0); b[0][1] = bx_frag_at(S.b[0], rb, 1); a[0][1] = bx_frag_at(S.a[0], ra, 1);
  b[1][0] = bx_frag_at(S.b[1], rb, 0); b[1][1] = bx_frag_at(S.b[1], rb, 1);
  a[1][0] = bx_frag_at(S.a[1], ra, 0); a[1][1] = bx_frag_at(S.a[1], ra, 1);
  b[2][0] = bx_frag_at(S.b[2], rb, 0); b[2][1] = bx_frag_at(S.b[2], rb, 1);
  a[2][0] = bx_frag_at(S.a[2], ra, 0); a[2][1] = bx_frag_at(S.a[2], ra, 1);
}

// The ping-pong driver of loops 1 - 3 over a tile body TILE<STAGE>(buffer, src, where the NEXT tile lands, ..., rd, acc, SUM): whole
// pairs with a tile behind them, so that every tile of the loop stages the next one, then one or two tail tiles, the last of which
// stages nothing. SYNC stands in front of every tile (loop 1: __syncthreads(); loops 2 and 3: nothing, their barriers are in the
// tile body). Uses nk, S0, S1, src, d0, d1, ka, kb, lane_off, rd and acc of the scope it stands in.
#define BX_PAIRS_AND_TAIL(SYNC, TILE, SUM)                   \
  int kt = 0;                                                \
  for (; kt + 2 < nk; kt += 2) {                             \
    SYNC;                                                    \
    TILE<true>(S0, src, d1, ka, kb, lane_off, rd, acc, SUM); \
    SYNC;                                                    \
    TILE<true>(S1, src, d0, ka, kb, lane_off, rd, acc, SUM); \
  }                                                          \
  SYNC;                                                      \
  if (kt + 1 < nk) {                                         \
    TILE<true>(S0, src, d1, ka, kb, lane_off, rd, acc, SUM); \
    SYNC;                                                    \
    TILE<false>(S1, src, d0, 0, 0, lane_off, rd, acc, SUM);  \
  } else {                                                   \
    TILE<false>(S0, src, d1, 0, 0, lane_off, rd, acc, SUM);  \
  }

// ---- loop 1 ----------------------------------------------------------------------------------------------------------------------
// The arithmetic of bx_mma per output element — 12 accumulations per k-tile in the same order into a fresh accumulator, one
// round-to-nearest add into the running sum — with everything that is not an MFMA placed under the MFMAs:
//   * a k-tile's program order is written out and pinned with fences (bx_fence). Step 0 runs product by product as bx_mma does;
//     behind its MFMAs 0 .. 3 the carried sum's adds, behind 4 .. 12 the next tile's DMAs, behind 12 .. 17 step 1's reads. Step 1
//     runs sub-tile by sub-tile (six dependent MFMAs each, which cost no throughput); the 16 adds of a finished sub-tile go behind
//     MFMAs 2 .. 5 of the next, and the last sub-tile's sum is carried over the barrier;
//   * the compiler counts no LDS read past a pending DMA (its waits turn into lgkmcnt(0)), so the one full wait is taken by hand
//     behind the last DMA, where step 0's reads are long back, and step 1's reads, issued behind it, are seven MFMAs old at theirs;
//   * WAR / RAW: the __syncthreads() in front of a tile retires this wave's DMAs of it (vmcnt(0)) and ends every wave's reads of the
//     other buffer, into which this tile's DMAs go.
// One k-tile of loop 1: 48 MFMAs, each behind a fence with what issues in its shadow.
template <bool STAGE>
__device__ __forceinline__ void bx_tile(const Bx3Bufs &S, Bx3Src &src, const Bx3Dst &dst, int64_t ka, int64_t kb, uint32_t lane_off, const uint32_t (&rd)[4],
                                        bx_f32x16 (&acc)[2][2], bx_f32x16 &carry) {
  bx_f32x16 part[2][2];
  bx_bf16x8 a0[3][2], b0[3][2], a1[3][2], b1[3][2];
  // the lane's read offsets (A step 0 / 1, B step 0 / 1), opaque per tile: the twelve plane addresses of a tile are then one add each
  // here, not two dozen registers held over the loop
  uint32_t ra0 = rd[0], ra1 = rd[1], rb0 = rd[2], rb1 = rd[3];
  asm volatile("" : "+v"(ra0), "+v"(ra1), "+v"(rb0), "+v"(rb1));
  bx_read12(S, ra0, rb0, a0, b0);
  bx_fence();
  // step 0: product-major as bx_mma. Under it: the carried sum (MFMAs 0 .. 3), step 1's fragments in the order its sub-tiles need them
  // (two reads behind each of MFMAs 12 .. 17: the last is seven MFMAs old when step 1 starts)
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int n = q * 4 + i * 2 + j;
        if (q == 0) {
          const bx_f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
          part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[0][i], b0[0][j], zero, 0, 0, 0);
        } else {
          part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0[BX_PA[q]][i], b0[BX_PB[q]][j], part[i][j], 0, 0, 0);
        }
        if (n < 4) bx_fold4(acc[1][1], carry, 4 * n);
        if (n >= 4 && n <= 12) {   // the next tile's nine pieces, one behind each of MFMAs 4 .. 12
          if (STAGE) bx_dma_n(src, dst, n - 4, ka, kb, lane_off);
          // The compiler counts no fragment read past a pending DMA: every wait behind one is lgkmcnt(0). Taken here, where step 0's
          // reads are a dozen MFMAs old, it is free, and the waits on step 1's reads behind it are counted again.
          if (n == 12) __builtin_amdgcn_s_waitcnt(0xC07F);
        }
        switch (n) {
          case 12: a1[0][0] = bx_frag_at(S.a[0], ra1, 0); b1[0][0] = bx_frag_at(S.b[0], rb1, 0); break;
          case 13: b1[1][0] = bx_frag_at(S.b[1], rb1, 0); a1[1][0] = bx_frag_at(S.a[1], ra1, 0); break;
          case 14: b1[2][0] = bx_frag_at(S.b[2], rb1, 0); a1[2][0] = bx_frag_at(S.a[2], ra1, 0); break;
          case 15: b1[0][1] = bx_frag_at(S.b[0], rb1, 1); b1[1][1] = bx_frag_at(S.b[1], rb1, 1); break;
          case 16: b1[2][1] = bx_frag_at(S.b[2], rb1, 1); a1[0][1] = bx_frag_at(S.a[0], ra1, 1); break;
          case 17: a1[1][1] = bx_frag_at(S.a[1], ra1, 1); a1[2][1] = bx_frag_at(S.a[2], ra1, 1); break;
          default: break;
        }
        bx_fence();
      }
  // step 1: sub-tile by sub-tile; a sub-tile's 16 adds go under MFMAs 2 .. 5 of the next one (its last result is two MFMAs old by then)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = t >> 1, j = t & 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1[BX_PA[q]][i], b1[BX_PB[q]][j], part[i][j], 0, 0, 0);
      if (t > 0 && q >= 2) bx_fold4(acc[(t - 1) >> 1][(t - 1) & 1], part[(t - 1) >> 1][(t - 1) & 1], 4 * (q - 2));
      bx_fence();
    }
  }
  carry = part[1][1];
}

// ---- loop 2 ----------------------------------------------------------------------------------------------------------------------
// The two halves of the block (waves 0 .. 3 and 4 .. 7: one wave of each per SIMD) run one segment apart. A k-tile is two k16 steps,
// a step two segments: L — the step's 12 fragment reads, the wave's share of the next tile's DMAs and, in step 0, the fold of the
// tile before — and C — its 24 MFMAs and nothing else. Every segment ends in a raw s_barrier (no fence: DMAs are in flight across
// it); half 1 takes ONE barrier more in front of the loop and half 0 one behind it, so that in every slot each SIMD has one wave in
// C and its partner in L, and both halves execute 4 nk + 1 barriers behind the prologue's. The arithmetic per output element is
// bx_mma's: 12 accumulations per k-tile in the same order into a fresh accumulator, one round-to-nearest add into the running sum.
// By count, with slots numbered so that half 0 runs L(j) in slot 2 j and C(j) in 2 j + 1, half 1 one slot later (j = 2 kt + s):
//   WAR  the last read of tile kt - 1's buffer is half 1's L(2 kt - 1) in slot 4 kt - 1, retired by the lgkmcnt(0) in front of that
//        slot's barrier; the DMAs of tile kt + 1 into that buffer issue in L(2 kt) and L(2 kt + 1), from slot 4 kt on;
//   RAW  every wave takes vmcnt(0) at the end of its L(2 kt + 1) — slot 4 kt + 2 for half 0, 4 kt + 3 for half 1 — in front of the
//        barrier; tile kt + 1 is first read in half 0's L(2 kt + 2), slot 4 kt + 4, behind the barrier that ends slot 4 kt + 3.
// The barrier: the instruction between two scheduling fences and two compiler memory fences (no instruction of their own), so
// that neither a fragment read nor an MFMA changes its segment.
__device__ __forceinline__ void bx2_barrier() {
  bx_fence();
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  bx_fence();
}

// One k-tile of loop 2: L(2 kt) B C(2 kt) B L(2 kt + 1) B C(2 kt + 1) B. part: the sum of the tile before on entry (folded in
// L(2 kt), before C(2 kt) starts it afresh from a zero C operand), this tile's on return. The nine pieces of the next tile: three
// behind L(2 kt)'s reads and six between the MFMAs of C(2 kt), one behind every fourth — none in L(2 kt + 1), whose vmcnt(0) then
// waits for pieces that are a segment old or older (with pieces in both L segments and none in C the loop LOST to loop 1:
// DESIGN.md).
template <bool STAGE>
__device__ __forceinline__ void bx2_tile(const Bx3Bufs &S, Bx3Src &src, const Bx3Dst &dst, int64_t ka, int64_t kb, uint32_t lane_off, const uint32_t (&rd)[4],
                                         bx_f32x16 (&acc)[2][2], bx_f32x16 (&part)[2][2]) {
  constexpr int NL = 3, CSTEP = 4;   // pieces in L(2 kt); one piece behind every CSTEP-th MFMA of C(2 kt), from its second
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    // L: one step's fragments live at a time (48 registers)
    bx_bf16x8 a[3][2], b[3][2];
    uint32_t ra = rd[s], rb = rd[2 + s];
    asm volatile("" : "+v"(ra), "+v"(rb));
    bx_read12(S, ra, rb, a, b);
    bx_fence();
    if (s == 0) {
      if (STAGE) {
#pragma unroll
        for (int n = 0; n < NL; ++n) bx_dma_n(src, dst, n, ka, kb, lane_off);
      }
      bx_fence();
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 16; e += 4) bx_fold4(acc[t >> 1][t & 1], part[t >> 1][t & 1], e);
      bx_fence();
    }
    // step 0: the reads are back before the barrier (WAR, and C holds no wait). Step 1: and so are this wave's nine pieces (RAW)
    if (s == 0) __builtin_amdgcn_s_waitcnt(0xC07F);
    else __builtin_amdgcn_s_waitcnt(0x0070);
    bx2_barrier();
    // C: product-major, consecutive MFMAs write different accumulators; every MFMA behind a fence, as in loop 1
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int n = q * 4 + i * 2 + j;
          if (s == 0 && q == 0) {
            const bx_f32x16 zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0][i], b[0][j], zero, 0, 0, 0);
          } else {
            part[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[BX_PA[q]][i], b[BX_PB[q]][j], part[i][j], 0, 0, 0);
          }
          if (STAGE && s == 0 && n % CSTEP == 1 && NL + n / CSTEP < 9) bx_dma_n(src, dst, NL + n / CSTEP, ka, kb, lane_off);
          bx_fence();
        }
    bx2_barrier();
  }
}

// ---- loop 3 ----------------------------------------------------------------------------------------------------------------------
// Loop 2's halves and barriers on v_mfma_f32_16x16x32_bf16: one instruction covers the k-tile (K = 32), so an output sub-tile's whole
// k-tile sum is SIX accumulations (a1b1, a1b2, a2b1, a1b3, a2b2, a3b1) into an accumulator that starts at zero, and the 64 x 64 wave
// tile is formed as two 32 x 64 halves, one per C segment: C(2 kt) rows 0 .. 31, C(2 kt + 1) rows 32 .. 63, each 8 sub-tiles x 6
// products = 48 MFMAs of 16 cycles (the 768 cycles of a C segment of loop 2). `part` is one half (32 registers): a half's sum is
// folded into the running sum in the L segment behind its C segment, before the next C segment starts it afresh.
// Reads, 24 ds_read_b128 per wave and k-tile as loop 2: L(2 kt) all of B (4 column blocks x 3 planes, live over both C segments)
// and A rows 0 .. 31 (2 x 3); L(2 kt + 1) A rows 32 .. 63.
// LDS image: lane l of a 16-row operand reads chunk l >> 4 of row l & 15. Under loop 0 - 2's slot c ^ ((r >> 2) & 3) the first
// 16-lane group of ds_read_b128 (lanes 0 - 3, 12 - 15, 20 - 27: rows 0 - 3 and 12 - 15 at chunk 0, rows 4 - 11 at chunk 1) puts rows
// 0 - 3 and 4 - 7 on the same banks, and rows 8 - 11 and 12 - 15: 2-way. Loop 3's slot is c ^ h((r >> 2) & 3) with h = 0, 2, 3, 1
// (bx3_swz): every group then covers the 16 slots of 256 B once. Only the DMA's per-lane source offset and the read offsets differ.
// By count, slots as in loop 2 (half 0 runs L(j) in slot 2 j and C(j) in 2 j + 1, half 1 one slot later):
//   WAR  tile kt's buffer is read in L(2 kt) (18 reads) and L(2 kt + 1) (6 reads) and nowhere else: the last read is half 1's
//        L(2 kt + 1) in slot 4 kt + 3, retired by the lgkmcnt(0) in front of that slot's barrier; the DMAs of tile kt + 2 into that
//        buffer issue in L(2 kt + 2) and C(2 kt + 2), from slot 4 kt + 4 on;
//   RAW  every wave takes vmcnt(0) at the end of its L(2 kt + 1) — slot 4 kt + 2 for half 0, 4 kt + 3 for half 1 — with no fresh
//        DMA in front of it (the last piece went out in C(2 kt)); tile kt + 1 is first read in half 0's L(2 kt + 2), slot
//        4 kt + 4, behind the barrier that ends slot 4 kt + 3.
__device__ __forceinline__ uint32_t bx3_swz(int g) { return (0x78u >> (2 * g)) & 3u; }   // 0, 2, 3, 1

// the lane's offset of row rb + (l & 15), chunk l >> 4; the 16-row block i of the wave's 64 rows lies i KiB further
__device__ __forceinline__ uint32_t bx3_read_off(int rb) {
  const int l = threadIdx.x & 63, r = rb + (l & 15), c = l >> 4;
  return (uint32_t)(r * BX_ROWB + ((c ^ bx3_swz((r >> 2) & 3)) << 4));
}
__device__ __forceinline__ bx_bf16x8 bx3_frag_at(const char *S, uint32_t off, int i) {
  return __builtin_bit_cast(bx_bf16x8, *(const bx_i32x4 *)(S + off + i * 16 * BX_ROWB));
}

// acc += part as four scalar adds, pinned where they stand (bx_fold4)
__device__ __forceinline__ void bx3_fold4(bx_f32x4 &acc, const bx_f32x4 &part) {
  float r0 = acc[0] + part[0], r1 = acc[1] + part[1], r2 = acc[2] + part[2], r3 = acc[3] + part[3];
  asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));
  acc[0] = r0; acc[1] = r1; acc[2] = r2; acc[3] = r3;
}

// One k-tile of loop 3: L(2 kt) B C(2 kt) B L(2 kt + 1) B C(2 kt + 1) B. part: the sum of rows 32 .. 63 of the tile before on entry
// (folded in L(2 kt)), of this tile's on return; rows 0 .. 31 are folded in L(2 kt + 1). The nine pieces as in loop 2: three behind
// L(2 kt)'s reads, six between the MFMAs of C(2 kt), one behind every eighth (128 cycles apart, as there).
template <bool STAGE>
__device__ __forceinline__ void bx3_tile(const Bx3Bufs &S, Bx3Src &src, const Bx3Dst &dst, int64_t ka, int64_t kb, uint32_t lane_off, const uint32_t (&rd)[2],
                                         bx_f32x4 (&acc)[4][4], bx_f32x4 (&part)[2][4]) {
  constexpr int NL = 3, CSTEP = 8;
  bx_bf16x8 b[3][4];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    bx_bf16x8 a[3][2];
    uint32_t ra = rd[0], rb = rd[1];
    asm volatile("" : "+v"(ra), "+v"(rb));
    if (h == 0) {   // in the order the products first need them
#pragma unroll
      for (int i = 0; i < 2; ++i) a[0][i] = bx3_frag_at(S.a[0], ra, i);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[0][j] = bx3_frag_at(S.b[0], rb, j);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[1][j] = bx3_frag_at(S.b[1], rb, j);
#pragma unroll
      for (int i = 0; i < 2; ++i) a[1][i] = bx3_frag_at(S.a[1], ra, i);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[2][j] = bx3_frag_at(S.b[2], rb, j);
#pragma unroll
      for (int i = 0; i < 2; ++i) a[2][i] = bx3_frag_at(S.a[2], ra, i);
    } else {
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < 2; ++i) a[p][i] = bx3_frag_at(S.a[p], ra, 2 + i);
    }
    bx_fence();
    if (h == 0 && STAGE) {
#pragma unroll
      for (int n = 0; n < NL; ++n) bx_dma_n(src, dst, n, ka, kb, lane_off);
    }
    bx_fence();
    // the half formed by the C segment before: rows 32 .. 63 (of the tile before) in L(2 kt), rows 0 .. 31 in L(2 kt + 1)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) bx3_fold4(acc[2 * (1 - h) + i][j], part[i][j]);
    bx_fence();
    // L(2 kt): the reads are back before the barrier (WAR, and C holds no wait). L(2 kt + 1): and so are this wave's nine pieces (RAW)
    if (h == 0) __builtin_amdgcn_s_waitcnt(0xC07F);
    else __builtin_amdgcn_s_waitcnt(0x0070);
    bx2_barrier();
    // C: product-major over the eight sub-tiles, consecutive MFMAs write different accumulators; every MFMA behind a fence
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int n = q * 8 + i * 4 + j;
          if (q == 0) {
            const bx_f32x4 zero = {0, 0, 0, 0};
            part[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0][i], b[0][j], zero, 0, 0, 0);
          } else {
            part[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[BX_PA[q]][i], b[BX_PB[q]][j], part[i][j], 0, 0, 0);
          }
          if (STAGE && h == 0 && n % CSTEP == 1 && NL + n / CSTEP < 9) bx_dma_n(src, dst, NL + n / CSTEP, ka, kb, lane_off);
          bx_fence();
        }
    bx2_barrier();
  }
}

// Loop 3 behind the tile origin, whole: its own lane offset (bx3_swz), sixteen 16 x 16 accumulators, loop 2's prologue and barriers,
// the driver over bx3_tile, and its own write-out. Accumulator element e of lane l: row 4 (l >> 4) + e, column l & 15 of the 16 x 16
// sub-tile, so one wave store writes 16 consecutive floats (a 64-B half line) of four rows; the stores run along j, so that the
// halves of a line (sub-tiles j, j + 1, same register) are written back to back.
template <bool STAMP>
__device__ __forceinline__ void bx3_run(const Bx3Args &g, const Bx3Bufs &S0, const Bx3Bufs &S1, int64_t m0, int64_t n0) {
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, l = threadIdx.x & 63;
  const int nk = (int)(g.K / BX_BK);
  const uint32_t lane_off = bx_lane_off(g.rs, l, bx3_swz((l >> 4) & 3));
  bx_f32x4 acc[4][4], part[2][4];   // +0 into a running sum that starts at +0 and is never -0 changes no bit: the first tile folds zeros
  BX_ZERO(acc, 4, 4, 4)
  BX_ZERO(part, 2, 4, 4)
  BX_STAMP_BEGIN(STAMP, st)
  const int uw = __builtin_amdgcn_readfirstlane(wave);
  BX_BASES(g, S0, S1, m0, n0, uw, src, d0, d1)
  const uint32_t rd[2] = {bx3_read_off(wm * 64), bx3_read_off(wn * 64)};
  const int half = uw >> 2;   // (in an SGPR: a scalar branch)
#pragma unroll
  for (int n = 0; n < 9; ++n) bx_dma_n(src, d0, n, 0, 0, lane_off);   // the prologue stages tile 0 whole
  __builtin_amdgcn_s_waitcnt(0x0070);
  bx2_barrier();
  if (half) bx2_barrier();   // HALF 1: one segment behind
  BX_PAIRS_AND_TAIL(/* no barrier of its own */, bx3_tile, part)
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) bx3_fold4(acc[2 + i][j], part[i][j]);
  if (!half) bx2_barrier();   // HALF 0: waits for its partners' last C (both halves: 4 nk + 1 barriers behind the prologue's)
  BX_STAMP_END(STAMP, g, st)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t m = m0 + wm * 64 + i * 16 + 4 * (l >> 4) + e, n = n0 + wn * 64 + j * 16 + (l & 15);
        g.C[m * g.c_ms + n] = acc[i][j][e];
      }
}

// ---- the six-product kernel ---------------------------------------------------------------------------------------------------------
// LDS objects, flag word, tile origin, then one section per loop. (Loops 1 and 2 stand in the body, not in functions of their own
// as loop 3 does: lifted out, each came out with other machine code.)
template <int LOOP, bool STAMP = false>
__global__ void __launch_bounds__(BX_NT) k_gemm_bf16x3(Bx3Args g) {
  __shared__ __attribute__((aligned(16))) char sA00[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA01[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA02[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB00[BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB01[BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB02[BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA10[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA11[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA12[BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB10[BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB11[BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB12[BX_BN * BX_ROWB];
  if (g.flag && *g.flag != 0) return;   // (uniform: one scalar load and branch)
  const Bx3Bufs S0{{sA00, sA01, sA02}, {sB00, sB01, sB02}}, S1{{sA10, sA11, sA12}, {sB10, sB11, sB12}};
  BX_ORIGIN(g, m0, n0)

  // -- loop 3 (the default): bx3_run over bx3_tile, with accumulators, swizzle and write-out of its own; nothing below belongs to it
  if constexpr (LOOP == 3) {
    bx3_run<STAMP>(g, S0, S1, m0, n0);
    return;
  }

  // -- loops 0 - 2: four 32 x 32 accumulators per wave, the common LDS image
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, l = threadIdx.x & 63;
  const int nk = (int)(g.K / BX_BK);
  const uint32_t lane_off = bx_lane_off(g.rs, l, (l >> 4) & 3);
  bx_f32x16 acc[2][2];
  BX_ZERO(acc, 2, 2, 16)
  BX_STAMP_BEGIN(STAMP, st)

  // -- loop 0: bx_stage / bx_mma under the two-buffer driver
  if constexpr (LOOP == 0) {
    BX_LOOP0(3, 6)
  }

  // -- loop 1: bx_tile under the driver, a __syncthreads() in front of every tile; the last sub-tile's sum is carried from tile to tile
  if constexpr (LOOP == 1) {
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    BX_BASES(g, S0, S1, m0, n0, uw, src, d0, d1)
    const uint32_t rd[4] = {bx_read_off(wm * 64, 0), bx_read_off(wm * 64, 1), bx_read_off(wn * 64, 0), bx_read_off(wn * 64, 1)};
    // the sum carried into the first tile: +0 into a running sum that starts at +0 and is never -0 changes no bit
    bx_f32x16 carry = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int n = 0; n < 9; ++n) bx_dma_n(src, d0, n, 0, 0, lane_off);   // the prologue stages tile 0 whole
    BX_PAIRS_AND_TAIL(__syncthreads(), bx_tile, carry)
#pragma unroll
    for (int e = 0; e < 16; e += 4) bx_fold4(acc[1][1], carry, e);
  }

  // -- loop 2: bx2_tile under the driver; the only statements that depend on the half are the two barriers marked
  if constexpr (LOOP == 2) {
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    BX_BASES(g, S0, S1, m0, n0, uw, src, d0, d1)
    const uint32_t rd[4] = {bx_read_off(wm * 64, 0), bx_read_off(wm * 64, 1), bx_read_off(wn * 64, 0), bx_read_off(wn * 64, 1)};
    const int half = uw >> 2;   // (in an SGPR: a scalar branch)
    bx_f32x16 part[2][2];   // +0 into a running sum that starts at +0 and is never -0 changes no bit: the first tile folds zeros
    BX_ZERO(part, 2, 2, 16)
#pragma unroll
    for (int n = 0; n < 9; ++n) bx_dma_n(src, d0, n, 0, 0, lane_off);   // the prologue stages tile 0 whole
    __builtin_amdgcn_s_waitcnt(0x0070);
    bx2_barrier();
    if (half) bx2_barrier();   // HALF 1: one segment behind
    BX_PAIRS_AND_TAIL(/* no barrier of its own */, bx2_tile, part)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 16; e += 4) bx_fold4(acc[t >> 1][t & 1], part[t >> 1][t & 1], e);
    if (!half) bx2_barrier();   // HALF 0: waits for its partners' last C (both halves: 4 nk + 1 barriers behind the prologue's)
  }

  BX_STAMP_END(STAMP, g, st)
  BX_WRITE_C(g, m0, n0, wm, wn, l, acc)
}

// ---- reduced products (option gemm_products 3 / 1) ---------------------------------------------------------------------------------
// The first NPROD = 3 (a1b1 + a1b2 + a2b1) or 1 (a1b1) products of the list over NP = 2 / 1 ROUNDED planes per operand
// (md_bf16x3_split_rn): loop 0 of the kernel above with its tile, swizzle, walk, flag word and write-out. Per k-tile and
// element 2 NPROD truncating accumulations into a fresh accumulator and one rounded add into the running sum, in a fixed order. LDS:
// two buffers of NP x (256 + 128) rows x 64 B = 96 / 48 KiB.
template <int NPROD>
__global__ void __launch_bounds__(BX_NT) k_gemm_bf16xp(Bx3Args g) {
  constexpr int NP = NPROD == 1 ? 1 : 2;
  __shared__ __attribute__((aligned(16))) char sA0[NP * BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB0[NP * BX_BN * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sA1[NP * BX_BM * BX_ROWB];
  __shared__ __attribute__((aligned(16))) char sB1[NP * BX_BN * BX_ROWB];
  if (g.flag && *g.flag != 0) return;   // (uniform: one scalar load and branch)
  // (plane 2's entries point one plane tile on; under NP = 1 they are never read)
  const Bx3Bufs S0{{sA0, sA0 + (NP - 1) * BX_BM * BX_ROWB, nullptr}, {sB0, sB0 + (NP - 1) * BX_BN * BX_ROWB, nullptr}};
  const Bx3Bufs S1{{sA1, sA1 + (NP - 1) * BX_BM * BX_ROWB, nullptr}, {sB1, sB1 + (NP - 1) * BX_BN * BX_ROWB, nullptr}};
  BX_ORIGIN(g, m0, n0)
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, l = threadIdx.x & 63;
  const int nk = (int)(g.K / BX_BK);
  const uint32_t lane_off = bx_lane_off(g.rs, l, (l >> 4) & 3);
  bx_f32x16 acc[2][2];
  BX_ZERO(acc, 2, 2, 16)
  BX_LOOP0(NP, NPROD)
  bx_write_c(g, m0, n0, wm, wn, l, acc);
}

// one split pass, launched for the plane count: k3 the truncating three-plane kernel, k2 / k1 the rounding ones
template <class... A>
void bx_launch_split(int nplanes, void (*k3)(A...), void (*k2)(A...), void (*k1)(A...), dim3 grid, A... a) {
  (nplanes == 1 ? k1 : nplanes == 2 ? k2 : k3)<<<grid, 256, 0, md_stream()>>>(a...);
}

}  // namespace

// gemm.hip's plan steps: see md_hip.h
int md_gemm_bf16x3_split(const float *src, bool k_contig, int64_t rows, int64_t K, int64_t stride, void *planes, unsigned *flag, int layout, int nplanes) {
  const int64_t plane = rows * K * 2;
  char *dst = (char *)planes;
  if (k_contig && layout) {
    const dim3 grid((unsigned)((K / 32 + 31) / 32), (unsigned)(rows / 2 < 65535 ? rows / 2 : 65535));
    bx_launch_split(nplanes, k_bf16x3_split_rows_kt, k_bf16xp_split_rows_kt<2>, k_bf16xp_split_rows_kt<1>, grid, src, rows, K, stride, dst, plane, flag);
  } else if (k_contig) {
    const dim3 grid((unsigned)((K / 8 + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535));
    bx_launch_split(nplanes, k_bf16x3_split_rows, k_bf16xp_split_rows<2>, k_bf16xp_split_rows<1>, grid, src, rows, K, stride, dst, plane, flag);
  } else {
    const dim3 grid((unsigned)(rows / 64), (unsigned)(K / 32 < 65535 ? K / 32 : 65535));
    const int64_t prs = md_bf16x3_row_stride(layout, K), pks = md_bf16x3_k_step(layout, rows);
    bx_launch_split(nplanes, k_bf16x3_split_cols, k_bf16xp_split_cols<2>, k_bf16xp_split_cols<1>, grid, src, rows, K, stride, dst, plane, prs, pks, flag);
  }
  return MD_LAUNCH_CHECK("matmul(bf16x3 split)");
}

int md_gemm_bf16x3(const void *a_planes, const void *b_planes, float *c, int64_t M, int64_t N, int64_t K, int64_t c_ms, const unsigned *flag, int loop,
                   int layout, int band, int products, unsigned long long *stamp) {
  Bx3Args a{};
  a.A = (const char *)a_planes; a.B = (const char *)b_planes; a.C = c;
  a.K = K; a.c_ms = c_ms;
  a.a_plane = M * K * 2; a.b_plane = N * K * 2;
  a.rs = md_bf16x3_row_stride(layout, K); a.a_kstep = md_bf16x3_k_step(layout, M); a.b_kstep = md_bf16x3_k_step(layout, N);
  a.tiles_m = (int)(M / BX_BM); a.tiles_n = (int)(N / BX_BN);
  a.gm = md_bf16x3_band(a.tiles_m, MD_NUM_CUS / 8, band);   // (one block per CU: the CUs of an XCD hold that many tiles at a time)
  a.flag = flag;
  a.stamp = stamp;
  md_opt_table()[MD_OPT_GEMM_BF16X3_RUNS] += 1;
  const dim3 grid((unsigned)(a.tiles_m * a.tiles_n));
  // the six-product kernel by [loop][stamped]: any loop but 0, 2 and 3 is loop 1. The reduced kernels have one loop and no stamp.
  static void (*const six[4][2])(Bx3Args) = {{k_gemm_bf16x3<0, false>, k_gemm_bf16x3<0, true>},
                                             {k_gemm_bf16x3<1, false>, k_gemm_bf16x3<1, true>},
                                             {k_gemm_bf16x3<2, false>, k_gemm_bf16x3<2, true>},
                                             {k_gemm_bf16x3<3, false>, k_gemm_bf16x3<3, true>}};
  void (*const kernel)(Bx3Args) = products == 1   ? k_gemm_bf16xp<1>
                                  : products == 3 ? k_gemm_bf16xp<3>
                                                  : six[loop == 0 || loop == 2 || loop == 3 ? loop : 1][stamp != nullptr];
  MD_LAUNCH(kernel, grid, BX_NT, a);
  return MD_LAUNCH_CHECK("matmul(f32 as bf16x3)");
}
