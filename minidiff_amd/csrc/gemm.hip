// gemm.hip — matmul forward/backward on gfx950 matrix cores.
//
// Serves reference minidiff/backend/numpy.py:84 (np.matmul; also dot/tensordot
// :68,91 through the shim) and with it the three GEMMs of
// minidiff/ops/definitions.py:487-492:  C = A·B (NN), dA = G·Bᵀ (NT),
// dB = Aᵀ·G (TN). The transposes arrive as strided VIEWS (x.T is a stride
// permutation), so the kernel takes element strides for both operands and picks
// a tile loader per layout instead of materialising a transpose.
//
// f32: v_mfma_f32_32x32x2_f32 — exact f32 fma chain in k order, 256 FLOP/clk/CU
// (MI355X_MICROARCH.md "Matrix cores"): bound = 157.3 TFLOP/s.
//   block tile BM x BN x BK (256x128x16 for large problems; a cost model picks smaller tiles
//   for grids that do not fill whole rounds), 4 waves (2x2; 8 on the 128x128 tile of one-tile-per-CU grids), each wave (BM/2)x(BN/2) in 32x32
//   MFMA tiles (128 accumulator VGPRs at 256x128). Operands are staged in LDS k-major ([k][m], [k][n])
//   so a fragment read is one conflict-free ds_read_b32 per MFMA operand. Three
//   tiles are in flight per block: LDS buffer `cur` (being multiplied), the other
//   LDS buffer (being written from registers during the first MFMA steps) and the
//   registers (global loads of tile k+2 issued in step 2); fragment reads run one
//   step ahead in a register double buffer; one barrier per k-step. The k-tile body is
//   branch-free (one scheduling region) and sched_group_barrier places a slice of the step's
//   LDS reads / LDS writes / global loads behind EVERY MFMA, so a wave keeps the matrix pipe
//   fed while its memory work issues in the gaps (136 -> 139.5 TFLOP/s at 4096^3; with one
//   block per CU 60 -> 66). The loop is rotated: a tile's first fragments are read right
//   behind the barrier that publishes it, under the previous step's MFMAs.
//   Workgroup ids are remapped so the 8 XCDs each own a contiguous band of
//   output tiles (per-XCD L2 locality on the shared A row panel).
// Aligned operands whose tiles divide the problem (every BASELINE shape) run the DIRECT-TO-LDS kernels further down
// (k_gemm_f32_kc_glds for NN / NT, k_gemm_f32_tn_glds for TN: global_load_lds_dwordx4, no staging registers, no ds_write;
// 256x256x32 tiles, or eight waves on one 128x128x32 tile for grids of one tile per CU; DMA addresses as scalar base + 32-bit
// lane offset): 150-152 TFLOP/s at 4096^3 against 139.5 for the register-staged kernel described above, which keeps the
// unaligned / 16-deep / split-K cases (ragged sizes with 4-multiples run RAGGED variants of the direct-to-LDS kernels).
// ragged or unaligned shapes: guarded edge variant of the same kernel; few tiles and a long k:
// split-K with a deterministic split-order sum. f64: the same scheme on v_mfma_f64_16x16x4_f64
// (k_gemm_f64_mfma). Integers / tiny problems: a plain LDS-tiled kernel.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <utility>
#include <vector>

#include <hip/hip_ext.h>

#include "md_hip.h"

extern "C" int mdhip_alloc(size_t, void **);
extern "C" int mdhip_unary(int, const mdhip_array *, const mdhip_array *);
extern "C" int mdhip_free(void *);
extern "C" int mdhip_convert(const mdhip_array *, const mdhip_array *);

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LDP = 4;  // LDS row pad (floats): keeps the transposing ds_write_b32 at <=2-way conflicts

struct GemmArgs {
  const float *A, *B;
  float *C;
  int64_t M, N, K;
  int64_t a_bs, a_ms, a_ks, b_bs, b_ks, b_ns, c_bs, c_ms, c_ns;
  int tiles_m, tiles_n;
  int super_h;  // tile rows per band of the XCD-compact numbering (0: plain row-major)
  int vec_ok;  // EDGE kernels: operands are 16-B aligned, so a fully inside vector may be loaded whole
  // split-K (gridDim.y > 1): block y multiplies k in [y*k_chunk, (y+1)*k_chunk) into its own
  // partial C (C + y*c_split), summed afterwards in split order by k_gemm_splitk_sum
  int64_t k_chunk, c_split;
  // EPI = 1 (bias + relu epilogue): instead of C the kernel writes mask[m][n] = (acc + bias[n] > 0) and ONE partial
  // sum of max(acc + bias[n], 0) per block (partial[blockIdx.x]); see mdhip_matmul_bias_relu_sum
  const float *bias;
  uint8_t *mask;
  float *partial;
  float *sum_out;     // the 0-d result, written by the block that arrives last at `tickets` (md_ticket.h)
  unsigned *tickets;
  // diagnostic (MDHIP_GEMM_STAMP=1, never set in production): per block {shader cycles, 100 MHz ticks} around the whole kernel body
  unsigned long long *stamp;
  // ragged direct-to-LDS kernels: 16 B of zeros in device memory — what a DMA lane fetches for a position outside the operand
  const float *zero;
  // host side only: the row-contiguous operand A (B) sits in a buffer of OURS whose rows are padded to a multiple of four
  // elements (repacked copy, HipExec::gemm): a 16-B piece that straddles the M (N) edge reads the padding, which only feeds
  // output rows (columns) outside C — so M (N) need not be a multiple of 4 for the direct-to-LDS kernels
  int pad_m, pad_n;
  // C is addressed with unit stride along ROWS (a swapped "TT" product, HipExec::gemm) and everything is 16-B aligned: the direct-to-LDS
  // NN kernel stores the four consecutive rows a lane holds of one column as one vector
  int c_vec_rows;
  // non-null: the launch is the fp32 stand-in behind a bf16x3 product (plan_bf16x3) and runs only when the split passes set the word
  // (an operand holds an inf or a NaN); every block returns at once otherwise — one uniform load and branch at kernel entry
  const unsigned *run_if_set;
};

// ---- what the MFMA kernels share (f32 and f64, register-staged and direct-to-LDS) ---------------------------------------------------
// The pieces that stand in a kernel's own body (its tile, the accumulators, the k-tile driver and boundary, the write-out) are MACROS:
// as inlined functions they left the source equivalent but changed what the compiler made of nearly every kernel — the scalar prologue
// came out in another order, and with it the register assignment of the k loop — and this file's speed hangs on that (see SPLITK below:
// "instruction-for-instruction the same but with another register assignment", -2.4 %). Text expanded in place compiles to the code the
// copies it replaces compiled to. What runs INSIDE a k-tile lambda (md_mfma_slots, the DMA callables) and the tile loaders are functions:
// those changed nothing (scripts/isa_diff.py, profiles/gemm_shared_helpers_isa.txt).
template <int V> struct MdInt { static constexpr int value = V; };

// XCD-aware tile order: ids b, b+8, b+16.. share an XCD -> give them neighbours. Declares `bid`.
#define MD_XCD_BID(bid, nblk)                                          \
  int bid = blockIdx.x;                                                \
  if (((nblk) & 7) == 0) bid = (bid & 7) * ((nblk) >> 3) + (bid >> 3);
// The block's tile of the f32 kernels: the XCD order, then the band numbering (GemmArgs::super_h). Declares `tm`, `tn`.
// Bands: tiles are numbered column-major inside bands of super_h tile rows, so that the nblk/8 consecutive
// ids of one XCD form a compact block (8 x 8 tiles at 4096^2 instead of 2 x 32): fewer distinct
// A/B panels per XCD L2, i.e. less L2 <- fabric traffic for the same work (speed-neutral: the
// kernel is not fabric-bound)
#define MD_BLOCK_TILE(g, tm, tn)                                                                              \
  const int nblk = (g).tiles_m * (g).tiles_n;                                                                 \
  MD_XCD_BID(bid, nblk)                                                                                       \
  int tm, tn;                                                                                                 \
  if ((g).super_h > 1) {                                                                                      \
    const int band = bid / ((g).super_h * (g).tiles_n), within = bid - band * ((g).super_h * (g).tiles_n);    \
    const int hgt = (band + 1) * (g).super_h <= (g).tiles_m ? (g).super_h : (g).tiles_m - band * (g).super_h; \
    tn = within / hgt;                                                                                        \
    tm = band * (g).super_h + within - tn * hgt;                                                              \
  } else {                                                                                                    \
    tm = bid / (g).tiles_n;                                                                                   \
    tn = bid - tm * (g).tiles_n;                                                                              \
  }
// acc[WTM][WTN] of vectors of R elements = 0
#define MD_ZERO_ACC(acc, WTM, WTN, R)                                   \
  _Pragma("unroll") for (int i = 0; i < (WTM); ++i)                     \
    _Pragma("unroll") for (int j = 0; j < (WTN); ++j)                   \
      _Pragma("unroll") for (int r = 0; r < (R); ++r) acc[i][j][r] = 0;
// C write-out of a wave's WTM x WTN accumulator tiles (the kernel's constants); GUARD (compile-time): the tile may reach past C (edge
// and ragged kernels).
// C/D layout of the 32x32 f32 accumulator: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
#define MD_STORE_C32(GUARD, acc, C, g, m0, n0, wm, wn, l32, h)                                           \
  _Pragma("unroll") for (int i = 0; i < WTM; ++i)                                                        \
    _Pragma("unroll") for (int j = 0; j < WTN; ++j) {                                                    \
      const int64_t col = n0 + wn * (WTN * 32) + j * 32 + l32;                                           \
      _Pragma("unroll") for (int r = 0; r < 16; ++r) {                                                   \
        const int64_t row = m0 + wm * (WTM * 32) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;              \
        if (!(GUARD) || (row < (g).M && col < (g).N)) C[row * (g).c_ms + col * (g).c_ns] = acc[i][j][r]; \
      }                                                                                                  \
    }
// C/D of the f64 16x16 tile: col = lane&15, row = (lane>>4) + 4*r
#define MD_STORE_C64(GUARD, acc, C, g, m0, n0, wm, wn, l16, h)                                           \
  _Pragma("unroll") for (int i = 0; i < WTM; ++i)                                                        \
    _Pragma("unroll") for (int j = 0; j < WTN; ++j) {                                                    \
      const int64_t col = n0 + wn * (WTN * 16) + j * 16 + l16;                                           \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                    \
        const int64_t row = m0 + wm * (WTM * 16) + i * 16 + h + 4 * r;                                   \
        if (!(GUARD) || (row < (g).M && col < (g).N)) C[row * (g).c_ms + col * (g).c_ns] = acc[i][j][r]; \
      }                                                                                                  \
    }
// The k-tile driver of the direct-to-LDS kernels. ktile(MdInt<CUR>, kn) multiplies the tile in buffer CUR while the DMAs of k-tile
// kn go out; the loop is unrolled by NBUF so that the buffer is fixed at compile time (see k_gemm_f32_tn_glds). Three buffers:
// tile T is computed out of buffer T % 3 while the DMAs of tile T + 2 go out (past the end: a discarded re-read of the last tile)
#define MD_KTILE_ROTATE(NBUF, nk, ktile)                \
  int64_t kt = 0;                                       \
  if constexpr ((NBUF) == 2) {                          \
    for (; kt + 1 < nk; kt += 2) {                      \
      ktile(MdInt<0>{}, kt + 1);                        \
      ktile(MdInt<1>{}, kt + 2 < nk ? kt + 2 : nk - 1); \
    }                                                   \
    if (kt < nk) ktile(MdInt<0>{}, nk - 1);             \
  } else {                                              \
    for (; kt + 2 < nk; kt += 3) {                      \
      ktile(MdInt<0>{}, kt + 2);                        \
      ktile(MdInt<1>{}, kt + 3 < nk ? kt + 3 : nk - 1); \
      ktile(MdInt<2>{}, kt + 4 < nk ? kt + 4 : nk - 1); \
    }                                                   \
    if (kt < nk) ktile(MdInt<0>{}, nk - 1);             \
    if (kt + 1 < nk) ktile(MdInt<1>{}, nk - 1);         \
  }
// Publishes the tile computed next. Two buffers: __syncthreads(), which drains the DMAs in flight (vmcnt(0)). Three: a counted wait —
// this wave's DMAs of the tile computed NEXT are done (issued a whole k-tile ago; in the prologue: tile 0 landed), the PIECES it issued
// last (the tile after that) may still fly; the barrier then publishes every wave's share of the next tile and frees this tile's buffer.
// The s_waitcnt immediate of gfx9: vmcnt in bits 3:0 and 15:14; expcnt (7) and lgkmcnt (15) at their maxima, i.e. not waited for.
constexpr int md_vmcnt_imm(int n) { return (n & 0xF) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }
#define MD_PUBLISH_TILE(NBUF, PIECES)                                                                            \
  if constexpr ((NBUF) == 2) {                                                                                   \
    __syncthreads();                                                                                             \
  } else {                                                                                                       \
    constexpr int NW8 = (PIECES);   /* (a local, as the copies had: without it four kernels' code changed) */    \
    __builtin_amdgcn_s_waitcnt(md_vmcnt_imm(NW8));                                                               \
    __builtin_amdgcn_s_barrier();                                                                                \
  }
// the buffer the DMAs go to while buffer CUR is multiplied: the one behind CUR in the rotation (the other one of two)
constexpr int md_dma_buf(int nbuf, int cur) { return (cur + nbuf - 1) % nbuf; }
// Scheduling slots behind the MPS MFMAs of step `t` of a fragment pair: one MFMA each, behind it a fragment read of the next pair (if
// there is one: `more_reads`; NRD reads per pair) and a DMA piece (n_dma issued in this step). Tiles with >= 8 MFMAs per step: a read
// slot behind EVERY MFMA (measured best there); smaller ones: the next pair's reads go behind the FIRST MFMAs of this pair, one each
// (with a read slot behind every MFMA of the pair the scheduler parked the reads at its end, right in front of the wait for them)
template <int NRD, int MPS> __device__ __forceinline__ void md_mfma_slots(bool more_reads, int t, int n_dma) {
  constexpr bool RD_EVERY = MPS >= 8;
  const int rd_slots = RD_EVERY ? MPS : more_reads ? (NRD - t * MPS < 0 ? 0 : (NRD - t * MPS > MPS ? MPS : NRD - t * MPS)) : 0;
#pragma unroll
  for (int m = 0; m < MPS; ++m) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if (m < rd_slots) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    if (m < n_dma) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
  }
}

// Tile loaders for a ROWS x BK operand tile of T (float / double), NT threads, 16 B (V elements) per thread per pass.
// KC = the operand's k axis is the contiguous one in memory (row-major A, or B given as Bt).
template <class T> struct MdVec16 {
  static constexpr int N = 16 / sizeof(T);
  typedef T type __attribute__((ext_vector_type(N)));
};
template <int ROWS, int BK, int NT, bool KC, bool EDGE, class T>
__device__ __forceinline__ void load_tile(const T *__restrict__ P, int64_t rs, int64_t ks, int64_t row0, int64_t k0, int64_t rows, int64_t K,
                                          typename MdVec16<T>::type (&r)[ROWS * BK / (MdVec16<T>::N * NT)], bool vec_ok = true) {
  typedef typename MdVec16<T>::type vec;
  constexpr int V = MdVec16<T>::N;
  constexpr int PASSES = ROWS * BK / (V * NT);
  constexpr int TPR = BK / V;            // KC: threads per row
  constexpr int RPP = NT / TPR;          // KC: rows per pass
  constexpr int TPK = ROWS / V;          // !KC: threads per k-row
  constexpr int KPP = NT / TPK;          // !KC: k-rows per pass
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < PASSES; ++i) {
    int row, k;
    if constexpr (KC) { row = t / TPR + RPP * i; k = (t % TPR) * V; }
    else { k = t / TPK + KPP * i; row = (t % TPK) * V; }
    if constexpr (!EDGE) {
      r[i] = *reinterpret_cast<const vec *>(P + (row0 + row) * rs + (k0 + k) * ks);
    } else {
      // ragged M/N/K: a vector that lies wholly inside the operand is still ONE 16-B load (only the
      // last tile row/column and the K tail take the per-element path); unaligned operands always do
      const int64_t rr0 = row0 + row, kk0 = k0 + k;
      const bool inside = KC ? (rr0 < rows && kk0 + (V - 1) < K) : (kk0 < K && rr0 + (V - 1) < rows);
      if (vec_ok && inside) {
        r[i] = *reinterpret_cast<const vec *>(P + rr0 * rs + kk0 * ks);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const int64_t rr = rr0 + (KC ? 0 : j), kk = kk0 + (KC ? j : 0);
          r[i][j] = (rr < rows && kk < K) ? P[rr * rs + kk * ks] : (T)0;
        }
      }
    }
  }
}
// one pass (16 B per thread) of load_tile (whole aligned tiles only): lets the k-tile body place the global loads one by one
template <int ROWS, int BK, int NT, bool KC>
__device__ __forceinline__ void load_tile_pass(const float *__restrict__ P, int64_t rs, int64_t ks, int64_t row0, int64_t k0, f32x4 (&r)[ROWS * BK / (4 * NT)], int i) {
  constexpr int TPR = BK / 4, RPP = NT / TPR, TPK = ROWS / 4, KPP = NT / TPK;
  const int t = threadIdx.x;
  int row, k;
  if constexpr (KC) { row = t / TPR + RPP * i; k = (t % TPR) * 4; }
  else { k = t / TPK + KPP * i; row = (t % TPK) * 4; }
  r[i] = *reinterpret_cast<const f32x4 *>(P + (row0 + row) * rs + (k0 + k) * ks);
}
// the staged tile into its k-major LDS image; PAD = the image's row pad in elements (LDP / LDP64)
template <int ROWS, int BK, int NT, bool KC, int PAD, class T>
__device__ __forceinline__ void store_tile(T (*S)[ROWS + PAD], const typename MdVec16<T>::type (&r)[ROWS * BK / (MdVec16<T>::N * NT)]) {
  typedef typename MdVec16<T>::type vec;
  constexpr int V = MdVec16<T>::N;
  constexpr int PASSES = ROWS * BK / (V * NT);
  constexpr int TPR = BK / V, RPP = NT / TPR, TPK = ROWS / V, KPP = NT / TPK;
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < PASSES; ++i) {
    if constexpr (KC) {
      const int row = t / TPR + RPP * i, k = (t % TPR) * V;
      if constexpr (V == 2) {   // (written out: as a loop of two it changed the f64 kernels' code)
        S[k][row] = r[i][0];
        S[k + 1][row] = r[i][1];
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) S[k + j][row] = r[i][j];
      }
    } else {
      const int k = t / TPK + KPP * i, row = (t % TPK) * V;
      *reinterpret_cast<vec *>(&S[k][row]) = r[i];
    }
  }
}

// Fused epilogue of  loss = sum(where(X @ W + b > 0, X @ W + b, 0))  (reference call pattern: matmul
// definitions.py:487-492 -> add :424-427 -> greater :468-471 -> where :555-559 -> sum :403-407): the pre-activation
// never goes to memory; what the backward pass needs of it — the mask — does, as numpy.bool_ bytes, and the block's
// relu sum goes to partial[blockIdx.x]; the block that finishes last sums the partials in index order into sum_out.
// The accumulator layout gives a lane ONE column and 16 rows: written as it stands the mask would go out in 32-byte
// pieces of single bytes (measured: +106 us on the 8192 x 4096 x 4096 product). Instead the four lanes of a quad
// exchange their 16 result bits, each lane packs the 4 adjacent columns of 4 of the rows into one dword, the tile's
// mask is assembled in LDS (`sm`: an operand buffer, free by now; 16-byte groups XOR-swizzled by the row so that
// neither the dword writes nor the 16-byte reads conflict) and leaves as whole 128-byte rows. NPASS > 1: the tile's
// rows go through a scratch of BM / NPASS rows in NPASS rounds (256x256 tile: 64 KiB of mask, 32 KiB operand buffers).
// Called by every thread of the block, behind a barrier that retires the last reads of the operand buffers.
template <int BM, int BN, int WM, int WN, int NPASS>
__device__ __forceinline__ void md_epi_bias_relu(const f32x16 (&acc)[BM / (32 * WM)][BN / (32 * WN)], const GemmArgs &g, int64_t m0, int64_t n0,
                                                 uint32_t *sm, float *red) {
  constexpr int NT = 64 * WM * WN, WTM = BM / (32 * WM), WTN = BN / (32 * WN);
  constexpr int FP = WTM / NPASS;              // fragment rows of a wave per pass
  constexpr int SROWS = BM / NPASS;            // scratch rows
  static_assert(WTM % NPASS == 0 && BN % 16 == 0, "whole fragment rows per pass, 16-byte mask vectors");
  constexpr int RW = BN / 4;                   // dwords per mask row of the tile
  constexpr int GX = (BN / 16) < 8 ? (BN / 16) : 8;   // 16-byte groups per row that take part in the swizzle
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN, l32 = lane & 31, h = lane >> 5;
  const int q = l32 >> 2, jq = l32 & 3;
  float lsum = 0.0f;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    if (p > 0) __syncthreads();
#pragma unroll
    for (int ii = 0; ii < FP; ++ii) {
      const int i = p * FP + ii;
#pragma unroll
      for (int j = 0; j < WTN; ++j) {
        const int lcol = wn * (WTN * 32) + j * 32 + l32;
        const float bv = g.bias[n0 + lcol];
        uint32_t bits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float z = acc[i][j][r] + bv;
          const bool on = z > 0.0f;
          lsum += on ? z : 0.0f;
          bits |= (uint32_t)on << r;
        }
        uint32_t qb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) qb[k] = (uint32_t)__shfl((int)bits, (lane & ~3) + k, 64);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int r = jq + 4 * t;                                   // this lane packs accumulator rows r = jq, jq+4, jq+8, jq+12
          const uint32_t d = ((qb[0] >> r) & 1u) | (((qb[1] >> r) & 1u) << 8) | (((qb[2] >> r) & 1u) << 16) | (((qb[3] >> r) & 1u) << 24);
          const int srow = wm * (FP * 32) + ii * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;   // scratch row
          const int w = (wn * (WTN * 32) + j * 32) / 4 + q;          // dword index inside the mask row
          const int grp = (w >> 2) ^ (srow & (GX - 1));               // swizzled 16-byte group
          sm[srow * RW + (grp << 2) + (w & 3)] = d;
        }
      }
    }
    __syncthreads();
    constexpr int VPR = BN / 16;  // 16-byte vectors per row
    for (int v = threadIdx.x; v < SROWS * VPR; v += NT) {
      const int srow = v / VPR, gv = v - srow * VPR;
      const int swm = srow / (FP * 32), rem = srow - swm * (FP * 32);
      const int64_t row = m0 + swm * (WTM * 32) + p * (FP * 32) + rem;
      const uint4 val = *reinterpret_cast<const uint4 *>(sm + srow * RW + ((gv ^ (srow & (GX - 1))) << 2));
      *reinterpret_cast<uint4 *>(g.mask + row * g.N + n0 + gv * 16) = val;
    }
  }
  // block sum in a fixed order: lanes by shuffle, then the waves through LDS
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) lsum += __shfl_down(lsum, d, 64);
  if (lane == 0) red[wave] = lsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.0f;
#pragma unroll
    for (int w = 0; w < WM * WN; ++w) t += red[w];
    md_st_sc1(g.partial + blockIdx.x, t);
  }
  // the block that arrives last sums the per-block partials in index order (md_ticket.h): no finishing launch
  unsigned *flag = reinterpret_cast<unsigned *>(red + 32);
  const unsigned nblk = gridDim.x;
  if (!(nblk >= 64 ? md_ticket_last2(g.tickets, blockIdx.x, nblk, flag) : md_ticket_last(g.tickets, nblk, flag))) return;
  float t = md_fold_partials<RSum>(g.partial, nblk);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
  if (lane == 0) red[wave] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.0f;
#pragma unroll
    for (int w = 0; w < WM * WN; ++w) tot += red[w];
    g.sum_out[0] = tot;
  }
}

// BM x BN block tile, BK k-step, WM x WN waves, each wave (WTM*32) x (WTN*32).
// SPLITK is a separate instantiation on purpose: with the k-range arithmetic compiled into the plain
// kernel its main loop came out instruction-for-instruction the same but with another register
// assignment, and NN at 4096^3 dropped from 136.6 to 133.3 TFLOP/s (same-box A/B).
// (two waves per SIMD is what the schedule counts on for every tile up to 256 x 128 — 128 accumulator registers. The epilogue
// variants DECLARE it: left alone the bias/relu epilogue took 171 + 128 registers, one wave per SIMD, the whole product 5 % slower.
// The plain kernel keeps its allocation — 61 VGPRs + 128 AGPRs — untouched.)
template <int BM, int BN, int BK, int WM, int WN, bool A_KC, bool B_KC, bool EDGE, bool SPLITK = false, int SCHED = 0, int EPI = 0>
__global__ void __launch_bounds__(64 * WM * WN, (EPI != 0 && BM * BN <= 256 * 128 && WM * WN <= 4) ? 2 : 1) k_gemm_f32_mfma(GemmArgs g) {
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / (32 * WM), WTN = BN / (32 * WN);  // MFMA tiles per wave along m / n
  __shared__ float As[2][BK][BM + LDP];
  __shared__ float Bs[2][BK][BN + LDP];
  if (g.run_if_set && *g.run_if_set == 0) return;

  MD_BLOCK_TILE(g, tm, tn)
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t bz = blockIdx.z;
  const float *A = g.A + bz * g.a_bs;
  const float *B = g.B + bz * g.b_bs;
  float *C = g.C + bz * g.c_bs;
  int64_t Kl = g.K;  // this block's k extent
  if constexpr (SPLITK) {
    const int64_t ks0 = (int64_t)blockIdx.y * g.k_chunk;
    A += ks0 * g.a_ks;
    B += ks0 * g.b_ks;
    C += (int64_t)blockIdx.y * g.c_split;
    Kl = g.K - ks0 > g.k_chunk ? g.k_chunk : g.K - ks0;
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l32 = lane & 31, h = lane >> 5;
  unsigned long long st_c = 0, st_r = 0;
  if (g.stamp) { st_c = __builtin_amdgcn_s_memtime(); st_r = __builtin_amdgcn_s_memrealtime(); }

  f32x16 acc[WTM][WTN];
  MD_ZERO_ACC(acc, WTM, WTN, 16)

  f32x4 ra[BM * BK / (4 * NT)], rb[BN * BK / (4 * NT)];
  const int64_t nk = (Kl + BK - 1) / BK;
  // A tile rows = m (row stride a_ms), B tile rows = n (row stride b_ns)
  // Pipeline: LDS buffer `cur` holds tile kt, registers hold tile kt+1 (landed), and
  // inside the MFMA stream of tile kt the wave (step 0/1) writes tile kt+1 to the
  // other LDS buffer and (step 2) issues the global loads of tile kt+2 - so staging
  // costs no MFMA time of its own and the loads have ~6 steps (>3000 cycles) to land.
  const bool vec_ok = g.vec_ok != 0;
  load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, 0, g.M, Kl, ra, vec_ok);
  load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, 0, g.N, Kl, rb, vec_ok);
  store_tile<BM, BK, NT, A_KC, LDP>(As[0], ra);
  store_tile<BN, BK, NT, B_KC, LDP>(Bs[0], rb);
  if (nk > 1) {
    load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, BK, g.M, Kl, ra, vec_ok);
    load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, BK, g.N, Kl, rb, vec_ok);
  }
  __syncthreads();

  int cur = 0;
  float fa[2][WTM], fb[2][WTN];
  if constexpr (SCHED != 0) {  // rotated loop: a tile's first fragments are read right behind the barrier that publishes it
#pragma unroll
    for (int i = 0; i < WTM; ++i) fa[0][i] = As[0][h][wm * (WTM * 32) + i * 32 + l32];
#pragma unroll
    for (int j = 0; j < WTN; ++j) fb[0][j] = Bs[0][h][wn * (WTN * 32) + j * 32 + l32];
  }
  for (int64_t kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk, more2 = kt + 2 < nk;
    if constexpr (SCHED == 0) {
#pragma unroll
      for (int i = 0; i < WTM; ++i) fa[0][i] = As[cur][h][wm * (WTM * 32) + i * 32 + l32];
#pragma unroll
      for (int j = 0; j < WTN; ++j) fb[0][j] = Bs[cur][h][wn * (WTN * 32) + j * 32 + l32];
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int c = (kk >> 1) & 1;
      if (kk + 2 < BK) {  // fragment reads one step ahead (register double buffer)
#pragma unroll
        for (int i = 0; i < WTM; ++i) fa[c ^ 1][i] = As[cur][kk + 2 + h][wm * (WTM * 32) + i * 32 + l32];
#pragma unroll
        for (int j = 0; j < WTN; ++j) fb[c ^ 1][j] = Bs[cur][kk + 2 + h][wn * (WTN * 32) + j * 32 + l32];
      }
      if constexpr (SCHED == 0) {
        if (kk == 0 && more) store_tile<BM, BK, NT, A_KC, LDP>(As[cur ^ 1], ra);
        if (kk == 2 && more) store_tile<BN, BK, NT, B_KC, LDP>(Bs[cur ^ 1], rb);
        if (kk == 4 && more2) {
          load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, (kt + 2) * BK, g.M, Kl, ra, vec_ok);
          load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, (kt + 2) * BK, g.N, Kl, rb, vec_ok);
        }
        // pin the order: staging and prefetch are issued ahead of this step's MFMAs
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
          for (int j = 0; j < WTN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      } else {
        // branch-free body (the staging of the last two tiles is redundant, never wrong: the other
        // LDS buffer is not read again, and the tile index is clamped) so that the whole k-tile is
        // ONE scheduling region, and every MFMA is followed by a slice of the step's memory work
        if (kk == 0) store_tile<BM, BK, NT, A_KC, LDP>(As[cur ^ 1], ra);
        if (kk == 2) store_tile<BN, BK, NT, B_KC, LDP>(Bs[cur ^ 1], rb);
        // small tiles (2-4 MFMAs per step): the refill of the staging registers starts the step after they were written to LDS,
        // one 16-B load per step — A's passes from step 1, then B's — instead of all of them in step 4: a load issued in step 4
        // has 4 steps x 2 MFMAs (~1000 cycles at two waves per SIMD) to land before its LDS store, which the memory latency
        // exceeds (ablation: the operand loads cost these tiles 11 %, the 256x128 tile 4 %); 2048^3: 112.3-113.1 -> 115.7-116.2
        // TFLOP/s. The 256x128 tile keeps the step-4 burst (spread: 139.6-140.2 -> 137.4-137.9).
        constexpr bool SPREAD = !EDGE && BM * BN <= 128 * 128;
        constexpr int PA = BM * BK / (4 * NT), PB = BN * BK / (4 * NT);
        if constexpr (SPREAD) {
          const int64_t ktl = more2 ? kt + 2 : nk - 1;
          const int sidx = kk >> 1;
          if (sidx >= 1 && sidx - 1 < PA) load_tile_pass<BM, BK, NT, A_KC>(A, g.a_ms, g.a_ks, m0, ktl * BK, ra, sidx - 1);
          if (sidx - 1 >= PA && sidx >= 2 && sidx - 1 - PA < PB) load_tile_pass<BN, BK, NT, B_KC>(B, g.b_ns, g.b_ks, n0, ktl * BK, rb, sidx - 1 - PA);
        } else if (kk == 4) {
          const int64_t ktl = more2 ? kt + 2 : nk - 1;
          load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, ktl * BK, g.M, Kl, ra, vec_ok);
          load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, ktl * BK, g.N, Kl, rb, vec_ok);
        }
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
          for (int j = 0; j < WTN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i], fb[c][j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int m = 0; m < WTM * WTN; ++m) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                  // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                  // one LDS read (next step's fragments)
          if (kk == 0 || kk == 2) __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);  // LDS writes of the staged tile
          if (SPREAD ? (m == 0 && kk >= 2) : kk == 4) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);     // one global load of tile kt+2
        }
      }
    }
    __syncthreads();
    cur ^= 1;
    if constexpr (SCHED != 0) {  // (the last step's MFMAs are register-only and sink below the barrier: they cover these reads)
#pragma unroll
      for (int i = 0; i < WTM; ++i) fa[0][i] = As[cur][h][wm * (WTM * 32) + i * 32 + l32];
#pragma unroll
      for (int j = 0; j < WTN; ++j) fb[0][j] = Bs[cur][h][wn * (WTN * 32) + j * 32 + l32];
    }
  }

  if (g.stamp && threadIdx.x == 0) {   // (the stamps go to a buffer of their own: MI355X_MICROARCH.md "DVFS give-back" item 6)
    g.stamp[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st_c;
    g.stamp[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
  }
  if constexpr (EPI == 1) {
    static_assert(sizeof(As) >= (size_t)BM * BN, "the tile's mask must fit the A staging buffers");
    __syncthreads();
    md_epi_bias_relu<BM, BN, WM, WN, 1>(acc, g, m0, n0, reinterpret_cast<uint32_t *>(&As[0][0][0]), &Bs[0][0][0]);
    return;
  }
  MD_STORE_C32(EDGE, acc, C, g, m0, n0, wm, wn, l32, h)
}

// ---- TN products (both operands row-contiguous along the tile's rows) staged global -> LDS directly ------------------
// global_load_lds_dwordx4: one wave-instruction moves 64 lanes x 16 B = 1 KiB of the unpadded [BK][ROWS] image (ROWS/256 of a
// k-row, or 256/ROWS whole k-rows): no staging registers, no ds_write. The LDS address is wave-uniform (M0) + lane * 16, the
// SOURCE address is per lane. One tile ahead: tile kt+1 lands in the other buffer while tile kt is multiplied, and the barrier
// that ends the k-tile waits for it (vmcnt(0), which __syncthreads() emits for an LDS-DMA in flight). The two buffers of an
// operand are SEPARATE __shared__ objects and the k-loop is unrolled by two with the buffer fixed at compile time: with one
// array indexed by a runtime `cur` the compiler cannot tell the fragment reads of buffer cur from the DMA writes to cur^1 and
// drains the DMA (s_waitcnt vmcnt(0)) in front of every step's ds_read (seen in the .s of the first version of this kernel).
typedef __attribute__((address_space(3))) void md_lds_void;
typedef __attribute__((address_space(1))) const void md_gbl_void;
// RAGGED (problem sizes that the tiles do not divide; operand rows a multiple of 4 so that no 16-B piece straddles the edge): a lane
// whose four rows or whose k lie outside the operand fetches 16 B of zeros instead (the SOURCE of a DMA is per lane) — the tile
// image is then complete, the main loop is the same, the epilogue drops the rows / columns outside C.
template <int ROWS, int BK, int NT, bool RAGGED = false>
__device__ __forceinline__ void glds_tile_pass(const float *__restrict__ P, int64_t ks, int64_t row0, int64_t k0, float *S, int i,
                                               int64_t rows_total = 0, int64_t k_total = 0, const float *zero = nullptr) {
  constexpr int NW = NT / 64;
  static_assert(ROWS * BK % (256 * NW) == 0 && (ROWS & (ROWS - 1)) == 0, "whole 1-KiB pieces per wave");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int piece = i * NW + wave;
  const int f = piece * 256 + lane * 4, k = f / ROWS, r = f % ROWS;
  const float *src = P + (row0 + r) + (k0 + k) * ks;
  if constexpr (RAGGED) src = (row0 + r < rows_total && k0 + k < k_total) ? src : zero;
  __builtin_amdgcn_global_load_lds((md_gbl_void *)src, (md_lds_void *)(S + piece * 256), 16, 0, 0);
}

// The same piece with the address split into a WAVE-UNIFORM base (scalar registers; advanced per pass and per k-tile by scalar
// arithmetic) and a loop-invariant 32-bit per-lane byte offset: the DMA then takes its address as `v_offset, s[base]` and costs no
// vector ALU work. With the full 64-bit address per lane (above) the compiler re-derived it for every piece — a 32-bit multiply, a
// 64-bit multiply-add and two 64-bit shift-adds, ~45 cycles of VALU per DMA, which a lone wave per SIMD cannot hide behind a 64-cycle
// MFMA: ablation (profiles/r2_gemm_glds_ab.log, fifth part) priced the DMAs at 3.9 % of the 256x256 kernel and 8.7 % of the eight-wave
// 128x128 one. Whole-tile kernels only (the ragged variants select between two addresses per lane).
template <int ROWS> __device__ __forceinline__ uint32_t glds_tile_lane_off(int64_t ks) {
  const int lane = threadIdx.x & 63;
  constexpr int LPR = ROWS / 4 > 64 ? 64 : ROWS / 4;   // lanes per k-row
  return (uint32_t)(((int64_t)(lane / LPR) * ks + (lane % LPR) * 4) * 4);
}
// A wave-uniform 64-bit address, made opaque to the optimiser as two scalar words: the DMA's address is then visibly
// (scalar base) + (zero-extended 32-bit lane offset) and nothing else — left transparent, the compiler re-associated the sum of
// several pieces as ((lane offset + k offset) + piece base), a 64-bit VECTOR add per piece, and the DMA took the per-lane 64-bit
// address form (half the pieces of the NT kernel, scripts/isa_check.py). No instruction is emitted for this.
__device__ __forceinline__ const char *md_opaque_uniform(const char *p) {
  uint32_t lo = (uint32_t)(uintptr_t)p, hi = (uint32_t)((uintptr_t)p >> 32);
  asm("" : "+s"(lo), "+s"(hi));
  return reinterpret_cast<const char *>(((uintptr_t)hi << 32) | lo);
}
// `wbase` = the wave's first piece of tile 0 (uniform pointer: P + row0 + wave * KPP * ks), `step` = floats between a wave's consecutive
// pieces (NW * KPP * ks), `koff` = floats from tile 0 to this k-tile (k0 * ks): adds only, in scalar registers.
template <int ROWS, int BK, int NT, bool PRED = false>
__device__ __forceinline__ void glds_tile_pass_u(const float *wbase, int64_t step, int64_t koff, float *S, int i, uint32_t lane_off, bool pred = true) {
  constexpr int NW = NT / 64;
  static_assert(ROWS <= 256, "a piece covers whole k-rows");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const char *ub = md_opaque_uniform(reinterpret_cast<const char *>(wbase + koff + (int64_t)i * step));
  // keeps the 32 -> 64-bit extension of the lane offset next to the DMA (address mode `v_offset, s[base]`; hoisted out of the loop it
  // arrives as a 64-bit register pair and the DMA takes the slow per-lane 64-bit form): an empty, NON-volatile statement that "depends" on
  // the k-tile offset, so it can neither leave the loop nor pin the instruction order
  asm("" : "+v"(lane_off) : "s"((int)koff));
  // `pred` (rows-only ragged kernels): a lane whose four rows lie outside the operand fetches nothing — its LDS slot keeps whatever an
  // earlier tile left there, which only reaches outputs outside C (row m of A feeds row m of C alone, column n of B column n alone)
  if constexpr (PRED) {
    if (pred) __builtin_amdgcn_global_load_lds((md_gbl_void *)(ub + lane_off), (md_lds_void *)(S + (i * NW + wave) * 256), 16, 0, 0);
  } else {
    __builtin_amdgcn_global_load_lds((md_gbl_void *)(ub + lane_off), (md_lds_void *)(S + (i * NW + wave) * 256), 16, 0, 0);
  }
}

// RAGGED: 0 whole tiles | 1 any ragged size (zero-filled lanes, 64-bit lane addresses) | 2 ragged M / N with K % BK == 0 (predicated lanes,
// scalar-base addresses: the fast form)
// (NBUF = 3: three LDS buffers, DMA two k-tiles ahead, counted vmcnt at the boundary — see k_gemm_f32_kc_glds)
template <int BM, int BN, int BK, int WM, int WN, int RAGGED = 0, int NBUF = 2>
__global__ void __launch_bounds__(64 * WM * WN) k_gemm_f32_tn_glds(GemmArgs g) {
  static_assert(NBUF == 2 || (NBUF == 3 && RAGGED == 0), "three buffers: whole-tile kernel only");
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / (32 * WM), WTN = BN / (32 * WN);
  constexpr int PA = BM * BK / (4 * NT), PB = BN * BK / (4 * NT);
  // the next tile's DMA pieces go out within the first two steps of the k-tile (with the scalar-base addressing a DMA costs next to
  // nothing to issue; the eight-wave tile gained 7 % at 2048^3 over spreading them, the 256x256 tile is indifferent)
  constexpr int DMA_STEPS = 2;
  constexpr int PPS = (PA + PB + DMA_STEPS - 1) / DMA_STEPS;
  __shared__ __attribute__((aligned(16))) float A0[BK][BM];   // (DMA destinations: 16-B pieces)
  __shared__ __attribute__((aligned(16))) float A1[BK][BM];
  __shared__ __attribute__((aligned(16))) float B0[BK][BN];
  __shared__ __attribute__((aligned(16))) float B1[BK][BN];
  __shared__ __attribute__((aligned(16))) float A2[NBUF == 3 ? BK : 1][BM];
  __shared__ __attribute__((aligned(16))) float B2[NBUF == 3 ? BK : 1][BN];
  if (g.run_if_set && *g.run_if_set == 0) return;

  MD_BLOCK_TILE(g, tm, tn)
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t bz = blockIdx.z;
  const float *A = g.A + bz * g.a_bs;
  const float *B = g.B + bz * g.b_bs;
  float *C = g.C + bz * g.c_bs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l32 = lane & 31, h = lane >> 5;
  const int am = wm * (WTM * 32) + l32, bn = wn * (WTN * 32) + l32;

  f32x16 acc[WTM][WTN];
  MD_ZERO_ACC(acc, WTM, WTN, 16)

  const int64_t nk = RAGGED == 1 ? (g.K + BK - 1) / BK : g.K / BK;   // (forms 0 and 2: whole k-tiles only, the launcher checks)
#pragma unroll
  for (int i = 0; i < PA; ++i) glds_tile_pass<BM, BK, NT, RAGGED != 0>(A, g.a_ks, m0, 0, &A0[0][0], i, g.M, g.K, g.zero);
#pragma unroll
  for (int i = 0; i < PB; ++i) glds_tile_pass<BN, BK, NT, RAGGED != 0>(B, g.b_ks, n0, 0, &B0[0][0], i, g.N, g.K, g.zero);
  if constexpr (NBUF == 3) {   // tile 1 into buffer 1 (K >= 2 k-tiles: the launcher checks)
#pragma unroll
    for (int i = 0; i < PA; ++i) glds_tile_pass<BM, BK, NT, false>(A, g.a_ks, m0, BK, &A1[0][0], i, g.M, g.K, g.zero);
#pragma unroll
    for (int i = 0; i < PB; ++i) glds_tile_pass<BN, BK, NT, false>(B, g.b_ks, n0, BK, &B1[0][0], i, g.N, g.K, g.zero);
  }
  const uint32_t la = glds_tile_lane_off<BM>(g.a_ks), lb = glds_tile_lane_off<BN>(g.b_ks);   // per-lane parts of the DMA addresses (loop-invariant)
  const int uw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float *wa = A + m0 + (int64_t)uw * (256 / BM) * g.a_ks, *wb = B + n0 + (int64_t)uw * (256 / BN) * g.b_ks;   // uniform parts
  const int64_t sa = (int64_t)(NT / 64) * (256 / BM) * g.a_ks, sb = (int64_t)(NT / 64) * (256 / BN) * g.b_ks;
  // rows-only ragged form: which lanes' four rows lie inside the operands (the same lanes in every piece of a [k][row] image)
  bool pra = true, prb = true;
  if constexpr (RAGGED == 2) {
    pra = m0 + (int64_t)((threadIdx.x & 63) % (BM / 4 > 64 ? 64 : BM / 4)) * 4 < g.M;
    prb = n0 + (int64_t)((threadIdx.x & 63) % (BN / 4 > 64 ? 64 : BN / 4)) * 4 < g.N;
  }
  MD_PUBLISH_TILE(NBUF, PA + PB)   // tile 0 landed; with three buffers tile 1 may still fly

  // fragments for TWO steps (4 k) per LDS instruction: rows 4p+h and 4p+2+h of the [k][row] image lie 2*ROWS floats apart, a
  // multiple of 64 dwords, so the two loads of a lane fuse into one ds_read2st64_b32 — half the LDS read instructions; MFMA t of
  // the pair takes k = 4p+2t (lanes 0-31) and 4p+2t+1 (lanes 32-63): the plain k order
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  constexpr int NPR = BK / 4;
  f32x2 fa[2][WTM], fb[2][WTN];
#define MD_TN_BUF(X, BUF) ((BUF) == 0 ? X##0 : (BUF) == 1 ? X##1 : X##2)   /* buffer BUF (compile-time) of operand X */
#define MD_TN_READ(BUF, p, c)                                                                                          \
  {                                                                                                                    \
    _Pragma("unroll") for (int i = 0; i < WTM; ++i) {                                                                  \
      fa[c][i][0] = MD_TN_BUF(A, BUF)[4 * (p) + h][am + i * 32];                                                       \
      fa[c][i][1] = MD_TN_BUF(A, BUF)[4 * (p) + 2 + h][am + i * 32];                                                   \
    }                                                                                                                  \
    _Pragma("unroll") for (int q = 0; q < WTN; ++q) {                                                                  \
      fb[c][q][0] = MD_TN_BUF(B, BUF)[4 * (p) + h][bn + q * 32];                                                       \
      fb[c][q][1] = MD_TN_BUF(B, BUF)[4 * (p) + 2 + h][bn + q * 32];                                                   \
    }                                                                                                                  \
  }
  MD_TN_READ(0, 0, 0)
  // DMA piece pi of k-tile kn into buffer DST (compile-time), per operand: the addressing form of the RAGGED variant
  auto dma_a = [&](auto dstc, int64_t kn, int pi) __attribute__((always_inline)) {
    float *const S = &MD_TN_BUF(A, decltype(dstc)::value)[0][0];
    if constexpr (RAGGED == 1) glds_tile_pass<BM, BK, NT, true>(A, g.a_ks, m0, kn * BK, S, pi, g.M, g.K, g.zero);
    else if constexpr (RAGGED == 2) glds_tile_pass_u<BM, BK, NT, true>(wa, sa, kn * BK * g.a_ks, S, pi, la, pra);
    else glds_tile_pass_u<BM, BK, NT>(wa, sa, kn * BK * g.a_ks, S, pi, la);
  };
  auto dma_b = [&](auto dstc, int64_t kn, int pi) __attribute__((always_inline)) {
    float *const S = &MD_TN_BUF(B, decltype(dstc)::value)[0][0];
    if constexpr (RAGGED == 1) glds_tile_pass<BN, BK, NT, true>(B, g.b_ks, n0, kn * BK, S, pi, g.N, g.K, g.zero);
    else if constexpr (RAGGED == 2) glds_tile_pass_u<BN, BK, NT, true>(wb, sb, kn * BK * g.b_ks, S, pi, lb, prb);
    else glds_tile_pass_u<BN, BK, NT>(wb, sb, kn * BK * g.b_ks, S, pi, lb);
  };
  auto ktile = [&](auto curc, int64_t kn) {
    constexpr int CUR = decltype(curc)::value;
#pragma unroll
    for (int p = 0; p < NPR; ++p) {
      const int c = p & 1;
      if (p + 1 < NPR) MD_TN_READ(CUR, p + 1, c ^ 1)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int sidx = 2 * p + t;
        int n_dma = 0;
#pragma unroll
        for (int q = 0; q < PPS; ++q) {
          const int pi = sidx * PPS + q;
          if (pi < PA) {
            dma_a(MdInt<md_dma_buf(NBUF, CUR)>{}, kn, pi);
            ++n_dma;
          } else if (pi < PA + PB) {
            dma_b(MdInt<md_dma_buf(NBUF, CUR)>{}, kn, pi - PA);
            ++n_dma;
          }
        }
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
          for (int j = 0; j < WTN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i][t], fb[c][j][t], acc[i][j], 0, 0, 0);
        md_mfma_slots<WTM + WTN, WTM * WTN>(p + 1 < NPR, t, n_dma);
      }
    }
    MD_PUBLISH_TILE(NBUF, PA + PB)
    MD_TN_READ((CUR + 1) % NBUF, 0, 0)
  };
  MD_KTILE_ROTATE(NBUF, nk, ktile)
#undef MD_TN_READ
#undef MD_TN_BUF

  MD_STORE_C32(RAGGED != 0, acc, C, g, m0, n0, wm, wn, l32, h)
}

// ---- NN / NT products: the k-contiguous operand(s) direct to LDS as well -------------------------------------------------
// A lane-linear DMA cannot transpose, so the k-contiguous operand keeps its memory order in LDS: 1-KiB pieces of 16 rows x 16 k,
// stored [k/4][row][4] (lane = (k/4) * 16 + row: the source of one wave-instruction is 16 rows x 64 B, as with register staging).
// A fragment is then ONE ds_read_b128 per 32 rows and EIGHT k: the lanes of half h take the four k of group 2j+h, and MFMA t of
// the pair multiplies k = 8j + t (lanes 0-31) and k = 8j + 4 + t (lanes 32-63) — v_mfma_f32_32x32x2 does not care WHICH two k a
// call carries, only that A and B agree. The sum over k therefore runs in the order (0,4),(1,5),(2,6),(3,7),(8,12).. instead of
// (0,1),(2,3)..: a different rounding sequence from the register-staged kernel (both are plain f32 fma chains; integers stay exact).
// B is either k-contiguous too (NT: same image) or row-contiguous (NN: the [k][n] image of k_gemm_f32_tn_glds, b32 reads at
// k = 8j + 4h + t). 16 consecutive lanes of a b128 read cover one 256-B run of a piece: no bank conflicts.
template <int ROWS, int BK, int NT, bool RAGGED = false>
__device__ __forceinline__ void glds_kc_pass(const float *__restrict__ P, int64_t rs, int64_t row0, int64_t k0, float *S, int i,
                                             int64_t rows_total = 0, int64_t k_total = 0, const float *zero = nullptr) {
  constexpr int NW = NT / 64, KH = BK / 16;
  static_assert(ROWS * BK % (256 * NW) == 0 && BK % 16 == 0, "whole 1-KiB pieces per wave");
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // a wave takes BOTH k-halves of a 16-row block back to back (the two pieces share their 128-B lines)
  const int rb = (i / KH) * NW + wave, kh = i % KH;
  const int row = rb * 16 + (lane & 15), k = kh * 16 + (lane >> 4) * 4;
  const float *src = P + (row0 + row) * rs + k0 + k;
  if constexpr (RAGGED) src = (row0 + row < rows_total && k0 + k < k_total) ? src : zero;   // (K % 4 == 0: no piece straddles the end)
  __builtin_amdgcn_global_load_lds((md_gbl_void *)src, (md_lds_void *)(S + (rb * KH + kh) * 256), 16, 0, 0);
}

__device__ __forceinline__ uint32_t glds_kc_lane_off(int64_t rs) {
  const int lane = threadIdx.x & 63;
  return (uint32_t)(((int64_t)(lane & 15) * rs + (lane >> 4) * 4) * 4);
}
// `wbase` = P + (row0 + wave * 16) * rs (uniform), `step` = NW * 16 * rs floats between a wave's 16-row blocks, `k0` = first k of the tile
template <int ROWS, int BK, int NT, bool PRED = false>
__device__ __forceinline__ void glds_kc_pass_u(const float *wbase, int64_t step, int64_t k0, float *S, int i, uint32_t lane_off, int rows_left = 0) {
  constexpr int NW = NT / 64, KH = BK / 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rb = (i / KH) * NW + wave, kh = i % KH;
  // (the k-half's 64 bytes ride in the LANE offset: with them in the base, two pieces 64 B apart were folded into one 64-bit per-lane
  // address plus a constant and the DMAs fell back to the `v[N:N+1], off` form with a v_lshl_add_u64 each: scripts/isa_check.py)
  const char *ub = md_opaque_uniform(reinterpret_cast<const char *>(wbase + (int64_t)(i / KH) * step + k0));
  lane_off += (uint32_t)(kh * 64);
  asm("" : "+v"(lane_off) : "s"((int)k0));   // (as in glds_tile_pass_u)
  // `rows_left` = rows of the operand from this tile's first row on (rows-only ragged kernels; see glds_tile_pass_u)
  if (!PRED || (int)(threadIdx.x & 15) + rb * 16 < rows_left) __builtin_amdgcn_global_load_lds((md_gbl_void *)(ub + lane_off), (md_lds_void *)(S + (rb * KH + kh) * 256), 16, 0, 0);
}

// NBUF = 3 (whole tiles, no epilogue; MDHIP_GEMM_NBUF=3, experiment): THREE LDS buffers per operand, the DMA runs TWO k-tiles ahead and the
// k-tile boundary waits with a COUNTED `s_waitcnt vmcnt(PA + PB)` — the tile needed next is complete, the one just issued may still be
// in flight — instead of the full drain a `__syncthreads()` brings (SQ counters: the small tiles park 20 % of their cycles there).
// CT: C is addressed with unit stride along rows (a "TT" product run as the swapped NN product, HipExec::gemm): 16-B stores of the
// four consecutive rows a lane holds. A separate instantiation — as a run-time branch it cost the 256x256 NN kernel its last registers.
template <int BM, int BN, int BK, int WM, int WN, bool B_KC, int EPI = 0, int RAGGED = 0, int NBUF = 2, bool CT = false>
__global__ void __launch_bounds__(64 * WM * WN) k_gemm_f32_kc_glds(GemmArgs g) {
  static_assert(NBUF == 2 || (NBUF == 3 && EPI == 0 && RAGGED == 0), "three buffers: plain whole-tile kernel only");
  static_assert(!CT || (!B_KC && EPI == 0 && RAGGED == 0), "transposed C addressing: whole-tile NN form only");
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / (32 * WM), WTN = BN / (32 * WN);
  constexpr int PA = BM * BK / (4 * NT), PB = BN * BK / (4 * NT), NP = BK / 8, KH = BK / 16;
  // the next tile's DMA pieces go out within the first DMA_STEPS steps of the k-tile (16 steps at BK 32); same-box A/B at 4096^3 NT,
  // r2_gemm_glds_ab.log: 16 steps 138.9 | 8: 144.6 | 4: 146.0 | 3: 145.5 | 2: 143.8 | 1: 140.4 TFLOP/s
  constexpr int DMA_STEPS = 4;   // (re-checked after the scalar-base addressing: 2 -> NT 146.7, 8 -> 147.9, 4 -> 149.2; all of the
                                 //  eight-wave tile's four pieces behind ONE step: NN 124 -> 114, NT 121 -> 99 at 2048^3)
  constexpr int PPS = (PA + PB + DMA_STEPS - 1) / DMA_STEPS;   // DMA pieces per step
  static_assert(NP % 2 == 0, "an even number of k-pairs per tile (fragment double buffer)");
  __shared__ __attribute__((aligned(16))) float A0[BM * BK];
  __shared__ __attribute__((aligned(16))) float A1[BM * BK];
  __shared__ __attribute__((aligned(16))) float B0[BN * BK];
  __shared__ __attribute__((aligned(16))) float B1[BN * BK];
  __shared__ __attribute__((aligned(16))) float A2[NBUF == 3 ? BM * BK : 4];
  __shared__ __attribute__((aligned(16))) float B2[NBUF == 3 ? BN * BK : 4];
  if (g.run_if_set && *g.run_if_set == 0) return;

  MD_BLOCK_TILE(g, tm, tn)
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t bz = blockIdx.z;
  const float *A = g.A + bz * g.a_bs;
  const float *B = g.B + bz * g.b_bs;
  float *C = g.C + bz * g.c_bs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l32 = lane & 31, h = lane >> 5;
  // lane bases (floats) into the images; fragment i / pair j add compile-time offsets
  const int arow = wm * (WTM * 32) + l32;
  const int abase = (arow >> 4) * (KH * 256) + (arow & 15) * 4 + h * 64;
  const int brow = wn * (WTN * 32) + l32;
  const int bbase = B_KC ? (brow >> 4) * (KH * 256) + (brow & 15) * 4 + h * 64 : h * 4 * BN + brow;

  f32x16 acc[WTM][WTN];
  MD_ZERO_ACC(acc, WTM, WTN, 16)

  const int64_t nk = RAGGED == 1 ? (g.K + BK - 1) / BK : g.K / BK;
  unsigned long long st_c = 0, st_r = 0;   // diagnostic stamps (MDHIP_GEMM_STAMP=1), as in k_gemm_f32_mfma
  if (g.stamp) { st_c = __builtin_amdgcn_s_memtime(); st_r = __builtin_amdgcn_s_memrealtime(); }
#pragma unroll
  for (int i = 0; i < PA; ++i) glds_kc_pass<BM, BK, NT, RAGGED != 0>(A, g.a_ms, m0, 0, A0, i, g.M, g.K, g.zero);
#pragma unroll
  for (int i = 0; i < PB; ++i) {
    if constexpr (B_KC) glds_kc_pass<BN, BK, NT, RAGGED != 0>(B, g.b_ns, n0, 0, B0, i, g.N, g.K, g.zero);
    else glds_tile_pass<BN, BK, NT, RAGGED != 0>(B, g.b_ks, n0, 0, B0, i, g.N, g.K, g.zero);
  }
  if constexpr (NBUF == 3) {   // tile 1 into buffer 1 (K >= 2 k-tiles: the launcher checks)
#pragma unroll
    for (int i = 0; i < PA; ++i) glds_kc_pass<BM, BK, NT, false>(A, g.a_ms, m0, BK, A1, i, g.M, g.K, g.zero);
#pragma unroll
    for (int i = 0; i < PB; ++i) {
      if constexpr (B_KC) glds_kc_pass<BN, BK, NT, false>(B, g.b_ns, n0, BK, B1, i, g.N, g.K, g.zero);
      else glds_tile_pass<BN, BK, NT, false>(B, g.b_ks, n0, BK, B1, i, g.N, g.K, g.zero);
    }
  }
  const uint32_t la = glds_kc_lane_off(g.a_ms), lb = B_KC ? glds_kc_lane_off(g.b_ns) : glds_tile_lane_off<BN>(g.b_ks);   // (loop-invariant lane parts of the DMA addresses)
  const int uw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float *wa = A + (m0 + (int64_t)uw * 16) * g.a_ms;   // uniform parts: adds only inside the loop
  const float *wb = B_KC ? B + (n0 + (int64_t)uw * 16) * g.b_ns : B + n0 + (int64_t)uw * (256 / BN) * g.b_ks;
  const int64_t sa = (int64_t)(NT / 64) * 16 * g.a_ms, sb = B_KC ? (int64_t)(NT / 64) * 16 * g.b_ns : (int64_t)(NT / 64) * (256 / BN) * g.b_ks;
  // rows-only ragged form (RAGGED == 2): rows of the operands from this tile's first row on / lanes of the [k][n] image inside B
  int rla = 0, rlb = 0;
  bool prb = true;
  if constexpr (RAGGED == 2) {
    rla = (int)(g.M - m0 < (1 << 30) ? g.M - m0 : (1 << 30));
    rlb = (int)(g.N - n0 < (1 << 30) ? g.N - n0 : (1 << 30));
    if constexpr (!B_KC) prb = n0 + (int64_t)((threadIdx.x & 63) % (BN / 4 > 64 ? 64 : BN / 4)) * 4 < g.N;
  }
  MD_PUBLISH_TILE(NBUF, PA + PB)   // tile 0 landed; with three buffers tile 1 may still fly

  f32x4 fa[2][WTM], fb[2][WTN];
  // fragments of k-pair j out of buffer BUF (compile-time) into register set c
#define MD_KC_BUF(X, BUF) ((BUF) == 0 ? X##0 : (BUF) == 1 ? X##1 : X##2)   /* buffer BUF (compile-time) of operand X */
#define MD_KC_READ(BUF, j, c)                                                                                                   \
  {                                                                                                                             \
    const int joff = ((j) >> 1) * 256 + (((2 * (j)) & 3) * 64);   /* (a constant once the pair loop is unrolled) */             \
    _Pragma("unroll") for (int i = 0; i < WTM; ++i)                                                                             \
      fa[c][i] = *reinterpret_cast<const f32x4 *>(MD_KC_BUF(A, BUF) + abase + i * (2 * KH * 256) + joff);                       \
    _Pragma("unroll") for (int q = 0; q < WTN; ++q) {                                                                           \
      if constexpr (B_KC) fb[c][q] = *reinterpret_cast<const f32x4 *>(MD_KC_BUF(B, BUF) + bbase + q * (2 * KH * 256) + joff);   \
      else {                                                                                                                    \
        _Pragma("unroll") for (int t = 0; t < 4; ++t) fb[c][q][t] = MD_KC_BUF(B, BUF)[bbase + (8 * (j) + t) * BN + q * 32];     \
      }                                                                                                                         \
    }                                                                                                                           \
  }
  MD_KC_READ(0, 0, 0)
  // DMA piece pi of k-tile kn into buffer DST (compile-time), per operand: the addressing form of the RAGGED variant and, for B, of
  // its image (B_KC: the k-contiguous pieces, else the [k][n] rows of k_gemm_f32_tn_glds)
  auto dma_a = [&](auto dstc, int64_t kn, int pi) __attribute__((always_inline)) {
    float *const S = MD_KC_BUF(A, decltype(dstc)::value);
    if constexpr (RAGGED == 1) glds_kc_pass<BM, BK, NT, true>(A, g.a_ms, m0, kn * BK, S, pi, g.M, g.K, g.zero);
    else if constexpr (RAGGED == 2) glds_kc_pass_u<BM, BK, NT, true>(wa, sa, kn * BK, S, pi, la, rla);
    else glds_kc_pass_u<BM, BK, NT>(wa, sa, kn * BK, S, pi, la);
  };
  auto dma_b = [&](auto dstc, int64_t kn, int pi) __attribute__((always_inline)) {
    float *const S = MD_KC_BUF(B, decltype(dstc)::value);
    if constexpr (RAGGED == 1) {
      if constexpr (B_KC) glds_kc_pass<BN, BK, NT, true>(B, g.b_ns, n0, kn * BK, S, pi, g.N, g.K, g.zero);
      else glds_tile_pass<BN, BK, NT, true>(B, g.b_ks, n0, kn * BK, S, pi, g.N, g.K, g.zero);
    } else if constexpr (RAGGED == 2) {
      if constexpr (B_KC) glds_kc_pass_u<BN, BK, NT, true>(wb, sb, kn * BK, S, pi, lb, rlb);
      else glds_tile_pass_u<BN, BK, NT, true>(wb, sb, kn * BK * g.b_ks, S, pi, lb, prb);
    } else {
      if constexpr (B_KC) glds_kc_pass_u<BN, BK, NT>(wb, sb, kn * BK, S, pi, lb);
      else glds_tile_pass_u<BN, BK, NT>(wb, sb, kn * BK * g.b_ks, S, pi, lb);
    }
  };

  auto ktile = [&](auto curc, int64_t kn) {
    constexpr int CUR = decltype(curc)::value;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int c = j & 1;
      if (j + 1 < NP) MD_KC_READ(CUR, j + 1, c ^ 1)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int sidx = j * 4 + t;
        int n_dma = 0;
#pragma unroll
        for (int q = 0; q < PPS; ++q) {
          const int pi = sidx * PPS + q;
          if (pi < PA) {
            dma_a(MdInt<md_dma_buf(NBUF, CUR)>{}, kn, pi);
            ++n_dma;
          } else if (pi < PA + PB) {
            dma_b(MdInt<md_dma_buf(NBUF, CUR)>{}, kn, pi - PA);
            ++n_dma;
          }
        }
#pragma unroll
        for (int i = 0; i < WTM; ++i)
#pragma unroll
          for (int q = 0; q < WTN; ++q) acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i][t], fb[c][q][t], acc[i][q], 0, 0, 0);
        md_mfma_slots<WTM + (B_KC ? WTN : 4 * WTN), WTM * WTN>(j + 1 < NP, t, n_dma);   // (a b32 image of B: four reads per fragment)
      }
    }
    MD_PUBLISH_TILE(NBUF, PA + PB)
    MD_KC_READ((CUR + 1) % NBUF, 0, 0)
  };
  MD_KTILE_ROTATE(NBUF, nk, ktile)
#undef MD_KC_READ
#undef MD_KC_BUF

  if (g.stamp && threadIdx.x == 0) {
    g.stamp[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - st_c;
    g.stamp[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - st_r;
  }
  if constexpr (EPI == 1) {   // bias + relu-sum + mask instead of C (md_epi_bias_relu); the mask goes through A0, 32 KiB at most
    constexpr int NPASS = (BM * BN > BM * BK * 4) ? (BM * BN) / (BM * BK * 4) : 1;
    __syncthreads();
    md_epi_bias_relu<BM, BN, WM, WN, NPASS>(acc, g, m0, n0, reinterpret_cast<uint32_t *>(A0), B0);
    return;
  }
  if constexpr (CT) {
    // C^T addressing of a swapped TT product: rows are the unit-stride axis. A lane holds four consecutive rows of ONE column, so
    // stored as they stand a wave-store is 32 columns x 32 B — pieces of lines, which drain slowly (the kernel lasted 1041 us against
    // NN's 942 with dispatches serialised). Each 32 x 32 accumulator tile is transposed through a wave-private LDS patch instead
    // ([column][row], rows padded to 36 words: 16-B aligned, conflict-light) and leaves as whole 128-B row segments: eight lanes per
    // C^T row, eight rows per store.
    __shared__ __attribute__((aligned(16))) float Tt[WM * WN][32][36];
    float(*T)[36] = Tt[wave];
    const int rl = lane >> 3, cl = (lane & 7) * 4;   // read side: column rl + 8k of the tile, rows cl .. cl + 3
#pragma unroll
    for (int i = 0; i < WTM; ++i)
#pragma unroll
      for (int j = 0; j < WTN; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          *reinterpret_cast<f32x4 *>(&T[l32][8 * q + 4 * h]) = f32x4{acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
        __builtin_amdgcn_wave_barrier();   // (the LDS queue of a wave is in order: the reads below see the writes above)
        const int64_t row = m0 + wm * (WTM * 32) + i * 32 + cl;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t col = n0 + wn * (WTN * 32) + j * 32 + rl + 8 * k;
          *reinterpret_cast<f32x4 *>(C + row + col * g.c_ns) = *reinterpret_cast<const f32x4 *>(&T[rl + 8 * k][cl]);
        }
        __builtin_amdgcn_wave_barrier();
      }
    return;
  }
  MD_STORE_C32(RAGGED != 0, acc, C, g, m0, n0, wm, wn, l32, h)
}

// Repack of a misaligned operand (HipExec::gemm): rows x cols with unit stride along cols and ANY row stride / start -> rows padded to
// `ld`. A block copies 1024 columns of four rows: coalesced 4-B loads (the source rows start anywhere), 4-B stores.
__global__ void __launch_bounds__(256) k_repack_rows(const float *__restrict__ src, int64_t rows, int64_t cols, int64_t row_stride, float *__restrict__ dst,
                                                     int64_t ld) {
  const int64_t c0 = (int64_t)blockIdx.x * 1024 + threadIdx.x, r0 = (int64_t)blockIdx.y * 4;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int64_t r = r0 + rr;
    if (r >= rows) break;
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t c = c0 + 256 * k;
      v[k] = c < cols ? src[r * row_stride + c] : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t c = c0 + 256 * k;
      if (c < cols) dst[r * ld + c] = v[k];
    }
  }
}

// ---- plain tiled kernel: any dtype, any strides (f64 / ints / tiny problems) ------
template <class T>
__global__ void __launch_bounds__(256) k_gemm_generic(MdGemm g) {
  __shared__ T As[16][17];
  __shared__ T Bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t bz = blockIdx.z;
  const T *A = (const T *)g.a + bz * g.a_bs;
  const T *B = (const T *)g.b + bz * g.b_bs;
  T *C = (T *)g.c + bz * g.c_bs;
  const int64_t row = (int64_t)blockIdx.y * 16 + ty, col = (int64_t)blockIdx.x * 16 + tx;
  T acc = (T)0;
  for (int64_t k0 = 0; k0 < g.K; k0 += 16) {
    const int64_t ka = k0 + tx, kb = k0 + ty;
    As[ty][tx] = (row < g.M && ka < g.K) ? A[row * g.a_ms + ka * g.a_ks] : (T)0;
    Bs[ty][tx] = (kb < g.K && col < g.N) ? B[kb * g.b_ks + col * g.b_ns] : (T)0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if constexpr (md_is_float<T>::value) acc = fma(As[ty][k], Bs[k][tx], acc);
      else acc = BAdd::apply(acc, BMul::apply(As[ty][k], Bs[k][tx]));
    }
    __syncthreads();
  }
  if (row < g.M && col < g.N) C[row * g.c_ms + col * g.c_ns] = acc;
}

// C[b][m][n] = sum over splits (in split order: deterministic) of the partial products
__global__ void __launch_bounds__(MD_BLOCK) k_gemm_splitk_sum(const float *__restrict__ part, int splits, int64_t batch, int64_t M, int64_t N,
                                                             float *C, int64_t c_bs, int64_t c_ms, int64_t c_ns) {
  const int64_t total = batch * M * N, gs = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gs) {
    float acc = part[i];
    for (int s = 1; s < splits; ++s) acc += part[(int64_t)s * total + i];
    const int64_t b = i / (M * N), r = i - b * (M * N), m = r / N, n = r - m * N;
    C[b * c_bs + m * c_ms + n * c_ns] = acc;
  }
}


// ======================= f64: v_mfma_f64_16x16x4_f64 ===========================================
// Same staging scheme as the f32 kernel (k-major LDS double buffer, registers hold the tile in
// flight, fragment reads one step ahead), 16x16x4 MFMA tiles: lane l feeds A[l&15][k=l>>4] /
// B[k=l>>4][l&15]; the accumulator holds C[(l>>4)+4r][l&15], r=0..3 (the f64 map differs from
// every other MFMA shape, cdna_hip_programming.md "Fragment layout"). Bound: 78.6 TFLOP/s.
// Serves the reference's own tests, which run in float64 (tests/test_ops.py:311-323, (10,30)@(30,20)
// and up) and any f64 user; the fp32 headline never comes here.
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int LDP64 = 18;  // LDS row pad (doubles): transposing b64 stores of a half-wave hit 64 distinct banks; fragment reads overlap by 2 lanes

struct GemmArgs64 {
  const double *A, *B;
  double *C;
  int64_t M, N, K;
  int64_t a_bs, a_ms, a_ks, b_bs, b_ks, b_ns, c_bs, c_ms, c_ns;
  int tiles_m, tiles_n;
  int vec_ok;
};

template <int BM, int BN, int BK, int WM, int WN, bool A_KC, bool B_KC, bool EDGE>
__global__ void __launch_bounds__(64 * WM * WN) k_gemm_f64_mfma(GemmArgs64 g) {
  constexpr int NT = 64 * WM * WN;
  constexpr int WTM = BM / (16 * WM), WTN = BN / (16 * WN);
  __shared__ double As[2][BK][BM + LDP64];
  __shared__ double Bs[2][BK][BN + LDP64];
  const int nblk = g.tiles_m * g.tiles_n;
  MD_XCD_BID(bid, nblk)
  const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t bz = blockIdx.z;
  const double *A = g.A + bz * g.a_bs;
  const double *B = g.B + bz * g.b_bs;
  double *C = g.C + bz * g.c_bs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int l16 = lane & 15, h = lane >> 4;
  const bool vec_ok = g.vec_ok != 0;

  f64x4 acc[WTM][WTN];
  MD_ZERO_ACC(acc, WTM, WTN, 4)

  f64x2 ra[BM * BK / (2 * NT)], rb[BN * BK / (2 * NT)];
  const int64_t nk = (g.K + BK - 1) / BK;
  load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, 0, g.M, g.K, ra, vec_ok);
  load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, 0, g.N, g.K, rb, vec_ok);
  store_tile<BM, BK, NT, A_KC, LDP64>(As[0], ra);
  store_tile<BN, BK, NT, B_KC, LDP64>(Bs[0], rb);
  if (nk > 1) {
    load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, BK, g.M, g.K, ra, vec_ok);
    load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, BK, g.N, g.K, rb, vec_ok);
  }
  __syncthreads();

  // same schedule as the f32 kernel: branch-free k-tile body, a slice of the step's memory work behind every
  // MFMA, a tile's first fragments read right behind the barrier that publishes it
  int cur = 0;
  double fa[2][WTM], fb[2][WTN];
#pragma unroll
  for (int i = 0; i < WTM; ++i) fa[0][i] = As[0][h][wm * (WTM * 16) + i * 16 + l16];
#pragma unroll
  for (int j = 0; j < WTN; ++j) fb[0][j] = Bs[0][h][wn * (WTN * 16) + j * 16 + l16];
  for (int64_t kt = 0; kt < nk; ++kt) {
    const bool more2 = kt + 2 < nk;
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      const int c = (kk >> 2) & 1;
      if (kk + 4 < BK) {
#pragma unroll
        for (int i = 0; i < WTM; ++i) fa[c ^ 1][i] = As[cur][kk + 4 + h][wm * (WTM * 16) + i * 16 + l16];
#pragma unroll
        for (int j = 0; j < WTN; ++j) fb[c ^ 1][j] = Bs[cur][kk + 4 + h][wn * (WTN * 16) + j * 16 + l16];
      }
      if (kk == 0) store_tile<BM, BK, NT, A_KC, LDP64>(As[cur ^ 1], ra);
      if (kk == 4) store_tile<BN, BK, NT, B_KC, LDP64>(Bs[cur ^ 1], rb);
      if (kk == 8) {
        const int64_t ktl = more2 ? kt + 2 : nk - 1;
        load_tile<BM, BK, NT, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, ktl * BK, g.M, g.K, ra, vec_ok);
        load_tile<BN, BK, NT, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, ktl * BK, g.N, g.K, rb, vec_ok);
      }
#pragma unroll
      for (int i = 0; i < WTM; ++i)
#pragma unroll
        for (int j = 0; j < WTN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[c][i], fb[c][j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int m = 0; m < WTM * WTN; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (kk == 0 || kk == 4) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
        if (kk == 8) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
    }
    __syncthreads();
    cur ^= 1;
#pragma unroll
    for (int i = 0; i < WTM; ++i) fa[0][i] = As[cur][h][wm * (WTM * 16) + i * 16 + l16];
#pragma unroll
    for (int j = 0; j < WTN; ++j) fb[0][j] = Bs[cur][h][wn * (WTN * 16) + j * 16 + l16];
  }
  MD_STORE_C64(EDGE, acc, C, g, m0, n0, wm, wn, l16, h)
}

// ---- float64 TN on the direct-to-LDS scheme (round 3) -------------------------------------------------------------------
// Same idea as k_gemm_f32_tn_glds: `global_load_lds_dwordx4` moves 64 lanes x 16 B = 1 KiB = 128 doubles — ONE k-row of a
// 128-row tile — straight into LDS (no staging registers, no ds_write), one k-tile ahead, two separate buffers per operand with
// the buffer fixed at compile time (loop unrolled by two). 128 x 128 x 16 tiles, four waves (wave tile 64 x 64 = 4 x 4 MFMAs
// of v_mfma_f64_16x16x4_f64 per k-step, 128 accumulator registers), two blocks per CU (72 KiB of LDS each). k-rows sit
// 1152 B apart (pad 128 B: the four k of a fragment land on different banks) -> a fragment is one ds_read_b64 of S[k][row].
// Addresses: wave-uniform base (opaque to the optimiser: md_opaque_uniform) + loop-invariant 32-bit lane offset -> the DMA's
// `vN, s[base]` form (checked with scripts/isa_check.py: 16 / 16 per two k-tiles, no ds_write, no vmcnt(0) drain).
// Only the TN layout (both operands row-contiguous: the weight gradient A^T G): 4096^3 72.5-72.9 -> 73.4-75.5 TFLOP/s of 78.6.
// The k-contiguous image (16 rows x 8 k per piece, as in k_gemm_f32_kc_glds) was built and measured too: NN 67-70, NT 62-64
// against 73-74 for the register-staged kernel — a piece brings 64 B per row, half a cache line per DMA lane group — so NN / NT
// (and every ragged or unaligned shape) stay on k_gemm_f64_mfma (profiles/r3_gemm_f64.log).
constexpr int F64_TILE_LD = 128 + 16;   // doubles between the k-rows of an operand image
// k-row p (0..15) of a 128-row x 16-k operand tile whose first k is k0; `base` = operand + first row of the tile (+ batch)
__device__ __forceinline__ void glds64_krow(const double *base, int64_t ks, int64_t k0, double *S, int p, uint32_t lane_off) {
  const char *ub = md_opaque_uniform(reinterpret_cast<const char *>(base + (k0 + p) * ks));
  asm("" : "+v"(lane_off) : "s"((int)k0));   // (keeps the offset's zero-extension next to the DMA: see glds_tile_pass_u)
  __builtin_amdgcn_global_load_lds((md_gbl_void *)(ub + lane_off), (md_lds_void *)(S + p * F64_TILE_LD), 16, 0, 0);
}

__global__ void __launch_bounds__(256, 2) k_gemm_f64_tn_glds(GemmArgs64 g) {
  constexpr int BM = 128, BN = 128, BK = 16, WTM = 4, WTN = 4;
  __shared__ __attribute__((aligned(16))) double A0[BK * F64_TILE_LD];
  __shared__ __attribute__((aligned(16))) double A1[BK * F64_TILE_LD];
  __shared__ __attribute__((aligned(16))) double B0[BK * F64_TILE_LD];
  __shared__ __attribute__((aligned(16))) double B1[BK * F64_TILE_LD];
  const int nblk = g.tiles_m * g.tiles_n;
  MD_XCD_BID(bid, nblk)
  const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;
  const int64_t bz = blockIdx.z;
  const double *A = g.A + bz * g.a_bs + m0;
  const double *B = g.B + bz * g.b_bs + n0;
  double *C = g.C + bz * g.c_bs;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int l16 = lane & 15, h = lane >> 4;
  const uint32_t lo = (uint32_t)(lane * 16);

  f64x4 acc[WTM][WTN];
  MD_ZERO_ACC(acc, WTM, WTN, 4)

  const int64_t nk = g.K / BK;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    glds64_krow(A, g.a_ks, 0, A0, i * 4 + wave, lo);
    glds64_krow(B, g.b_ks, 0, B0, i * 4 + wave, lo);
  }
  __syncthreads();

  double fa[2][WTM], fb[2][WTN];
  // fragment of k-step s: lane (l16, h) supplies k = 4 s + h
#define MD_F64_READ(BUF, s, c)                                                                                                     \
  {                                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < WTM; ++i) fa[c][i] = ((BUF) ? A1 : A0)[(4 * (s) + h) * F64_TILE_LD + wm * 64 + i * 16 + l16]; \
    _Pragma("unroll") for (int j = 0; j < WTN; ++j) fb[c][j] = ((BUF) ? B1 : B0)[(4 * (s) + h) * F64_TILE_LD + wn * 64 + j * 16 + l16]; \
  }
  MD_F64_READ(0, 0, 0)
  auto ktile = [&](auto curc, int64_t kn) {
    constexpr int CUR = decltype(curc)::value;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = s & 1;
      if (s + 1 < 4) MD_F64_READ(CUR, s + 1, c ^ 1)
      if (s < 2) {   // the next tile's eight k-rows of this wave go out behind the first two k-steps
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          glds64_krow(A, g.a_ks, kn * BK, CUR ? A0 : A1, (2 * s + q) * 4 + wave, lo);
          glds64_krow(B, g.b_ks, kn * BK, CUR ? B0 : B1, (2 * s + q) * 4 + wave, lo);
        }
      }
#pragma unroll
      for (int i = 0; i < WTM; ++i)
#pragma unroll
        for (int j = 0; j < WTN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[c][i], fb[c][j], acc[i][j], 0, 0, 0);
#pragma unroll
      for (int m = 0; m < WTM * WTN; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        if (m < 8 && s + 1 < 4) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        if (s < 2 && m < 4) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
      }
    }
    __syncthreads();
    MD_F64_READ(CUR ^ 1, 0, 0)
  };
  MD_KTILE_ROTATE(2, nk, ktile)
#undef MD_F64_READ
  MD_STORE_C64(false, acc, C, g, m0, n0, wm, wn, l16, h)
}

// ======================= host side: plan, then run ===============================================================================
// plan_gemm lists what a product will run — repacks, kernel launches (layout, tile, staging, buffers, grid, arguments), split-order
// sums, hand-offs to skinny.hip (which decides for itself: the steps behind a hand-off run when it declines), the generic kernel —
// and the temporaries, allocating and launching nothing (the cached md_zero_block aside). run_plan allocates, launches, frees.

// 64 B of zeros in device memory for the ragged direct-to-LDS kernels (GemmArgs::zero); allocated once, never freed
static const float *md_zero_block() {
  static const float *z = [] {
    void *p = nullptr;
    if (hipMalloc(&p, 64) != hipSuccess || hipMemset(p, 0, 64) != hipSuccess) return (const float *)nullptr;
    return (const float *)p;
  }();
  return z;
}

// Three LDS buffers (DMA two k-tiles ahead, counted vmcnt at the k-tile boundary) for the 128-row direct-to-LDS tiles: when the grid
// gives a CU one block at most — the third buffer's 32 KiB cost nothing then, and such grids (2048^3, the 1024-row shards of an 8-rank
// cfg4, the all-reduce panels) are the ones whose k-tile (1.7 us) is about one DMA round trip: 2048^3 NN 132.9 -> 139.0, NT 132.7 ->
// 140.1 TFLOP/s (profiles/r3_gemm_nbuf_ab.log). Larger grids keep two buffers and two blocks per CU. option gemm_nbuf = 2 / 3 forces
// (A/B runs, exactness tests).
static bool md_gemm_nbuf3(int64_t blocks, int64_t K, int bk) {
  if (K < 2 * bk) return false;
  if (const int64_t f = md_opt(MD_OPT_GEMM_NBUF)) return f == 3;
  return blocks <= MD_NUM_CUS;
}

// Launch of a main GEMM kernel: with events attached (mdhip_event_attach_next, bench.py) the dispatch itself carries the start / stop
// timestamps — no marker packets around the kernel.
static void md_gemm_launch(void (*kernel)(GemmArgs), dim3 grid, int threads, const GemmArgs &ga) {
  hipEvent_t e0, e1;
  if (md_prof_take(&e0, &e1)) hipExtLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), 0, md_stream(), e0, e1, 0, ga);
  else hipLaunchKernelGGL(kernel, grid, dim3((unsigned)threads), 0, md_stream(), ga);
}

// diagnostic only (MDHIP_GEMM_STAMP=1): one persistent stamp buffer; what the last stamped launch wrote is printed at exit
struct StampDump {
  static constexpr size_t kMax = 8192;
  unsigned long long *dev = nullptr;
  int bm = 0, bn = 0, bk = 0;
  size_t blocks = 0;
  int64_t ktiles = 0;   // k-tiles of the stamped loop, where the launcher knows them (0: not reported)
  static StampDump &get() { static StampDump d; return d; }
  unsigned long long *buffer() {
    if (!dev) (void)hipMalloc((void **)&dev, kMax * 16);
    return dev;
  }
  void note(int m, int n, int k, size_t b, int64_t kt = 0) { bm = m; bn = n; bk = k; blocks = b; ktiles = kt; }
  ~StampDump() {
    if (!dev || !blocks) return;
    std::vector<unsigned long long> h(blocks * 2);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return;
    std::vector<double> ghz, us, cyc;
    for (size_t b = 0; b < blocks; ++b)
      if (h[2 * b + 1]) { ghz.push_back((double)h[2 * b] / (double)h[2 * b + 1] * 0.1); us.push_back((double)h[2 * b + 1] * 0.01); cyc.push_back((double)h[2 * b]); }
    std::sort(ghz.begin(), ghz.end());
    std::sort(us.begin(), us.end());
    std::sort(cyc.begin(), cyc.end());
    if (!ghz.empty())
      fprintf(stderr, "[mdhip] last gemm %dx%dx%d: in-kernel clock median %.3f GHz (min %.3f, max %.3f) over %zu blocks; block main loop median %.1f us (min %.1f, p10 %.1f, p90 %.1f, max %.1f)\n",
              bm, bn, bk, ghz[ghz.size() / 2], ghz.front(), ghz.back(), ghz.size(), us[us.size() / 2], us.front(), us[us.size() / 10], us[us.size() * 9 / 10], us.back());
    if (!cyc.empty() && ktiles > 0)
      fprintf(stderr, "[mdhip] last gemm %dx%dx%d: %lld k-tiles per block, shader cycles per k-tile and CU median %.0f (min %.0f, p10 %.0f, p90 %.0f, max %.0f)\n", bm, bn, bk,
              (long long)ktiles, cyc[cyc.size() / 2] / ktiles, cyc.front() / ktiles, cyc[cyc.size() / 10] / ktiles, cyc[cyc.size() * 9 / 10] / ktiles, cyc.back() / ktiles);
  }
};

// ---- the f32 tiles -------------------------------------------------------------------------------------------------------------------
// (128x128x32, 8-wave 256x128 and 256x256 tiles were measured and dropped: profiles/r1_gemm_tile_ab.log, r2_gemm_small_grid_ab.log)
enum { CFG_128x128x16 = 0, CFG_64x64x16, CFG_128x64x16, CFG_256x128x16, CFG_256x256x32, CFG_128x128x32, CFG_128x64x32, CFG_128x128_W8, CFG_COUNT };
struct Tile { int bm, bn, bk, wm, wn; };
// Per CFG and layout family ([0]: NN, NT, TT; [1]: TN): the register-staged tile, its direct-to-LDS form (bm = 0: none) and the
// model's full-grid rates in TFLOP/s (profiles/r1_gemm_tile_ab.log, r2_gemm_small_grid_ab.log, r2_gemm_glds_ab.log; both 0: not a
// candidate). TN's small tiles take 32-deep k-tiles to cover the latency of the tile staged two ahead (2048^3 TN: 106 -> 117); the
// k-contiguous layouts, held back by their transposing LDS stores, gain nothing. 16-deep 256x128 loses direct to LDS (135.7 -> 130.8).
// W8: eight waves on ONE 128x128 tile, two per SIMD from one block per CU, for grids of about one tile per CU: 2048^3 109-114 ->
// 118-123 TFLOP/s, 1024x4096x4096 114-118 -> 122-126 (profiles/r2_gemm_small_grid_ab.log).
struct TileCfg { Tile reg[2], dma[2]; double tf[2], tf_dma[2]; };
constexpr TileCfg kTiles[CFG_COUNT] = {
    /* 128x128x16 */ {{{128, 128, 16, 2, 2}, {128, 128, 16, 2, 2}}, {{128, 128, 32, 2, 2}, {}}, {133.0, 0.0}, {143.0, 0.0}},
    /* 64x64x16   */ {{{64, 64, 16, 2, 2}, {64, 64, 16, 2, 2}}, {{}, {}}, {120.0, 120.0}, {0.0, 0.0}},
    /* 128x64x16  */ {{{128, 64, 16, 2, 2}, {128, 64, 16, 2, 2}}, {{}, {}}, {126.0, 0.0}, {0.0, 0.0}},
    /* 256x128x16 */ {{{256, 128, 16, 2, 2}, {256, 128, 16, 2, 2}}, {{}, {}}, {139.0, 138.0}, {0.0, 0.0}},
    /* 256x256x32 */ {{{256, 128, 16, 2, 2}, {256, 256, 32, 2, 2}}, {{256, 256, 32, 2, 2}, {256, 256, 32, 2, 2}}, {0.0, 140.0}, {149.0, 150.0}},
    /* 128x128x32 */ {{{128, 128, 16, 2, 2}, {128, 128, 32, 2, 2}}, {{128, 128, 32, 2, 2}, {128, 128, 32, 2, 2}}, {0.0, 132.0}, {0.0, 146.0}},
    /* 128x64x32  */ {{{128, 64, 16, 2, 2}, {128, 64, 32, 2, 2}}, {{}, {128, 64, 32, 2, 2}}, {0.0, 126.7}, {0.0, 138.0}},
    /* W8         */ {{{128, 128, 16, 2, 4}, {128, 128, 32, 2, 4}}, {{128, 128, 32, 2, 4}, {128, 128, 32, 2, 4}}, {133.0, 134.0}, {143.5, 146.0}},
};
// the order in which the model weighs the candidates: ties go to the larger tile (listed first)
constexpr int kPickOrder[] = {CFG_256x256x32, CFG_256x128x16, CFG_128x128x16, CFG_128x128x32, CFG_128x128_W8, CFG_128x64x16, CFG_128x64x32, CFG_64x64x16};
// a third LDS buffer for a direct-to-LDS tile (md_gemm_nbuf3): the 128-row tiles have room for it, 256x256 does not
constexpr bool lds3_fits(Tile t) { return 3 * (t.bm + t.bn) * t.bk * 4 <= 128 * 1024; }

// `est` (optional): the model's time for the chosen tile, in units of 512 K / 1e12 seconds (rounds x BM x BN / TFLOP/s)
static int pick_cfg(int64_t M, int64_t N, int64_t K, int64_t batch, bool tn, bool dma_ok, double *est = nullptr) {
  if (est) *est = 64.0 * 64.0 / 120.0;   // (the early returns: one round of the small tile, split-K or not)
  {  // experiments / exactness tests only (option gemm_cfg)
    const int64_t v = md_opt(MD_OPT_GEMM_CFG);
    if (v >= 0 && v < CFG_COUNT) return (int)v;
  }
  // Cost model over the production tiles: a CU works through ceil(tiles / CUs) tiles of BM*BN outputs at the rate measured for that
  // tile — big tiles win on efficiency, small tiles on the partial last round of a grid that does not divide evenly (4097 rows: 3
  // rounds of 256x128 against 17 of 64x64, i.e. 0.80x the time). `dma_ok`: operands fit for the direct-to-LDS kernels
  // (dma_priced), whose rates apply to the tiles that have such a form.
  if (((M + 63) / 64) * ((N + 63) / 64) * batch < MD_NUM_CUS && K >= 1024) return CFG_64x64x16;  // split-K candidates
  int best = CFG_64x64x16;
  double best_t = 1e300;
  for (const int cfg : kPickOrder) {
    const TileCfg &c = kTiles[cfg];
    const bool dma = dma_ok && c.tf_dma[tn] > 0.0;   // (ragged sizes run the same kernels with zero-filled edges: plan_mfma checks what they need)
    const double tf = dma ? c.tf_dma[tn] : c.tf[tn];
    if (tf <= 0.0) continue;
    const Tile t = dma ? c.dma[tn] : c.reg[tn];
    const int64_t tiles = ((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn) * batch;
    double s = (double)((tiles + MD_NUM_CUS - 1) / MD_NUM_CUS) * t.bm * t.bn / tf;
    // a lone four-wave block per CU (one wave per SIMD) cannot keep the matrix pipe fed — except the 256x256 tile, whose rate was
    // measured that way (16 MFMAs per step and wave), and the eight-wave tile
    // (and the four-wave 128x128x32 direct-to-LDS tile of the TN layout: 127 against 119 TFLOP/s for the eight-wave one at 2048^3)
    if (tiles <= MD_NUM_CUS && cfg != CFG_128x128_W8 && cfg != CFG_256x256x32 && !(tn && dma && cfg == CFG_128x128x32)) s /= 0.8;
    if (cfg == CFG_256x256x32 && tiles < MD_NUM_CUS) continue;   // (half-empty chip: never the best choice)
    // the register-staged kernel's guarded edge variant runs ~15 % below its whole-tile rate (4000^3: 112-115 against 133-139);
    // the direct-to-LDS kernels pay nothing for a ragged edge (zero-filled DMA lanes)
    if (!dma && ((M % t.bm) || (N % t.bn) || (K % 16))) s /= 0.85;
    if (s < best_t * 0.999) { best_t = s; best = cfg; }
  }
  if (est && best_t < 1e299) *est = best_t;
  return best;
}

// ---- eligibility for the direct-to-LDS kernels -----------------------------------------------------------------------------------
// a kernel for the layout (NN / NT: k_gemm_f32_kc_glds, TN: k_gemm_f32_tn_glds; "TT" has none, plan_f32 swaps it into NN) with unit
// strides along the DMA'd vector axes; option gemm_glds = 0 keeps the register-staged kernels
template <class GA> static bool dma_family(const GA &ga, bool a_kc, bool b_kc) {
  return md_opt(MD_OPT_GEMM_GLDS) != 0 && (a_kc ? ga.a_ks == 1 : ga.a_ms == 1) && (b_kc ? ga.b_ks == 1 : ga.b_ns == 1) && (a_kc || !b_kc);
}
// every 16-B piece of a ragged tile lies wholly inside or outside its operand (or in a repack buffer's row padding: pad_m / pad_n)
static bool dma_pieces_whole(const GemmArgs &ga, bool a_kc, bool b_kc) {
  return ((a_kc || b_kc) ? ga.K % 4 == 0 : true) && (a_kc || ga.M % 4 == 0 || ga.pad_m) && (b_kc || ga.N % 4 == 0 || ga.pad_n);
}
// strides across the DMA'd rows: >= 0 (k-contiguous kernels) / > 0 (TN), and below `lim` where a lane's address part is a 32-bit byte
// offset of up to 15 rows / 3 k-rows (kLane32 f32 elements)
constexpr int64_t kLane32 = 1ll << 26;
template <class GA> static bool dma_strides(const GA &ga, bool a_kc, bool b_kc, int64_t lim) {
  if (a_kc) return ga.a_ms >= 0 && ga.b_ns >= 0 && ga.b_ks >= 0 && ga.a_ms < lim && (b_kc ? ga.b_ns : ga.b_ks) < lim;
  return ga.a_ks > 0 && ga.b_ks > 0 && ga.a_ks < lim && ga.b_ks < lim;
}
// what the cost model prices at the DMA rates — without the stride limits, which only the launch checks (plan_mfma, plan_epi)
static bool dma_priced(const GemmArgs &ga, bool a_kc, bool b_kc, bool aligned) {
  return aligned && dma_family(ga, a_kc, b_kc) && dma_pieces_whole(ga, a_kc, b_kc);
}
// ---- the plan --------------------------------------------------------------------------------------------------------------------------
enum { ST_REG, ST_DMA, ST_DMA_SELECT, ST_DMA_PRED };   // staging; the ragged DMA forms are the kernels' RAGGED = 1 (select) / 2 (predicated)
enum { S_LONGK, S_SKINNY, S_REPACK, S_F32, S_SUM, S_F64, S_GENERIC, S_NMFMA, S_NGENERIC, S_NCONV,   // S_N*: float16 / int8 / uint8 operands
       S_BX_CLEAR, S_BX_SPLIT_ROWS, S_BX_SPLIT_COLS, S_BX_GEMM };   // float32 on the bf16 matrix cores (gemm_bf16x3.hip): flag word, split passes, product
struct GemmStep {   // only the steps in use are initialised (GemmPlan::add)
  int kind, dtype, cfg, staging, nbuf, splits, epi, skip;   // cfg: kTiles row (S_F64: 0 64x64, 1 128x128, 2 TN direct to LDS); skip: hand-off
  int dtype_to;                                             // S_NCONV: the destination's dtype
  bool a_kc, b_kc, edge, ct, stamp, wide;                   // ct: C^T-vector stores (c_vec_rows); stamp: clock stamps (diagnostic);
                                                            // wide: narrow hand-offs / S_NMFMA / S_NGENERIC store the carrier (float32 / int32 c)
  Tile tile;
  dim3 grid;
  GemmArgs ga;
  GemmArgs64 ga64;
  MdGemm g;    // hand-offs, S_GENERIC, S_N*: the product; S_REPACK: a -> c, rows x cols = M x N, a_ms / c_ms row strides; S_SUM: K partials at a;
               // S_NCONV: a (dtype) -> c (dtype_to), batch x M x N with strides a_bs / a_ms / a_ks and c_bs / c_ms / c_ns
               // S_BX_*: b = the flag word; CLEAR: nothing else; SPLIT_*: a (M rows x K, a_ms the row / k-row stride) -> planes at c;
               // GEMM: planes at a, planes at b_planes, C at c with c_ms; SPLIT_* and GEMM: splits = the plane products (6 / 3 / 1)
  const void *b_planes;
  const char *what;
};
struct GemmPlan {
  static constexpr int kMaxSteps = 32, kMaxTmp = 12;   // (k ranges: 2 sub-products x (main + sum + 2 strips x (hand-off + main + sum)) + sum + 2 hand-offs = 19;
                                                       // a widened narrow product: 3 conversions around that, 3 more temporaries)
  GemmStep step[kMaxSteps];
  int n = 0;
  struct Tmp { size_t bytes; int first, last; } tmp[kMaxTmp];   // allocated before step `first`, freed after step `last` (-1: at the end)
  int ntmp = 0;
  GemmStep &add(int kind, const char *what = "") {
    GemmStep &s = step[n++] = GemmStep{};
    s.kind = kind; s.what = what; s.nbuf = 2; s.splits = 1;
    return s;
  }
  // temporary t is planned as a HANDLE, (t + 1) << 56 plus a byte offset: above user space, aligned like the allocation (pointer
  // arithmetic and alignment tests work on it); run_plan rebases it
  void *temp(size_t bytes, int first = -1) {
    tmp[ntmp] = {bytes, first < 0 ? n : first, -1};
    return (void *)((uintptr_t)++ntmp << 56);
  }
  void release_after_last_step(const void *h) { tmp[((uintptr_t)h >> 56) - 1].last = n - 1; }
};
// Split-order sum of `parts` partial products (both split-K forms): C[b][m][n] = sum over the parts, then the partials are freed
static void plan_sum(GemmPlan &p, const void *partial, int64_t parts, int64_t batch, int64_t M, int64_t N, void *c, int64_t c_bs, int64_t c_ms,
                     int64_t c_ns, const char *what) {
  p.add(S_SUM, what).g = MdGemm{batch, M, N, parts, partial, nullptr, c, 0, 0, 0, 0, 0, 0, c_bs, c_ms, c_ns};
  p.release_after_last_step(partial);
}
// tile counts and the XCD-compact band height (option gemm_super) of a tile over the product; -> the grid's x extent
static int64_t place(GemmArgs &ga, Tile t) {
  ga.tiles_m = (int)((ga.M + t.bm - 1) / t.bm);
  ga.tiles_n = (int)((ga.N + t.bn - 1) / t.bn);
  const int sh = (int)md_opt(MD_OPT_GEMM_SUPER);
  ga.super_h = (sh > 1 && ga.tiles_m >= sh && ga.tiles_n >= 8) ? sh : 0;
  return (int64_t)ga.tiles_m * ga.tiles_n;
}
static bool md_gemm_stamped(int64_t blocks) { return md_opt(MD_OPT_GEMM_STAMP) == 1 && blocks <= (int64_t)StampDump::kMax; }
// One f32 MFMA product: the tile, then the kernel that runs it.
static void plan_mfma(GemmPlan &p, GemmArgs ga, int64_t batch, bool a_kc, bool b_kc, bool aligned) {
  const bool tn = !a_kc && !b_kc, priced = dma_priced(ga, a_kc, b_kc, aligned);
  const int cfg = pick_cfg(ga.M, ga.N, ga.K, batch, tn, priced);
  GemmStep &s = p.add(S_F32, "matmul(f32 mfma)"); s.cfg = cfg; s.a_kc = a_kc; s.b_kc = b_kc;
  // NN / NT: k_gemm_f32_kc_glds when the tile has that form and the strides suit its lane offsets. A ragged tile needs the zero block
  // and, for NN, N a multiple of 4 (this kernel does not read a repacked B's padding: pad_n); otherwise the register-staged tile.
  const Tile d = kTiles[cfg].dma[0];
  if (a_kc && priced && d.bm && dma_strides(ga, true, b_kc, kLane32)) {
    const bool ragged = (ga.M % d.bm) || (ga.N % d.bn) || (ga.K % d.bk);
    if (!ragged || ((b_kc || ga.N % 4 == 0) && (ga.zero = md_zero_block()) != nullptr)) {
      const int64_t blocks = place(ga, d) * batch;
      s.tile = d; s.grid = dim3((unsigned)ga.tiles_m * ga.tiles_n, 1, (unsigned)batch);
      s.stamp = md_gemm_stamped(blocks);
      // whole k-tiles on the 128-row tiles: predicated lanes + scalar-base addresses (4100 x 4096 x 4100: 104-108 -> 112-124 TFLOP/s);
      // the 256x256 tile keeps the select form — the predicate's branch around each DMA splits its one scheduling region
      // (4000^3: 133-137 against 130 with the predicate)
      if (ragged) s.staging = (ga.K % d.bk == 0 && d.bm <= 128) ? ST_DMA_PRED : ST_DMA_SELECT;
      else { s.staging = ST_DMA; s.nbuf = lds3_fits(d) && md_gemm_nbuf3(blocks, ga.K, d.bk) ? 3 : 2; s.ct = !b_kc && ga.c_vec_rows; }
      s.ga = ga;
      return;
    }
  }
  const Tile t = s.tile = kTiles[cfg].reg[tn];
  const int64_t tiles = place(ga, t) * batch;
  ga.vec_ok = aligned; ga.k_chunk = ga.K;
  s.edge = !aligned || (ga.M % t.bm) || (ga.N % t.bn) || (ga.K % t.bk);
  // in-kernel split-K: a grid that cannot give every CU a block (skinny M or N with a long K, e.g. a 64 x 4096 batch through a
  // 4096 x 4096 layer) is widened along k over grid.y; >= 512 k per split (pick_cfg sends such shapes to 64x64)
  if (md_opt(MD_OPT_GEMM_SPLITK) && t.bm == 64 && t.bn == 64 && tiles < MD_NUM_CUS && ga.K >= 1024) {
    int64_t splits = (2 * MD_NUM_CUS + tiles - 1) / tiles;
    if (splits > ga.K / 512) splits = ga.K / 512;
    if (splits > 256) splits = 256;   // (64 until round 4: a single 64 x 64 output under k = 10^6 ran on 64 blocks, 13 TFLOP/s)
    if (splits > 1) {
      const int64_t n = batch * ga.M * ga.N;
      ga.k_chunk = ((ga.K + splits - 1) / splits + t.bk - 1) / t.bk * t.bk;
      splits = (ga.K + ga.k_chunk - 1) / ga.k_chunk;
      s.edge = s.edge || (ga.k_chunk % t.bk) || (ga.K % ga.k_chunk % t.bk);
      float *const c = ga.C;
      const int64_t c_bs = ga.c_bs, c_ms = ga.c_ms, c_ns = ga.c_ns;
      ga.C = (float *)p.temp((size_t)(splits * n) * sizeof(float), (int)(&s - p.step));   // (allocated before this launch)
      ga.c_bs = ga.M * ga.N; ga.c_ms = ga.N; ga.c_ns = 1; ga.c_split = n;
      s.splits = (int)splits; s.ga = ga;
      s.grid = dim3((unsigned)ga.tiles_m * ga.tiles_n, (unsigned)splits, (unsigned)batch);
      plan_sum(p, ga.C, splits, batch, ga.M, ga.N, c, c_bs, c_ms, c_ns, "matmul(f32 mfma, split-k)");
      return;
    }
  }
  s.grid = dim3((unsigned)ga.tiles_m * ga.tiles_n, 1, (unsigned)batch);
  s.stamp = !s.edge && md_gemm_stamped(tiles);
  if (tn && kTiles[cfg].dma[1].bm) {
    if (s.edge) {
      // ragged TN: still direct to LDS when every 16-B piece lies wholly inside or outside the operands; the select form takes any
      // positive strides, the predicated one (as on the k-contiguous kernel) 32-bit lane offsets
      if (aligned && dma_family(ga, false, false) && dma_pieces_whole(ga, false, false) && dma_strides(ga, false, false, INT64_MAX) &&
          (ga.zero = md_zero_block()) != nullptr)
        s.staging = (ga.K % t.bk == 0 && t.bm <= 128 && dma_strides(ga, false, false, kLane32)) ? ST_DMA_PRED : ST_DMA_SELECT;
    } else if (dma_family(ga, false, false) && !s.stamp && dma_strides(ga, false, false, kLane32)) {
      // whole tiles (stamped launches stay register-staged). Same-box A/B, profiles/r2_gemm_glds_ab.log: 256x256x32 at 4096^3
      // 140.1 -> 141.9 TFLOP/s, the 8-wave 128x128x32 at 2048^3 119.0 -> 127.8
      s.staging = ST_DMA;
      s.nbuf = lds3_fits(t) && md_gemm_nbuf3(tiles, ga.K, t.bk) ? 3 : 2;
    }
  }
  s.ga = ga;
}
// A product whose M and / or N are a few rows past a multiple of the big tile (x.T of a 4097-column matrix: 4097 x 4096 x 4100)
// pays for its ragged edge with a whole extra ROUND of tiles in a single launch (17 x 17 tiles of 256^2 for 256.3 tiles of work), or
// runs everything on small tiles. Peeled instead: the aligned main block [0, Mm) x [0, Nm) on the whole-tile kernels, the bottom strip
// [Mm, M) x [0, N) and the right strip [0, Mm) x [Nm, N) as two small products (a strip of up to eight rows / columns is a skinny
// product, skinny.hip; thin strips take the split-K route) — launches on one stream writing disjoint parts of C. Chosen by the same
// cost model as the tiles, when it beats the single launch by > 3 %.
static void plan_peeled(GemmPlan &p, const GemmArgs &ga, int64_t batch, bool a_kc, bool b_kc, bool aligned) {
  const int mode = (int)md_opt(MD_OPT_GEMM_PEEL);   // 0 never, 1 by the model, 2 whenever there is an edge to peel
  const int64_t G = 256;
  const int64_t Mm = ga.M / G * G, Nm = ga.N / G * G, Mr = ga.M - Mm, Nr = ga.N - Nm;
  if (mode == 0 || !aligned || (Mr == 0 && Nr == 0) || Mm == 0 || Nm == 0 || ga.K % 32) return plan_mfma(p, ga, batch, a_kc, b_kc, aligned);
  auto sub = [&](int64_t m0, int64_t m1, int64_t n0, int64_t n1) {
    GemmArgs x = ga;
    x.A = ga.A + m0 * ga.a_ms; x.B = ga.B + n0 * ga.b_ns; x.C = ga.C + m0 * ga.c_ms + n0 * ga.c_ns;
    x.M = m1 - m0; x.N = n1 - n0;
    if (x.c_vec_rows && (x.M % 4 || ((uintptr_t)x.C & 15))) x.c_vec_rows = 0;
    return x;
  };
  const GemmArgs main_blk = sub(0, Mm, 0, Nm), bottom = sub(Mm, ga.M, 0, ga.N), right = sub(0, Mm, Nm, ga.N);
  if (((uintptr_t)bottom.A & 15) || ((uintptr_t)right.B & 15)) return plan_mfma(p, ga, batch, a_kc, b_kc, aligned);   // (cannot happen for aligned operands: Mm, Nm are multiples of 256)
  if (mode == 1) {
    auto est = [&](const GemmArgs &x) { double t = 0; pick_cfg(x.M, x.N, x.K, batch, !a_kc && !b_kc, dma_priced(x, a_kc, b_kc, aligned), &t); return t; };
    const double launch = 6e-6 * 1e12 / (512.0 * (double)ga.K);   // ~6 us per extra launch (prologue / epilogue of a lone small kernel), in model units
    // the ragged single launch runs ~8 % under the model (4097 x 4096 x 4100: 112 TFLOP/s measured against 123 modelled)
    if (est(main_blk) + (Mr ? est(bottom) : 0) + (Nr ? est(right) : 0) + launch * ((Mr != 0) + (Nr != 0)) > 0.97 * (est(ga) / 0.92))
      return plan_mfma(p, ga, batch, a_kc, b_kc, aligned);
  }
  plan_mfma(p, main_blk, batch, a_kc, b_kc, aligned);
  for (const GemmArgs *x : {Mr ? &bottom : nullptr, Nr ? &right : nullptr}) {
    if (!x) continue;
    const int h = p.n;
    GemmStep &s = p.add(S_SKINNY);
    s.dtype = MDHIP_F32; s.g = MdGemm{batch, x->M, x->N, x->K, x->A, x->B, x->C, x->a_bs, x->a_ms, x->a_ks, x->b_bs, x->b_ks, x->b_ns, x->c_bs, x->c_ms, x->c_ns};
    plan_mfma(p, *x, batch, a_kc, b_kc, aligned);
    p.step[h].skip = p.n - h - 1;
  }
}
// Operand layout (f32 and f64; vec: elements per 16 B). a_kc / b_kc: vectorise A / B along k, else along m / n; mfma: unit strides
// and size fit the MFMA kernels; aligned: 16-B aligned operands whose vector axis' partner stride and batch steps keep rows aligned.
struct GemmLayout { bool mfma, a_kc, b_kc, aligned; };
static GemmLayout md_gemm_layout(const MdGemm &g, int vec) {
  const bool a_kc = g.a_ks == 1 || g.K == 1, a_mc = g.a_ms == 1 || g.M == 1;
  const bool b_kc = g.b_ks == 1 || g.K == 1, b_nc = g.b_ns == 1 || g.N == 1;
  GemmLayout L{g.M * g.N >= 64 * 64 && g.K >= 8 && (a_kc || a_mc) && (b_kc || b_nc) && g.M * g.N < (1ll << 40), a_kc && !(a_mc && g.a_ks != 1),
               b_kc && !(b_nc && g.b_ks != 1), false};
  const int64_t m = vec - 1;
  L.aligned = !((uintptr_t)g.a & 15) && !((uintptr_t)g.b & 15) && !((L.a_kc ? g.a_ms : g.a_ks) & m) && !((L.b_kc ? g.b_ns : g.b_ks) & m) &&
              !(g.a_bs & m) && !(g.b_bs & m);
  return L;
}
template <class GA> static void md_gemm_args(GA &ga, const MdGemm &g) {   // the product's operands and strides as kernel arguments
  ga.A = (decltype(ga.A))g.a; ga.B = (decltype(ga.B))g.b; ga.C = (decltype(ga.C))g.c;
  ga.M = g.M; ga.N = g.N; ga.K = g.K;
  ga.a_bs = g.a_bs; ga.a_ms = g.a_ms; ga.a_ks = g.a_ks; ga.b_bs = g.b_bs; ga.b_ks = g.b_ks; ga.b_ns = g.b_ns; ga.c_bs = g.c_bs; ga.c_ms = g.c_ms; ga.c_ns = g.c_ns;
}
static void plan_generic(GemmPlan &p, const MdGemm &g, int dtype) { GemmStep &s = p.add(S_GENERIC, "matmul(generic)"); s.g = g; s.dtype = dtype; }
// ---- float32 on the bf16 matrix cores (gemm_bf16x3.hip) ---------------------------------------------------------------------------
// Which products run as six bf16 products of pre-split planes (option gemm_bf16x3: 0 never | 1 above the floors | 2 every shape the
// kernels take whose fp32 plan is plain launches, see plan_bf16x3). Structure: batch 1, row-major C with unit column stride, both operands 16-B aligned with a unit stride along k or
// along their rows and the other stride a multiple of four, whole 256 x 128 x 32 tiles. The decision depends on M only through
// M >= 512 and divisibility (as plan_kranges' both-sides-at-most-2048 rule): a 512- or 1024-row panel of a product takes the route of
// the whole product, so panelled and un-panelled gradients stay bit-identical (every output element's bits are the same in both).
// Floors: the split passes stream 10 bytes per operand element and the 256 x 128 tiles must fill the chip; read off the option 0 / 2 sweep
// in profiles/gemm_bf16x3_after.txt so that no product with M >= 2048 loses (the 512- and 1024-row panels of such a product do).
// Option gemm_products (6 | 3 | 1, anything else 6) permits fewer products over fewer, rounded planes (k_gemm_bf16xp): the structure
// test and the form of the decision are the same in every mode; only the N and K floors are the mode's own. They are read off
// profiles/matmul_precision.txt by the same rule — the route must beat the default route of the shape (the six products from
// 4096, the fp32 plan below) at M = 2048 by more than the larger min - max spread: three products win at 2048^3 (94 against 125 us)
// and at neither 2048 x 1024 x 2048 nor 2048 x 2048 x 1024 (M x K x N); one product wins at K = 1024 too (43 against 66 us) and
// would at N = 1024 (58 against 91), but no N floor goes below 2048: 512 rows x 2048 columns are the 256 64 x 64 tiles from which
// the fp32 plan behind the product is one plain launch (plan_bf16x3), so the route cannot depend on M beyond the floor. The 512- and
// 1024-row panels lose under three products as they do under six (90 against 57 us at 512 x 2048 x 2048) and draw under one.
constexpr int64_t kBx3FloorN = 4096, kBx3FloorK = 4096;
constexpr int64_t kBxp3FloorN = 2048, kBxp3FloorK = 2048;   // gemm_products 3
constexpr int64_t kBxp1FloorN = 2048, kBxp1FloorK = 1024;   // gemm_products 1
static int bx_products() {
  const int64_t v = md_opt(MD_OPT_GEMM_PRODUCTS);
  return v == 3 || v == 1 ? (int)v : 6;
}
static bool bf16x3_takes(const MdGemm &g) {
  const int64_t mode = md_opt(MD_OPT_GEMM_BF16X3);
  if (mode == 0 || g.batch != 1 || g.c_ns != 1 || g.c_ms < g.N) return false;
  if (g.M < 256 || g.N < 128 || g.K < 32 || (g.M % 256) || (g.N % 128) || (g.K % 32)) return false;
  if (g.M > (1ll << 20) || g.N > (1ll << 20) || g.K > (1ll << 20)) return false;   // (grid extents, 32-bit lane offsets)
  auto side = [](const void *q, int64_t rows, int64_t K, int64_t rs, int64_t ks) {
    if ((uintptr_t)q & 15) return false;
    if (ks == 1) return rs >= K && rs % 4 == 0;
    return rs == 1 && ks >= rows && ks % 4 == 0;
  };
  if (!side(g.a, g.M, g.K, g.a_ms, g.a_ks) || !side(g.b, g.N, g.K, g.b_ns, g.b_ks)) return false;
  const int products = bx_products();
  const int64_t floor_n = products == 6 ? kBx3FloorN : products == 3 ? kBxp3FloorN : kBxp1FloorN;
  const int64_t floor_k = products == 6 ? kBx3FloorK : products == 3 ? kBxp3FloorK : kBxp1FloorK;
  return mode == 2 || (g.M >= 512 && g.N >= floor_n && g.K >= floor_k);
}
static void plan_f32(GemmPlan &p, const MdGemm &g_in, bool top = true);
// flag word = 0, split A, split B, the product, and behind it the fp32 plan of the same product with run_if_set: when a split pass
// met an inf or a NaN the product kernel returns at once and the fp32 kernels run (the fma chain's inf / NaN pattern, no host
// synchronisation); with finite operands the fp32 launches return at once. false: the fp32 plan is more than plain launches — a
// split-K launch with its sum, a k-range batch, a repack: steps with temporaries of their own that cannot be switched by the flag —
// and the product stays fp32. Such plans arise only from few 64 x 64 tiles under a long k (pick_cfg: < 256 tiles, K >= 1024) or
// misaligned operands, i.e. never above option 1's floors (M >= 512 and N >= 4096 are >= 512 such tiles, bf16x3_takes wants aligned
// operands, whole 256 x 128 tiles leave nothing to peel but 128-column strips the skinny hand-off declines); under option 2 a
// small shape may stay fp32 for this reason (tests/test_gemm_bf16x3.py pins both).
static bool plan_bf16x3(GemmPlan &p, const MdGemm &g) {
  GemmPlan q;
  plan_f32(q, g, false);
  if (q.ntmp || p.n + q.n + 4 > GemmPlan::kMaxSteps) return false;
  for (int i = 0; i < q.n; ++i) {
    const GemmStep &s = q.step[i];
    // (a hand-off in front of a peeled strip declines every strip of >= 128 rows and columns: md_gemm_skinny)
    if (!(s.kind == S_F32 && s.splits == 1 && !s.epi) && s.kind != S_SKINNY) return false;
  }
  const int products = bx_products(), nplanes = products == 6 ? 3 : products == 3 ? 2 : 1;
  const size_t a_bytes = (size_t)(nplanes * g.M * g.K) * 2, b_bytes = (size_t)(nplanes * g.N * g.K) * 2;
  char *buf = (char *)p.temp(256 + a_bytes + b_bytes);
  char *ap = buf + 256, *bp = ap + a_bytes;
  p.add(S_BX_CLEAR, "matmul(bf16x3 flag)").g.b = buf;
  const int layout = md_opt(MD_OPT_GEMM_BF16X3_PLANES) != 0;   // the plane image (md_bf16x3_layout.h), one for the three steps: GemmStep::cfg
  auto split = [&](const void *src, int64_t rows, int64_t rs, int64_t ks, void *dst) {
    GemmStep &st = p.add(ks == 1 ? S_BX_SPLIT_ROWS : S_BX_SPLIT_COLS, "matmul(bf16x3 split)");
    st.cfg = layout; st.splits = products;
    MdGemm &x = st.g;
    x.a = src; x.b = buf; x.c = dst; x.M = rows; x.K = g.K; x.a_ms = ks == 1 ? rs : ks;
  };
  split(g.a, g.M, g.a_ms, g.a_ks, ap);
  split(g.b, g.N, g.b_ns, g.b_ks, bp);
  GemmStep &m = p.add(S_BX_GEMM, "matmul(f32 as bf16x3)");
  m.g = g; m.g.a = ap; m.g.b = buf; m.b_planes = bp; m.cfg = layout; m.splits = products;
  for (int i = 0; i < q.n; ++i) {
    GemmStep &s = p.step[p.n++] = q.step[i];
    if (s.kind == S_F32) s.ga.run_if_set = (const unsigned *)buf;
  }
  return true;
}
// f32 past the hand-offs and the k ranges: bf16x3 (top: not for the sub-products of the k ranges), TT swap, repack, peel, MFMA; the
// generic kernel for what the MFMA kernels do not take
static void plan_f32(GemmPlan &p, const MdGemm &g_in, bool top) {
  if (top && bf16x3_takes(g_in) && plan_bf16x3(p, g_in)) return;
  MdGemm g = g_in;
  bool c_rows_unit = false;
  // "TT" (A^T B^T of two row-major arrays: A unit-stride along m, B along k) has no kernel of its own: C^T = B'A' is the NN
  // product of the two STORAGES (B' = N x K k-contiguous, A' = K x M row-contiguous), so it runs on the NN direct-to-LDS
  // kernels with the operands swapped and C addressed through swapped strides; the epilogue then holds four consecutive
  // elements of a C row per lane and stores them as one 16-B vector (c_vec_rows)
  if (md_opt(MD_OPT_GEMM_TT_SWAP) != 0 && g.a_ms == 1 && g.a_ks != 1 && g.b_ks == 1 && g.b_ns != 1 && g.M > 1 && g.N > 1 && g.K > 1) {
    g.a = g_in.b; g.b = g_in.a; g.M = g_in.N; g.N = g_in.M;
    g.a_bs = g_in.b_bs; g.a_ms = g_in.b_ns; g.a_ks = g_in.b_ks; g.b_bs = g_in.a_bs; g.b_ks = g_in.a_ks; g.b_ns = g_in.a_ms;
    g.c_ms = g_in.c_ns; g.c_ns = g_in.c_ms;
    c_rows_unit = g.c_ms == 1 && (g.c_ns & 3) == 0 && (g.c_bs & 3) == 0 && ((uintptr_t)g.c & 15) == 0 && g.M % 4 == 0;
  }
  const GemmLayout L = md_gemm_layout(g, 4);
  if (!L.mfma) return plan_generic(p, g, MDHIP_F32);
  GemmArgs ga{};  // (zero: no epilogue outputs, no diagnostic stamps)
  md_gemm_args(ga, g); ga.c_vec_rows = c_rows_unit ? 1 : 0;
  bool aligned = L.aligned;
  // Misaligned operands of a LARGE product (an odd leading dimension: x.T of a 4097-column matrix; a view that starts off a 16-B
  // boundary): one strided copy into an aligned buffer whose rows are padded to a multiple of four elements, then the direct-to-LDS
  // kernels — 4097 x 4096 x 4100 TN ran at 71 TFLOP/s on the register-staged edge kernel. Worth it when the product
  // is >= 50x the copy (2 M N K flop against 8 bytes per copied element).
  if (!aligned && md_opt(MD_OPT_GEMM_REPACK) != 0 && g.batch == 1 && (L.a_kc || L.b_kc ? g.K % 4 == 0 : true) && g.M >= 256 && g.N >= 256 && g.K >= 256) {
    // rows x cols, unit stride along cols -> rows x ld (ld = cols rounded up to 4; the padding stays unwritten)
    auto repack = [&](const float *src, int64_t rows, int64_t cols, int64_t row_stride, int64_t *ld) {
      *ld = (cols + 3) & ~(int64_t)3;
      void *dst = p.temp((size_t)(rows * *ld) * sizeof(float));
      MdGemm &r = p.add(S_REPACK, "matmul(repack)").g;
      r.a = src; r.c = dst; r.M = rows; r.N = cols; r.a_ms = row_stride; r.c_ms = *ld;
      return (const float *)dst;
    };
    if (((uintptr_t)g.a & 15) || ((L.a_kc ? g.a_ms : g.a_ks) & 3))
      ga.A = L.a_kc ? repack(ga.A, g.M, g.K, g.a_ms, &ga.a_ms) : (ga.pad_m = 1, repack(ga.A, g.K, g.M, g.a_ks, &ga.a_ks));
    if (((uintptr_t)g.b & 15) || ((L.b_kc ? g.b_ns : g.b_ks) & 3))
      ga.B = L.b_kc ? repack(ga.B, g.N, g.K, g.b_ns, &ga.b_ns) : (ga.pad_n = 1, repack(ga.B, g.K, g.N, g.b_ks, &ga.b_ks));
    aligned = true;
  }
  plan_peeled(p, ga, g.batch, L.a_kc, L.b_kc, aligned);
}
// A product whose output is a few dozen 128 x 128 tiles under a LONG k (the weight gradient of a 1000-wide layer over a 300,000-row
// batch: 64 tiles, a quarter of the chip, 32-52 TFLOP/s): k is cut into 2-4 ranges that run as the BATCH of one product (a_bs / b_bs
// step along k, c_bs from partial to partial), a second product takes the remainder, the partials are added in range order. The
// sub-products go to plan_f32: no hand-off can take them (t64 >= 256 with both sides <= 2048 puts both over 448: not long-k's <= 128,
// not skinny's <= 8), nor the k ranges again (a batch of >= 2 ranges, a remainder k < 128).
static bool kranges_shape(const MdGemm &g, int64_t *splits_out, int64_t *k_chunk_out) {
  const int64_t t128 = ((g.M + 127) / 128) * ((g.N + 127) / 128), t64 = ((g.M + 63) / 64) * ((g.N + 63) / 64);
  // (both sides at most 2048: the row panels dp.GradSync cuts a wide weight gradient into — 512 x 4096 — keep the plain product's
  // summation order, so panelled and un-panelled gradients stay bit-identical)
  if (!md_opt(MD_OPT_GEMM_SPLITK) || g.batch != 1 || t64 < MD_NUM_CUS || t128 > MD_NUM_CUS / 2 || g.M > 2048 || g.N > 2048 || g.K < 4096 ||
      g.K < 2 * (g.M > g.N ? g.M : g.N))
    return false;
  const int64_t splits = std::min<int64_t>(MD_NUM_CUS / t128, 4);
  const int64_t k_chunk = g.K / splits / 32 * 32;
  if (splits < 2 || k_chunk < 1024) return false;
  *splits_out = splits; *k_chunk_out = k_chunk;
  return true;
}
static bool plan_kranges(GemmPlan &p, const MdGemm &g) {
  int64_t splits, k_chunk;
  if (!kranges_shape(g, &splits, &k_chunk)) return false;
  const int64_t k_rem = g.K - splits * k_chunk;
  const int64_t parts = splits + (k_rem > 0 ? 1 : 0);
  float *partial = (float *)p.temp((size_t)(parts * g.M * g.N) * sizeof(float));
  MdGemm g2 = g;
  g2.batch = splits; g2.K = k_chunk; g2.a_bs = k_chunk * g.a_ks; g2.b_bs = k_chunk * g.b_ks;
  g2.c = partial; g2.c_bs = g.M * g.N; g2.c_ms = g.N; g2.c_ns = 1;
  plan_f32(p, g2, false);
  if (k_rem > 0) {
    MdGemm g3 = g2;
    g3.batch = 1; g3.K = k_rem;
    g3.a = (const float *)g.a + splits * k_chunk * g.a_ks; g3.b = (const float *)g.b + splits * k_chunk * g.b_ks; g3.c = partial + splits * g.M * g.N;
    plan_f32(p, g3, false);
  }
  plan_sum(p, partial, parts, 1, g.M, g.N, g.c, g.c_bs, g.c_ms, g.c_ns, "matmul(f32, k ranges as a batch)");
  return true;
}
static void plan_f64(GemmPlan &p, const MdGemm &g) {
  const GemmLayout L = md_gemm_layout(g, 2);
  if (!md_opt(MD_OPT_GEMM_F64_MFMA) || !L.mfma) return plan_generic(p, g, MDHIP_F64);
  GemmStep &s = p.add(S_F64, "matmul(f64 mfma)");
  s.a_kc = L.a_kc; s.b_kc = L.b_kc;
  GemmArgs64 &ga = s.ga64;
  md_gemm_args(ga, g);
  const int64_t t128 = ((g.M + 127) / 128) * ((g.N + 127) / 128) * g.batch;
  // TN, whole 128 x 128 tiles on a full chip: both operands direct to LDS (k_gemm_f64_tn_glds)
  if (!L.a_kc && !L.b_kc && L.aligned && dma_family(ga, false, false) && g.M % 128 == 0 && g.N % 128 == 0 && g.K % 16 == 0 && g.K >= 32 &&
      t128 >= MD_NUM_CUS && dma_strides(ga, false, false, kLane32 / 2)) {
    s.cfg = 2;
    ga.tiles_m = (int)(g.M / 128);
    ga.tiles_n = (int)(g.N / 128);
  } else {
    s.cfg = t128 >= 2 * MD_NUM_CUS ? 1 : 0;
    const int64_t bm = s.cfg ? 128 : 64;
    ga.tiles_m = (int)((g.M + bm - 1) / bm);
    ga.tiles_n = (int)((g.N + bm - 1) / bm);
    ga.vec_ok = L.aligned;
    s.edge = !L.aligned || (g.M % bm) || (g.N % bm) || (g.K % 16);
  }
  s.grid = dim3((unsigned)(ga.tiles_m * ga.tiles_n), 1, (unsigned)g.batch);
}
static void plan_gemm(GemmPlan &p, const MdGemm &g, int dtype) {
  // both sides thin and k long (np.dot of two vectors): k cut over the chip, fixed-order sum of the block partials (skinny.hip);
  // a thin side (matrix x vector, a few columns / rows): HBM-bound streaming kernels (skinny.hip)
  const int handoffs = dtype == MDHIP_F32 || dtype == MDHIP_F64 ? 2 : 1, h0 = p.n;   // (h0 > 0: the wide product of plan_widened)
  for (int h = 0; h < handoffs; ++h) {
    GemmStep &s = p.add(h ? S_SKINNY : S_LONGK);
    s.dtype = dtype; s.g = g;
  }
  // (a reduced mode's floors reach the k ranges' shapes — N = 2048 under K >= 4096, which M <= 1024 alone would send there: what
  // the reduced route takes stays off the k ranges, so that a row panel and its whole product keep one route)
  const bool reduced = dtype == MDHIP_F32 && bx_products() != 6 && bf16x3_takes(g);
  if (dtype == MDHIP_F32 && (reduced || !plan_kranges(p, g))) plan_f32(p, g);
  else if (dtype == MDHIP_F64) plan_f64(p, g);
  else if (dtype != MDHIP_F32) plan_generic(p, g, dtype);
  for (int h = h0; h < h0 + handoffs; ++h) p.step[h].skip = p.n - h - 1;
}
// ---- float16 / int8 / uint8 -------------------------------------------------------------------------------------------------------
// What the MFMA kernels of gemm_narrow.hip take, per operand: a unit-stride k axis (the KC image; K a multiple of the 16-B chunk) or a
// unit-stride row axis (the MN image; the rows a multiple of it), a 16-B aligned start, row / k-row and batch steps that are multiples of
// 16 B, and eight rows' step within a 32-bit lane offset.
struct NarrowLayout { bool ok, a_kc, b_kc, edge; };
static NarrowLayout md_narrow_layout(const MdGemm &g, int esz) {
  const int64_t epc = 16 / esz;
  auto side = [&](const void *p, int64_t rows, int64_t rs, int64_t ks, int64_t bs, bool *kc) {
    if (((uintptr_t)p & 15) || ((bs * esz) & 15)) return false;
    int64_t step;
    if (ks == 1 && g.K % epc == 0) { *kc = true; step = rs; }
    else if (rs == 1 && rows % epc == 0) { *kc = false; step = ks; }
    else return false;
    return step > 0 && !((step * esz) & 15) && step * esz * 8 < (1ll << 31);
  };
  NarrowLayout L{false, false, false, false};
  L.ok = side(g.a, g.M, g.a_ms, g.a_ks, g.a_bs, &L.a_kc) && side(g.b, g.N, g.b_ns, g.b_ks, g.b_bs, &L.b_kc);
  L.edge = (g.M % 128) || (g.N % 128) || (g.K % (128 / esz));
  return L;
}
// the shapes md_gemm_longk (skinny.hip) takes: few outputs under a long k
static bool md_longk_shape(const MdGemm &g) {
  const int64_t big = g.M > g.N ? g.M : g.N;
  return g.M <= 128 && g.N <= 128 && (big <= 8 ? g.K >= 512 : (g.K >= 8192 && g.K >= 64 * big));
}
// The route the product had before it ran natively — convert both operands to the wide type (float32 / int32: the same bits of the
// result), the wide plan with its hand-offs (skinny / long-k streaming kernels, split-k), convert the result back — for the shapes whose
// wide kernels beat one launch of the narrow ones: thin or long-k products, unaligned operands of a large float16 product.
// `keep_wide`: c has the wide type itself (plan_narrow's wide_out) — the wide plan writes straight into it, no conversion back.
static void plan_widened(GemmPlan &p, const MdGemm &g, int dtype, int wide, bool keep_wide = false) {
  const size_t wsz = md_dtype_size(wide);
  const int64_t ba = g.a_bs ? g.batch : 1, bb = g.b_bs ? g.batch : 1, M = g.M, N = g.N, K = g.K;
  auto conv = [&](const void *src, int from, int64_t nb, int64_t rows, int64_t cols, int64_t bs, int64_t rs, int64_t cs, void *dst, int to,
                  int64_t dbs, int64_t drs, int64_t dcs) {
    GemmStep &s = p.add(S_NCONV, "matmul(narrow, conversion)");
    s.dtype = from; s.dtype_to = to;
    s.g = MdGemm{nb, rows, cols, 0, src, nullptr, dst, bs, rs, cs, 0, 0, 0, dbs, drs, dcs};
  };
  MdGemm w = g;
  w.a = p.temp((size_t)(ba * M * K) * wsz);
  conv(g.a, dtype, ba, M, K, g.a_bs, g.a_ms, g.a_ks, const_cast<void *>(w.a), wide, M * K, K, 1);
  w.b = p.temp((size_t)(bb * K * N) * wsz);
  conv(g.b, dtype, bb, K, N, g.b_bs, g.b_ks, g.b_ns, const_cast<void *>(w.b), wide, K * N, N, 1);
  w.a_bs = ba > 1 ? M * K : 0; w.a_ms = K; w.a_ks = 1;
  w.b_bs = bb > 1 ? K * N : 0; w.b_ks = N; w.b_ns = 1;
  if (keep_wide) return plan_gemm(p, w, wide);
  w.c = p.temp((size_t)(g.batch * M * N) * wsz);
  w.c_bs = M * N; w.c_ms = N; w.c_ns = 1;
  plan_gemm(p, w, wide);
  conv(w.c, wide, g.batch, M, N, M * N, N, 1, g.c, dtype, g.c_bs, g.c_ms, g.c_ns);
}
// float16 / int8 / uint8: first the long-k and the thin hand-offs on the operands as they are (skinny.hip: few outputs under a long k, <= 8
// rows or columns; option gemm_narrow_skinny = 0: never). What they decline is planned as before them: the MFMA kernels
// (gemm_narrow.hip) for what they take, unless the product is thin (the float32 streaming kernels of skinny.hip after a conversion) or
// float16 of a few tiles under a long k (split-k in the wide plan); small or odd-stride products on the generic narrow kernel; the rest
// the widened route.
// `wide_out`: float16 @ float16 -> float32, int8 @ int8 -> int32 (`dtype`: the operands') — the same choices with the carrier kept: the
// wide-output MFMA / generic kernels of gemm_narrow.hip, or the widened route without its conversion back. The few-tile / long-k
// cut-over is the narrow output's fit (same k loop; the 4-byte C adds to the epilogue only): profiles/gemm_bench_widen_few_tiles.txt shows
// no shape slower than the conversion route beyond its run-to-run spread, so it was kept. Option gemm_widen = 0: the route a caller had
// before — convert both operands, the wide plan — for every wide-output product with a k.
static void plan_narrow_declined(GemmPlan &p, const MdGemm &g, int dtype, bool wide_out) {
  const int esz = dtype == MDHIP_F16 ? 2 : 1, wide = dtype == MDHIP_F16 ? MDHIP_F32 : MDHIP_I32;
  const NarrowLayout L = md_narrow_layout(g, esz);
  const int64_t blocks = ((g.M + 127) / 128) * ((g.N + 127) / 128) * g.batch;
  const bool native = !wide_out || md_opt(MD_OPT_GEMM_WIDEN) != 0;
  // A float16 product of a few tiles runs its whole k loop on a few CUs (no k split: ~10.4 us per 1024 of k, whatever the tile
  // count up to a full chip), the widened route splits k over the chip for ~25 us of fixed cost plus ~(1.6 + 0.5 tiles) us per 1024
  // of k (fit to profiles/gemm_bench_narrow_few_tiles_before.txt, NN / NT / TN of 128^2 .. 1024^2 x 1024 .. 8192): the wide route when it
  // is the faster one — 1 tile from k ~ 2.7 K, 4 tiles from ~3.4 K, 9 from ~5 K, never from 18 tiles on.
  const double kk = (double)g.K / 1024.0;
  const bool thin = g.M <= 8 || g.N <= 8, few_long = esz == 2 && kk * (8.8 - 0.5 * (double)blocks) > 22.5;
  if (native && L.ok && g.K > 0 && !thin && !few_long && !(esz == 1 && md_longk_shape(g))) {
    GemmStep &s = p.add(S_NMFMA, wide_out ? (esz == 2 ? "matmul(f16 -> f32 mfma)" : "matmul(i8 -> i32 mfma)") : (esz == 2 ? "matmul(f16 mfma)" : "matmul(i8 mfma)"));
    s.dtype = dtype; s.g = g; s.a_kc = L.a_kc; s.b_kc = L.b_kc; s.edge = L.edge; s.wide = wide_out;
    return;
  }
  const bool small = g.K <= 512 && g.batch * g.M * g.N * g.K <= (1ll << 22);
  // (int8 / uint8 ran on the generic int64 kernel before: the narrow one is the same loop on 1-byte loads; long-k shapes keep long-k)
  if (g.K == 0 || (native && (small || (esz == 1 && !md_longk_shape(g))))) {
    GemmStep &s = p.add(S_NGENERIC, wide_out ? "matmul(wide-output generic)" : "matmul(narrow generic)");
    s.dtype = dtype; s.g = g; s.wide = wide_out;
    return;
  }
  plan_widened(p, g, dtype, wide, wide_out);
}
static void plan_narrow(GemmPlan &p, const MdGemm &g, int dtype, bool wide_out) {
  // (gemm_widen = 0 asks for the route a wide-output product had before any native one: no hand-off either)
  const int handoffs = md_opt(MD_OPT_GEMM_NARROW_SKINNY) != 0 && g.K > 0 && (!wide_out || md_opt(MD_OPT_GEMM_WIDEN) != 0) ? 2 : 0;
  const int h0 = p.n;
  for (int h = 0; h < handoffs; ++h) {
    GemmStep &s = p.add(h ? S_SKINNY : S_LONGK);
    s.dtype = dtype; s.g = g; s.wide = wide_out;
  }
  plan_narrow_declined(p, g, dtype, wide_out);
  for (int h = h0; h < h0 + handoffs; ++h) p.step[h].skip = p.n - h - 1;
}
// ---- run ---------------------------------------------------------------------------------------------------------------------------
typedef void (*GemmKernel)(GemmArgs);
template <class F> static auto with_layout(bool a_kc, bool b_kc, F &&f) {   // f(A_KC, B_KC) as std::bool_constant
  if (a_kc) return b_kc ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  return b_kc ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}
// (C^T stores exist for NN only: CT = !B_KC names the plain kernel for NT)
template <int BM, int BN, int BK, int WM, int WN, bool B_KC> static GemmKernel kc_kernel(const GemmStep &s) {
  if (s.epi) { if constexpr (!B_KC) return k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 1>; else return nullptr; }
  if (s.staging == ST_DMA_SELECT) return k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 0, 1>;
  if (s.staging == ST_DMA_PRED) return k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 0, 2>;
  if (s.nbuf == 3) {
    if constexpr (!lds3_fits(Tile{BM, BN, BK, WM, WN})) return nullptr;
    else return (!B_KC && s.ct) ? k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 0, 0, 3, !B_KC> : k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 0, 0, 3>;
  }
  return (!B_KC && s.ct) ? k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC, 0, 0, 2, !B_KC> : k_gemm_f32_kc_glds<BM, BN, BK, WM, WN, B_KC>;
}
template <int BM, int BN, int BK, int WM, int WN> static GemmKernel tn_kernel(const GemmStep &s) {
  if (s.staging == ST_DMA_SELECT) return k_gemm_f32_tn_glds<BM, BN, BK, WM, WN, 1>;
  if (s.staging == ST_DMA_PRED) return k_gemm_f32_tn_glds<BM, BN, BK, WM, WN, 2>;
  if (s.nbuf == 3) { if constexpr (lds3_fits(Tile{BM, BN, BK, WM, WN})) return k_gemm_f32_tn_glds<BM, BN, BK, WM, WN, 0, 3>; else return nullptr; }
  return k_gemm_f32_tn_glds<BM, BN, BK, WM, WN>;
}
// The kernel of a planned f32 launch. Instantiates exactly what kTiles lists for the layout: nothing the plan cannot name.
template <int CFG, bool A_KC, bool B_KC> static GemmKernel cfg_kernel(const GemmStep &s) {
  constexpr bool TN = !A_KC && !B_KC;
  constexpr Tile R = kTiles[CFG].reg[TN], D = kTiles[CFG].dma[TN];
  constexpr int SCHED = R.bm == 64 ? 0 : 1;   // (the 64x64 tile has 2 MFMAs per step: nothing to interleave with; measured 6 % slower)
  if (s.staging != ST_REG) {
    if constexpr (D.bm != 0 && A_KC) return kc_kernel<D.bm, D.bn, D.bk, D.wm, D.wn, B_KC>(s);
    else if constexpr (D.bm != 0 && TN) return tn_kernel<D.bm, D.bn, D.bk, D.wm, D.wn>(s);
    else return nullptr;
  }
  if (s.splits > 1) {
    if constexpr (R.bm == 64 && R.bn == 64) return s.edge ? k_gemm_f32_mfma<64, 64, 16, 2, 2, A_KC, B_KC, true, true> : k_gemm_f32_mfma<64, 64, 16, 2, 2, A_KC, B_KC, false, true>;
    else return nullptr;
  }
  if (s.epi) { if constexpr (A_KC && !B_KC) return k_gemm_f32_mfma<R.bm, R.bn, R.bk, R.wm, R.wn, true, false, false, false, SCHED, 1>; else return nullptr; }
  return s.edge ? k_gemm_f32_mfma<R.bm, R.bn, R.bk, R.wm, R.wn, A_KC, B_KC, true> : k_gemm_f32_mfma<R.bm, R.bn, R.bk, R.wm, R.wn, A_KC, B_KC, false, false, SCHED>;
}
template <bool A_KC, bool B_KC, int... C> static GemmKernel f32_kernel(const GemmStep &s, std::integer_sequence<int, C...>) {
  GemmKernel k = nullptr;
  ((s.cfg == C ? (void)(k = cfg_kernel<C, A_KC, B_KC>(s)) : (void)0), ...);
  return k;
}
static GemmKernel f32_kernel(const GemmStep &s) {
  return with_layout(s.a_kc, s.b_kc, [&](auto a, auto b) { return f32_kernel<decltype(a)::value, decltype(b)::value>(s, std::make_integer_sequence<int, CFG_COUNT>{}); });
}
static int run_step(const GemmStep &s, const void *const *tmp, int *skip) {
  auto at = [&](auto q) {   // a planned pointer with its temporary's handle rebased
    const uintptr_t u = (uintptr_t)q;
    return (u >> 56) ? (decltype(q))((char *)tmp[(u >> 56) - 1] + (u & ((1ull << 56) - 1))) : q;
  };
  MdGemm g = s.g;
  g.a = at(g.a); g.b = at(g.b); g.c = at(g.c);
  switch (s.kind) {
    case S_LONGK:
    case S_SKINNY: {
      const int rc = s.kind == S_LONGK ? md_gemm_longk(g, s.dtype, s.wide) : md_gemm_skinny(g, s.dtype, s.wide);
      *skip = rc < 0 ? 0 : s.skip;
      return rc < 0 ? MDHIP_OK : rc;
    }
    case S_REPACK: {
      if (g.M <= 65535 * 4) {   // (a row per blockIdx.y group: no div / mod per element — the generic strided copy took 89 us for 4096 x 4097)
        k_repack_rows<<<dim3((unsigned)((g.N + 1023) / 1024), (unsigned)((g.M + 3) / 4)), 256, 0, md_stream()>>>((const float *)g.a, g.M, g.N, g.a_ms, (float *)g.c, g.c_ms);
        return MD_LAUNCH_CHECK(s.what);
      }
      mdhip_array sd{}, dd{};
      sd.data = const_cast<void *>(g.a); sd.dtype = MDHIP_F32; sd.ndim = 2; sd.shape[0] = g.M; sd.shape[1] = g.N; sd.strides[0] = g.a_ms; sd.strides[1] = 1;
      dd = sd; dd.data = g.c; dd.strides[0] = g.c_ms;
      return mdhip_unary(MDHIP_U_COPY, &sd, &dd);
    }
    case S_F32: {
      GemmArgs ga = s.ga;
      ga.A = at(ga.A); ga.B = at(ga.B); ga.C = at(ga.C); ga.partial = at(ga.partial); ga.run_if_set = at(ga.run_if_set);
      if (s.epi) ga.tickets = md_tickets();
      const GemmKernel k = f32_kernel(s);
      if (!k) return md_fail(MDHIP_ERUNTIME, "matmul: no kernel for the planned launch (cfg %d)", s.cfg);
      // persistent: no sync behind the launch, the LAST launch's stamps are printed at exit (not the stand-in's behind a bf16x3
      // product, which does not run: the product kernel's own stamps stay)
      const bool stamped = s.stamp && !ga.run_if_set;
      if (stamped) ga.stamp = StampDump::get().buffer();
      if (stamped) StampDump::get().note(s.tile.bm, s.tile.bn, s.tile.bk, (size_t)s.grid.x * s.grid.z);
      if (s.splits > 1) hipLaunchKernelGGL(k, s.grid, dim3(64u * s.tile.wm * s.tile.wn), 0, md_stream(), ga);   // (not the timed launch)
      else md_gemm_launch(k, s.grid, 64 * s.tile.wm * s.tile.wn, ga);
      return MD_LAUNCH_CHECK(s.what);
    }
    case S_SUM:
      k_gemm_splitk_sum<<<md_grid_for(g.batch * g.M * g.N), MD_BLOCK, 0, md_stream()>>>((const float *)g.a, (int)g.K, g.batch, g.M, g.N, (float *)g.c,
                                                                                         g.c_bs, g.c_ms, g.c_ns);
      return MD_LAUNCH_CHECK(s.what);
    case S_F64: {
      auto k = with_layout(s.a_kc, s.b_kc, [&](auto a, auto b) -> void (*)(GemmArgs64) {
        constexpr bool A = decltype(a)::value, B = decltype(b)::value;
        if (s.cfg == 1) return s.edge ? k_gemm_f64_mfma<128, 128, 16, 2, 2, A, B, true> : k_gemm_f64_mfma<128, 128, 16, 2, 2, A, B, false>;
        return s.edge ? k_gemm_f64_mfma<64, 64, 16, 2, 2, A, B, true> : k_gemm_f64_mfma<64, 64, 16, 2, 2, A, B, false>;
      });
      hipLaunchKernelGGL(s.cfg == 2 ? k_gemm_f64_tn_glds : k, s.grid, dim3(256), 0, md_stream(), s.ga64);
      return MD_LAUNCH_CHECK(s.cfg == 2 ? "matmul(f64 mfma, direct-to-LDS)" : s.what);
    }
    case S_NMFMA: {
      const void *zero = s.edge ? md_zero_block() : nullptr;
      if (s.edge && !zero) return md_fail(MDHIP_EMEMORY, "matmul: zero block");
      return s.wide ? md_gemm_widen_mfma(g, s.dtype, s.a_kc, s.b_kc, s.edge, zero) : md_gemm_narrow_mfma(g, s.dtype, s.a_kc, s.b_kc, s.edge, zero);
    }
    case S_BX_CLEAR: return md_hip_check(hipMemsetAsync(const_cast<void *>(g.b), 0, 4, md_stream()), s.what);
    case S_BX_SPLIT_ROWS:
    case S_BX_SPLIT_COLS:   // launched plainly, as the repack: attached events wait for the product
      return md_gemm_bf16x3_split((const float *)g.a, s.kind == S_BX_SPLIT_ROWS, g.M, g.K, g.a_ms, g.c, (unsigned *)const_cast<void *>(g.b), s.cfg,
                                  s.splits == 6 ? 3 : s.splits == 3 ? 2 : 1);
    case S_BX_GEMM: {
      // diagnostic (option gemm_stamp): the six-product kernel's stamped instantiation, into the persistent stamp buffer
      const int64_t tiles = (g.M / 256) * (g.N / 128);
      unsigned long long *stamp = s.splits == 6 && md_gemm_stamped(tiles) ? StampDump::get().buffer() : nullptr;
      if (stamp) StampDump::get().note(256, 128, 32, (size_t)tiles, g.K / 32);
      return md_gemm_bf16x3(g.a, at(s.b_planes), (float *)g.c, g.M, g.N, g.K, g.c_ms, (const unsigned *)g.b, (int)md_opt(MD_OPT_GEMM_BF16X3_LOOP), s.cfg,
                            (int)md_opt(MD_OPT_GEMM_BF16X3_BAND), s.splits, stamp);
    }
    case S_NGENERIC: return s.wide ? md_gemm_widen_generic(g, s.dtype) : md_gemm_narrow_generic(g, s.dtype);
    case S_NCONV: {
      mdhip_array sd{}, dd{};
      sd.data = const_cast<void *>(g.a); sd.dtype = s.dtype; sd.ndim = 3;
      sd.shape[0] = g.batch; sd.shape[1] = g.M; sd.shape[2] = g.N;
      sd.strides[0] = g.a_bs; sd.strides[1] = g.a_ms; sd.strides[2] = g.a_ks;
      dd = sd; dd.data = g.c; dd.dtype = s.dtype_to;
      dd.strides[0] = g.c_bs; dd.strides[1] = g.c_ms; dd.strides[2] = g.c_ns;
      return mdhip_convert(&sd, &dd);
    }
    case S_GENERIC: {
      const dim3 grid((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16), (unsigned)g.batch);
      if (grid.y > 65535) return md_fail(MDHIP_EVALUE, "matmul: M too large for the generic kernel");
      switch (s.dtype) {
        case MDHIP_F32: k_gemm_generic<float><<<grid, 256, 0, md_stream()>>>(g); break;
        case MDHIP_F64: k_gemm_generic<double><<<grid, 256, 0, md_stream()>>>(g); break;
        case MDHIP_I32: k_gemm_generic<int32_t><<<grid, 256, 0, md_stream()>>>(g); break;
        default: k_gemm_generic<int64_t><<<grid, 256, 0, md_stream()>>>(g); break;
      }
      return MD_LAUNCH_CHECK(s.what);
    }
  }
  return md_fail(MDHIP_ERUNTIME, "matmul: unknown plan step");
}
// Temporaries are allocated before their first step and freed (stream-ordered) after their last; a hand-off that takes its product
// skips the steps it replaces.
static int run_plan(const GemmPlan &p) {
  void *tmp[GemmPlan::kMaxTmp] = {};
  int rc = MDHIP_OK;
  for (int i = 0; i < p.n && rc == MDHIP_OK; ++i) {
    for (int t = 0; t < p.ntmp && rc == MDHIP_OK; ++t) if (p.tmp[t].first == i) rc = mdhip_alloc(p.tmp[t].bytes, &tmp[t]);
    int skip = 0;
    if (rc == MDHIP_OK) rc = run_step(p.step[i], tmp, &skip);
    for (int t = 0; t < p.ntmp; ++t) if (p.tmp[t].last == i && tmp[t]) { mdhip_free(tmp[t]); tmp[t] = nullptr; }
    i += skip;
  }
  for (int t = 0; t < p.ntmp; ++t) if (tmp[t]) mdhip_free(tmp[t]);
  return rc;
}
struct HipExec {
  template <class Plan> static int run(const MdGemm &g, Plan &&plan) {
    if (g.batch > 65535) return md_fail(MDHIP_EVALUE, "matmul: batch extent %lld exceeds 65535", (long long)g.batch);
    GemmPlan p; plan(p);
    return run_plan(p);
  }
  template <class T> static int gemm(const MdGemm &g) { return run(g, [&](GemmPlan &p) { plan_gemm(p, g, md_dtype_of<T>::value); }); }
  // float16 / int8 / uint8 (md_matmul_dispatch): the same planner, its narrow steps
  static int gemm_narrow(const MdGemm &g, int dtype) { return run(g, [&](GemmPlan &p) { plan_narrow(p, g, dtype, false); }); }
  // float16 -> float32, int8 -> int32 (md_matmul_dispatch; `dtype`: the operands')
  static int gemm_widen(const MdGemm &g, int dtype) { return run(g, [&](GemmPlan &p) { plan_narrow(p, g, dtype, true); }); }
};
// mdhip_matmul_bias_relu_sum: the plain product's tile choice (and summation order: a mask recomputed from `a @ b + bias` agrees bit
// for bit), restricted to tiles that divide the problem; the fused DMA kernel takes whole k-tiles only. false: not covered.
static bool plan_epi(GemmPlan &p, GemmArgs ga) {
  // The promise is kept by planning the plain product itself: covered only when that is ONE fp32 MFMA launch over all of k — not a
  // long-k hand-off, k ranges, in-kernel split-K, a peeled product (other orders of summation) or bf16x3 (no epilogue form of that
  // kernel is built) — and the fused kernel is of the same family (below): the caller's plain product and fused tail otherwise.
  bool plain_kc;
  {
    MdGemm g{1, ga.M, ga.N, ga.K, ga.A, ga.B, ga.C, 0, ga.a_ms, ga.a_ks, 0, ga.b_ks, ga.b_ns, 0, ga.c_ms, ga.c_ns};
    GemmPlan q;
    if (md_longk_shape(g) || plan_kranges(q, g)) return false;
    plan_f32(q, g);
    if (q.n != 1 || q.step[0].kind != S_F32 || q.step[0].splits != 1) return false;
    plain_kc = q.step[0].staging != ST_REG;   // k_gemm_f32_kc_glds (whole or ragged tiles): k pairs (0, 4), (1, 5), .. of every eight
  }
  const bool priced = dma_priced(ga, true, false, true) && ga.K % 32 == 0;
  const int cfg = pick_cfg(ga.M, ga.N, ga.K, 1, false, priced);
  auto divides = [&](Tile t) { return t.bm && ga.M % t.bm == 0 && ga.N % t.bn == 0; };
  const bool dma = priced && divides(kTiles[cfg].dma[0]);
  if (dma && !dma_strides(ga, true, false, kLane32)) return false;   // (a tile chosen at its DMA rate does not fall back)
  // the register-staged kernels feed the MFMA the k pairs (0, 1), (2, 3), ..: a register-staged epilogue under a plain product on the
  // direct-to-LDS kernel (K % 32 != 0, or a tile that does not divide the problem: its ragged forms) would round differently, and a
  // pre-activation within an ulp of 0 would get another mask bit than `a @ b + bias > 0` (tests/test_matmul_paths.py: test_epilogue)
  if (dma != plain_kc) return false;
  int row = dma ? cfg : -1;
  // else the register-staged tile of the choice, then smaller ones: 128x128 after 256x128, 128x64 after all but 64x64, 64x64
  for (const int c : {cfg, cfg == CFG_256x128x16 ? (int)CFG_128x128x16 : -1, cfg != CFG_64x64x16 ? (int)CFG_128x64x16 : -1, (int)CFG_64x64x16})
    if (row < 0 && c >= 0 && divides(kTiles[c].reg[0])) row = c;
  if (row < 0) return false;
  const Tile t = dma ? kTiles[row].dma[0] : kTiles[row].reg[0];
  const int64_t tiles = ((ga.M + t.bm - 1) / t.bm) * ((ga.N + t.bn - 1) / t.bn);
  ga.sum_out = ga.partial;  // (the caller parked the 0-d result pointer here)
  ga.partial = (float *)p.temp((size_t)tiles * sizeof(float));
  GemmStep &s = p.add(S_F32, dma ? "matmul(f32 mfma, direct-to-LDS)" : "matmul(f32 mfma, bias+relu epilogue)");
  s.cfg = row; s.a_kc = true; s.epi = 1; s.tile = t; s.staging = dma ? ST_DMA : ST_REG; s.grid = dim3((unsigned)tiles, 1, 1);
  place(ga, t);
  if (dma) s.stamp = md_gemm_stamped(tiles);
  else ga.vec_ok = 1;
  s.ga = ga;
  return true;
}

}  // namespace

extern "C" int mdhip_matmul(const mdhip_array *a, const mdhip_array *b, const mdhip_array *c) {
  return md_matmul_dispatch<HipExec>(a, b, c);
}

// sum_out = sum(where(a @ b + bias > 0, a @ b + bias, 0)) and mask_out = (a @ b + bias > 0), one GEMM pass with the
// elementwise tail and the reduction in its epilogue. MDHIP_EVALUE ("not fused") for anything but row-major f32
// a (M x K) and b (K x N) with whole aligned tiles: the caller then runs the plain product and the fused tail.
extern "C" int mdhip_matmul_bias_relu_sum(const mdhip_array *a, const mdhip_array *b, const mdhip_array *bias,
                                          const mdhip_array *mask_out, const mdhip_array *sum_out) {
  MD_TRY(md_check_array(a, "matmul a"));
  MD_TRY(md_check_array(b, "matmul b"));
  MD_TRY(md_check_array(bias, "bias"));
  MD_TRY(md_check_array(mask_out, "mask"));
  MD_TRY(md_check_array(sum_out, "sum"));
  if (a->dtype != MDHIP_F32 || b->dtype != MDHIP_F32 || bias->dtype != MDHIP_F32 || sum_out->dtype != MDHIP_F32 || mask_out->dtype != MDHIP_BOOL)
    return md_fail(MDHIP_ETYPE, "matmul_bias_relu_sum: float32 operands, bool mask, float32 sum");
  if (a->ndim != 2 || b->ndim != 2 || mask_out->ndim != 2 || bias->ndim != 1)
    return md_fail(MDHIP_EVALUE, "matmul_bias_relu_sum: 2-D operands and mask, 1-D bias");
  const int64_t M = a->shape[0], K = a->shape[1], N = b->shape[1];
  if (b->shape[0] != K || bias->shape[0] != N || mask_out->shape[0] != M || mask_out->shape[1] != N)
    return md_fail(MDHIP_EVALUE, "matmul_bias_relu_sum: shapes do not agree");
  const bool row_major = a->strides[1] == 1 && b->strides[1] == 1 && bias->strides[0] == 1 && mask_out->strides[1] == 1 && mask_out->strides[0] == N;
  auto al16 = [](const void *p) { return ((uintptr_t)p & 15) == 0; };
  // (the epilogue writes the mask in 16-byte vectors and reads the bias per column: an offset bool view or a short bias view
  // passed through the C-ABI must take the general path, not misaligned 16-byte stores)
  if (!row_major || !al16(a->data) || !al16(b->data) || !al16(mask_out->data) || ((uintptr_t)bias->data & 3) || (N & 15) ||
      (a->strides[0] & 3) || (b->strides[0] & 3) || K < 16 || (K % 16))
    return md_fail(MDHIP_EVALUE, "matmul_bias_relu_sum: layout not covered by the fused kernel");
  GemmArgs ga{};
  ga.A = (const float *)a->data; ga.B = (const float *)b->data; ga.C = nullptr;
  ga.M = M; ga.N = N; ga.K = K;
  ga.a_ms = a->strides[0]; ga.a_ks = 1; ga.b_ks = b->strides[0]; ga.b_ns = 1;
  ga.c_ms = N; ga.c_ns = 1;
  ga.bias = (const float *)bias->data;
  ga.mask = (uint8_t *)mask_out->data;
  ga.partial = (float *)sum_out->data;
  GemmPlan p;
  if (!plan_epi(p, ga)) return md_fail(MDHIP_EVALUE, "matmul_bias_relu_sum: shape not covered by the fused kernel");
  return run_plan(p);
}
