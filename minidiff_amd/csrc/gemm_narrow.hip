// gemm_narrow.hip — float16 @ float16 -> float16, int8 @ int8 -> int8 and uint8 @ uint8 -> uint8 on the low-precision matrix cores.
//
// Serves np.matmul / dot / tensordot (reference minidiff/backend/numpy.py:68,84,91) for the three storage-only pairs whose NumPy
// loop is the pair's own: float16 accumulates in float32 and rounds once, int8 / uint8 keep the low byte of the exact integer sum.
//   float16   v_mfma_f32_32x32x16_f16, f32 accumulator, round to nearest-even on the store (overflow -> +-inf, as NumPy's cast)
//   int8/u8   v_mfma_i32_32x32x32_i8, i32 accumulator, the low byte stored. uint8 runs on the same kernel: its bytes read as int8
//             give products congruent mod 256, and the i32 sum wraps mod 2^32, a multiple of 256 — bit-exact for any K.
// Both are planned by gemm.hip (plan_narrow) and launched from its run_plan; what these kernels do not take (tiny, thin, unaligned
// or odd-stride operands) runs on k_gemm_narrow_generic below or on the wide kernels after a conversion (gemm.hip).
//
// Block tile 128 x 128, four waves 2 x 2 (wave tile 64 x 64 = 2 x 2 MFMA tiles of 32 x 32), k-tile 128 BYTES of every operand row
// (64 k of float16, 128 k of int8): 4 MFMA k-steps per k-tile. Both operands go global -> LDS directly (global_load_lds_dwordx4,
// 64 lanes x 16 B = one 1-KiB piece per wave-instruction, 16 pieces per operand tile), two LDS buffers per operand as SEPARATE
// __shared__ objects with the k-loop unrolled by two (the buffer a fragment read uses is known at compile time: no vmcnt(0) drain
// in front of it, as in gemm.hip's direct-to-LDS f32 kernels). Whole-tile launches address a DMA as a wave-uniform scalar base plus
// a loop-invariant 32-bit lane offset; ragged launches (EDGE) point the lanes outside the operand at a zero block.
// Two LDS images, both lane-linear per piece (the DMA cannot scatter), swizzled through the per-lane SOURCE address:
//   KC  (the operand's k axis is contiguous: row-major A, B given as B^T) — [row][128 B]; 16-B chunk c of row r sits in slot
//       c ^ ((r >> 1) & 7). A fragment (lane: row r = lane & 31, k-half h = lane >> 5) is ONE ds_read_b128 of chunk 2s + h; the 16
//       lanes of a group hit 16 distinct 16-B bank slots.
//   MN  (the operand's row axis is contiguous: A^T, row-major B — the NN / TN / TT views) — [k][128 elements], read with the
//       hardware transpose reads: ds_read_b64_tr_b16 (4 k-rows x 16 columns per 16-lane group, two per float16 fragment) and
//       ds_read_b64_tr_b8 (8 k-rows x 16 columns, two per int8 fragment). float16: 256-B k-rows, slot c ^ (((r & 3) << 2) | ((r >> 2) & 3));
//       int8: 128-B k-rows, slot c ^ (((r >> 1) & 3) << 1) — conflict-free for the transposed reads of a 32-lane half.
// The k order inside one MFMA does not matter (A and B take element j of a lane from the same k): the KC read gives element j =
// k 8h + j (16h + j for int8) of step s, the transposed reads give the same k.
// Wide-output forms (np.matmul's dtype=: float16 -> float32, int8 -> int32; k_gemm_widen_mfma, k_gemm_widen_generic) share the tile
// loop and store the accumulators as they are. uint8 has none: the signed MFMA's sums are right modulo 256 only.
// int8 outputs leave through LDS: the accumulator layout holds one column per lane, so the bytes are assembled into the tile's rows
// in LDS first and stored as 16-B pieces of whole rows.
#include "md_hip.h"

namespace {

typedef __attribute__((address_space(3))) void nl_lds_void;
typedef __attribute__((address_space(1))) const void nl_gbl_void;
typedef _Float16 nl_f16x8 __attribute__((ext_vector_type(8)));
typedef short nl_i16x4 __attribute__((ext_vector_type(4)));
typedef int nl_i32x2 __attribute__((ext_vector_type(2)));
typedef int nl_i32x4 __attribute__((ext_vector_type(4)));
typedef float nl_f32x16 __attribute__((ext_vector_type(16)));
typedef int nl_i32x16 __attribute__((ext_vector_type(16)));

constexpr int NL_TILE = 128;   // block tile rows = columns
constexpr int NL_KB = 128;     // bytes of k per operand row and k-tile
constexpr int NL_NT = 256;     // threads (four waves)

struct NarrowArgs {
  const char *A, *B;
  char *C;
  int64_t M, N, K;
  int64_t a_bs, a_ms, a_ks, b_bs, b_ks, b_ns, c_bs, c_ms, c_ns;   // BYTE strides
  const char *zero;                                              // 16 B of zeros (EDGE launches)
  int tiles_m, tiles_n, c_vec;                                   // c_vec: C rows unit-stride, 16-B aligned (int8 row stores)
};

// byte offset of 16-B chunk `c` of row `r` in the two images (ESZ: element bytes of the MN image)
__device__ __forceinline__ int kc_off(int r, int c) { return r * NL_KB + ((c ^ ((r >> 1) & 7)) << 4); }
template <int ESZ> __device__ __forceinline__ int mn_off(int r, int c) {
  if constexpr (ESZ == 2) return r * 256 + ((c ^ (((r & 3) << 2) | ((r >> 2) & 3))) << 4);
  else return r * 128 + ((c ^ (((r >> 1) & 3) << 1)) << 4);
}

// wave-uniform address held in scalar registers, opaque to the optimiser (gemm.hip md_opaque_uniform: keeps the DMA in the
// `vN, s[base]` form)
__device__ __forceinline__ const char *nl_uniform(const char *p) {
  uint32_t lo = (uint32_t)(uintptr_t)p, hi = (uint32_t)((uintptr_t)p >> 32);
  asm("" : "+s"(lo), "+s"(hi));
  return reinterpret_cast<const char *>(((uintptr_t)hi << 32) | lo);
}

// Per-lane geometry of one DMA piece of an operand tile (piece p = wave + 4 i). KC: 8 rows x 128 B; MN float16: 4 k-rows x 256 B;
// MN int8: 8 k-rows x 128 B. `line`: the row (KC) / k-row (MN) of the lane within the piece, `chunk`: the SOURCE chunk it fetches.
template <int ESZ, bool KC> struct Piece {
  static constexpr int LINES = (KC || ESZ == 1) ? 8 : 4;
  static __device__ __forceinline__ void lane(int p, int l, int *line, int *chunk) {
    if constexpr (KC) { *line = l >> 3; *chunk = (l & 7) ^ (((p & 1) << 2) | ((l >> 3) >> 1)); }          // row 8p + line
    else if constexpr (ESZ == 2) { *line = l >> 4; *chunk = (l & 15) ^ (((l >> 4) << 2) | (p & 3)); }     // k-row 4p + line
    else { *line = l >> 3; *chunk = (l & 7) ^ ((((l >> 3) >> 1) & 3) << 1); }                           // k-row 8p + line
  }
};

// Stage one operand tile (rows row0.., k k0..) into S. `P`: the operand (batch applied), `rs` / `ks`: byte strides along rows / k,
// `R` / `K`: extents. Whole tiles: scalar base + 32-bit lane offset; EDGE: a lane outside the operand reads the zero block.
template <int ESZ, bool KC, bool EDGE>
__device__ __forceinline__ void stage(const char *P, int64_t rs, int64_t ks, int64_t row0, int64_t k0, int64_t R, int64_t K, char *S,
                                      const char *zero) {
  using PC = Piece<ESZ, KC>;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
  constexpr int EPC = 16 / ESZ;   // elements per 16-B chunk
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = wave + 4 * i;
    int line, c;
    PC::lane(p, l, &line, &c);
    const char *src;
    if constexpr (KC) {
      const int64_t r = row0 + PC::LINES * p + line, k = k0 + (int64_t)c * EPC;
      if constexpr (EDGE) src = (r < R && k < K) ? P + r * rs + k * ESZ : zero;
      else {
        uint32_t off = (uint32_t)(line * rs + (c << 4));
        asm("" : "+v"(off) : "s"((int)k0));
        src = nl_uniform(P + (row0 + PC::LINES * p) * rs + k0 * ESZ) + off;
      }
    } else {
      const int64_t kr = k0 + PC::LINES * p + line, r = row0 + (int64_t)c * EPC;
      if constexpr (EDGE) src = (kr < K && r < R) ? P + kr * ks + r * ESZ : zero;
      else {
        uint32_t off = (uint32_t)(line * ks + (c << 4));
        asm("" : "+v"(off) : "s"((int)k0));
        src = nl_uniform(P + (k0 + PC::LINES * p) * ks + row0 * ESZ) + off;
      }
    }
    __builtin_amdgcn_global_load_lds((nl_gbl_void *)src, (nl_lds_void *)(S + p * 1024), 16, 0, 0);
  }
}

// The 16-B MFMA operand of lane l for k-step s (0..3) and the 32 rows / columns from rb: KC -> ds_read_b128, MN -> two transposed reads.
template <int ESZ, bool KC> __device__ __forceinline__ nl_i32x4 frag(const char *S, int rb, int s) {
  const int l = threadIdx.x & 63;
  if constexpr (KC) {
    return *(const nl_i32x4 *)(S + kc_off(rb + (l & 31), 2 * s + (l >> 5)));
  } else if constexpr (ESZ == 2) {
    // group G = l >> 4: columns rb + 16 (G & 1) .., k-rows 16 s + 8 (G >> 1) + 4 t ..; lane 4q + p of the group supplies row q,
    // columns 4p .. 4p + 3 and receives column (l & 15), rows 0..3 in its elements 0..3
    const int G = l >> 4, q = (l >> 2) & 3, p = l & 3;
    const int col = rb + 16 * (G & 1) + 4 * p, r0 = 16 * s + 8 * (G >> 1) + q;
    const int c = col >> 3, in = (col & 7) * 2;
    const nl_i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nl_i16x4 *)(S + mn_off<2>(r0, c) + in));
    const nl_i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) nl_i16x4 *)(S + mn_off<2>(r0 + 4, c) + in));
    return __builtin_bit_cast(nl_i32x4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  } else {
    // group G: columns rb + 16 (G & 1) .., k-rows 32 s + 16 (G >> 1) + 8 t ..; lane 2q + p supplies row q, columns 8p .. 8p + 7 and
    // receives column (l & 15), rows 0..7 in its bytes 0..7
    const int G = l >> 4, q = (l >> 1) & 7, p = l & 1;
    const int col = rb + 16 * (G & 1) + 8 * p, r0 = 32 * s + 16 * (G >> 1) + q;
    const int c = col >> 4, in = col & 15;
    const nl_i32x2 lo = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) nl_i32x2 *)(S + mn_off<1>(r0, c) + in));
    const nl_i32x2 hi = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) nl_i32x2 *)(S + mn_off<1>(r0 + 8, c) + in));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3);
  }
}

template <int ESZ> struct Acc;
template <> struct Acc<2> { typedef nl_f32x16 type; };
template <> struct Acc<1> { typedef nl_i32x16 type; };

template <int ESZ, bool A_KC, bool B_KC>
__device__ __forceinline__ void mma_tile(const char *SA, const char *SB, int wm, int wn, typename Acc<ESZ>::type (&acc)[2][2]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    nl_i32x4 a[2], b[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) a[i] = frag<ESZ, A_KC>(SA, wm * 64 + i * 32, s);
#pragma unroll
    for (int j = 0; j < 2; ++j) b[j] = frag<ESZ, B_KC>(SB, wn * 64 + j * 32, s);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (ESZ == 2)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(nl_f16x8, a[i]), __builtin_bit_cast(nl_f16x8, b[j]), acc[i][j], 0, 0, 0);
        else
          acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
      }
  }
}

// The block's output tile (XCD-aware order, bijective for any tile count: the blocks that share an XCD take a contiguous band of
// output tiles) and its whole k loop, shared by the narrow-output and the wide-output kernels. ESZ 2: float16, 1: int8 / uint8.
// A_KC / B_KC: operand images (above). EDGE: ragged tiles (zero-filled DMA lanes). The four LDS buffers are the kernel's own objects.
template <int ESZ, bool A_KC, bool B_KC, bool EDGE>
__device__ __forceinline__ void narrow_tile_product(const NarrowArgs &g, char *sA0, char *sA1, char *sB0, char *sB1, int64_t *m0_out, int64_t *n0_out,
                                                    typename Acc<ESZ>::type (&acc)[2][2]) {
  const int nwg = g.tiles_m * g.tiles_n, bid = blockIdx.x, xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int64_t m0 = (int64_t)(wg / g.tiles_n) * NL_TILE, n0 = (int64_t)(wg % g.tiles_n) * NL_TILE;
  const int64_t bz = blockIdx.z;
  const char *A = g.A + bz * g.a_bs, *B = g.B + bz * g.b_bs;
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
  constexpr int BK = NL_KB / ESZ;
  const int nk = (int)((g.K + BK - 1) / BK);
  // KC operands: rows along m / n with stride *_ms / *_ns, k unit; MN operands: k-rows with stride *_ks, rows unit
  auto stage_ab = [&](int kt, char *SA, char *SB) {
    const int64_t k0 = (int64_t)kt * BK;
    stage<ESZ, A_KC, EDGE>(A, g.a_ms, g.a_ks, m0, k0, g.M, g.K, SA, g.zero);
    stage<ESZ, B_KC, EDGE>(B, g.b_ns, g.b_ks, n0, k0, g.N, g.K, SB, g.zero);
  };
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;
  stage_ab(0, sA0, sB0);
  for (int kt = 0; kt < nk; kt += 2) {
    __syncthreads();   // tile kt is in buffer 0 (the barrier's vmcnt(0) retires the DMAs); every wave is done with buffer 1
    if (kt + 1 < nk) stage_ab(kt + 1, sA1, sB1);
    mma_tile<ESZ, A_KC, B_KC>(sA0, sB0, wm, wn, acc);
    if (kt + 1 >= nk) break;
    __syncthreads();
    if (kt + 2 < nk) stage_ab(kt + 2, sA0, sB0);
    mma_tile<ESZ, A_KC, B_KC>(sA1, sB1, wm, wn, acc);
  }
  *m0_out = m0; *n0_out = n0;
}

// float16 -> float16 (rounded on the store), int8 / uint8 -> the low byte
template <int ESZ, bool A_KC, bool B_KC, bool EDGE>
__global__ void __launch_bounds__(NL_NT, 2) k_gemm_narrow_mfma(NarrowArgs g) {
  __shared__ __attribute__((aligned(16))) char sA0[16384];
  __shared__ __attribute__((aligned(16))) char sA1[16384];
  __shared__ __attribute__((aligned(16))) char sB0[16384];
  __shared__ __attribute__((aligned(16))) char sB1[16384];
  int64_t m0, n0;
  typename Acc<ESZ>::type acc[2][2];
  narrow_tile_product<ESZ, A_KC, B_KC, EDGE>(g, sA0, sA1, sB0, sB1, &m0, &n0, acc);
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, l = threadIdx.x & 63;
  const int64_t bz = blockIdx.z;
  // epilogue. accumulator element e of lane l: row (e & 3) + 8 (e >> 2) + 4 (l >> 5), column l & 31 of the 32 x 32 tile
  char *C = g.C + bz * g.c_bs;
  if constexpr (ESZ == 2) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (l >> 5), n = n0 + wn * 64 + j * 32 + (l & 31);
          if (!EDGE || (m < g.M && n < g.N)) *(_Float16 *)(C + m * g.c_ms + n * g.c_ns) = (_Float16)acc[i][j][e];
        }
  } else {
    __syncthreads();   // every wave is past its last fragment read: buffer sA0 takes the 128 x 128 byte tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e)
          sA0[(wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (l >> 5)) * NL_TILE + wn * 64 + j * 32 + (l & 31)] = (char)acc[i][j][e];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NL_TILE * NL_TILE / 16 / NL_NT; ++t) {
      const int idx = t * NL_NT + threadIdx.x, row = idx >> 3, ch = idx & 7;
      const int64_t m = m0 + row, n = n0 + ch * 16;
      if (m >= g.M) continue;
      if (g.c_vec && n + 16 <= g.N) {
        *(nl_i32x4 *)(C + m * g.c_ms + n) = *(const nl_i32x4 *)(sA0 + row * NL_TILE + ch * 16);
      } else {
        for (int b = 0; b < 16 && n + b < g.N; ++b) C[m * g.c_ms + (n + b) * g.c_ns] = sA0[row * NL_TILE + ch * 16 + b];
      }
    }
  }
}

// The wide-output form: float16 operands -> float32 C, int8 -> int32 C, the accumulators stored as they are (c_* are byte strides of
// the 4-byte C). One wave store writes 32 consecutive elements of two rows (lane & 31 = column): whole 128-B lines, no detour through LDS.
template <int ESZ, bool A_KC, bool B_KC, bool EDGE>
__global__ void __launch_bounds__(NL_NT, 2) k_gemm_widen_mfma(NarrowArgs g) {
  __shared__ __attribute__((aligned(16))) char sA0[16384];
  __shared__ __attribute__((aligned(16))) char sA1[16384];
  __shared__ __attribute__((aligned(16))) char sB0[16384];
  __shared__ __attribute__((aligned(16))) char sB1[16384];
  int64_t m0, n0;
  typename Acc<ESZ>::type acc[2][2];
  narrow_tile_product<ESZ, A_KC, B_KC, EDGE>(g, sA0, sA1, sB0, sB1, &m0, &n0, acc);
  const int wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1, l = threadIdx.x & 63;
  char *C = g.C + (int64_t)blockIdx.z * g.c_bs;
  typedef typename md_cond<ESZ == 2, float, int32_t>::type CT;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int64_t m = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (l >> 5), n = n0 + wn * 64 + j * 32 + (l & 31);
        if (!EDGE || (m < g.M && n < g.N)) *(CT *)(C + m * g.c_ms + n * g.c_ns) = acc[i][j][e];
      }
}

// ---- generic: any strides, any size (tiny products, odd strides) ---------------------------------------------------------------
// 16 x 16 output tiles; each operand read in its own type, the sum in k order in the carrier: float (fma chain) for float16, int32
// (wrapping) for int8 / uint8 — what NumPy's own loops compute.
// (TC: the type stored — the operands' own, or the carrier for the wide-output products)
template <class T, class Acc, class TC>
__device__ __forceinline__ void narrow_generic_product(const MdGemm &g) {
  __shared__ Acc As[16][17];
  __shared__ Acc Bs[16][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int64_t bz = blockIdx.z;
  const T *A = (const T *)g.a + bz * g.a_bs;
  const T *B = (const T *)g.b + bz * g.b_bs;
  TC *C = (TC *)g.c + bz * g.c_bs;
  const int64_t row = (int64_t)blockIdx.y * 16 + ty, col = (int64_t)blockIdx.x * 16 + tx;
  Acc acc = 0;
  for (int64_t k0 = 0; k0 < g.K; k0 += 16) {
    const int64_t ka = k0 + tx, kb = k0 + ty;
    As[ty][tx] = (row < g.M && ka < g.K) ? (Acc)A[row * g.a_ms + ka * g.a_ks] : (Acc)0;
    Bs[ty][tx] = (kb < g.K && col < g.N) ? (Acc)B[kb * g.b_ks + col * g.b_ns] : (Acc)0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if constexpr (md_is_float<Acc>::value) acc = fmaf(As[ty][k], Bs[k][tx], acc);
      else acc = (Acc)((uint32_t)acc + (uint32_t)As[ty][k] * (uint32_t)Bs[k][tx]);
    }
    __syncthreads();
  }
  if (row < g.M && col < g.N) C[row * g.c_ms + col * g.c_ns] = (TC)acc;
}
template <class T, class Acc>
__global__ void __launch_bounds__(256) k_gemm_narrow_generic(MdGemm g) { narrow_generic_product<T, Acc, T>(g); }
template <class T, class Acc>
__global__ void __launch_bounds__(256) k_gemm_widen_generic(MdGemm g) { narrow_generic_product<T, Acc, Acc>(g); }

template <bool WIDE, int ESZ, bool A, bool B> static void (*mfma_kernel(bool edge))(NarrowArgs) {
  if constexpr (WIDE) return edge ? k_gemm_widen_mfma<ESZ, A, B, true> : k_gemm_widen_mfma<ESZ, A, B, false>;
  else return edge ? k_gemm_narrow_mfma<ESZ, A, B, true> : k_gemm_narrow_mfma<ESZ, A, B, false>;
}

// WIDE: the 4-byte C of the wide-output kernels (uint8 has none: the signed MFMA's sums are right modulo 256 only)
template <bool WIDE> int launch_mfma(const MdGemm &g, int dtype, bool a_kc, bool b_kc, bool edge, const void *zero) {
  const int esz = dtype == MDHIP_F16 ? 2 : 1, csz = WIDE ? 4 : esz;
  NarrowArgs a{};
  a.A = (const char *)g.a; a.B = (const char *)g.b; a.C = (char *)g.c;
  a.M = g.M; a.N = g.N; a.K = g.K;
  a.a_bs = g.a_bs * esz; a.a_ms = g.a_ms * esz; a.a_ks = g.a_ks * esz;
  a.b_bs = g.b_bs * esz; a.b_ks = g.b_ks * esz; a.b_ns = g.b_ns * esz;
  a.c_bs = g.c_bs * csz; a.c_ms = g.c_ms * csz; a.c_ns = g.c_ns * csz;
  a.zero = (const char *)zero;
  a.tiles_m = (int)((g.M + NL_TILE - 1) / NL_TILE);
  a.tiles_n = (int)((g.N + NL_TILE - 1) / NL_TILE);
  a.c_vec = !WIDE && g.c_ns == 1 && !((uintptr_t)g.c & 15) && !(g.c_ms & 15) && !(g.c_bs & 15);
  void (*k)(NarrowArgs);
  if (esz == 2) k = a_kc ? (b_kc ? mfma_kernel<WIDE, 2, true, true>(edge) : mfma_kernel<WIDE, 2, true, false>(edge))
                         : (b_kc ? mfma_kernel<WIDE, 2, false, true>(edge) : mfma_kernel<WIDE, 2, false, false>(edge));
  else k = a_kc ? (b_kc ? mfma_kernel<WIDE, 1, true, true>(edge) : mfma_kernel<WIDE, 1, true, false>(edge))
                : (b_kc ? mfma_kernel<WIDE, 1, false, true>(edge) : mfma_kernel<WIDE, 1, false, false>(edge));
  MD_LAUNCH(k, dim3((unsigned)(a.tiles_m * a.tiles_n), 1, (unsigned)g.batch), NL_NT, a);
  if (WIDE) return MD_LAUNCH_CHECK(esz == 2 ? "matmul(f16 -> f32 mfma)" : "matmul(i8 -> i32 mfma)");
  return MD_LAUNCH_CHECK(esz == 2 ? "matmul(f16 mfma)" : "matmul(i8 mfma)");
}

}  // namespace

// launches planned by gemm.hip (plan_narrow, plan_widen): see md_hip.h
int md_gemm_narrow_mfma(const MdGemm &g, int dtype, bool a_kc, bool b_kc, bool edge, const void *zero) {
  return launch_mfma<false>(g, dtype, a_kc, b_kc, edge, zero);
}
int md_gemm_widen_mfma(const MdGemm &g, int dtype, bool a_kc, bool b_kc, bool edge, const void *zero) {
  if (dtype != MDHIP_F16 && dtype != MDHIP_I8) return md_fail(MDHIP_ETYPE, "matmul: no wide-output kernel for %s operands", md_dtype_name(dtype));
  return launch_mfma<true>(g, dtype, a_kc, b_kc, edge, zero);
}

int md_gemm_narrow_generic(const MdGemm &g, int dtype) {
  const dim3 grid((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16), (unsigned)g.batch);
  if (grid.y > 65535) return md_fail(MDHIP_EVALUE, "matmul: M too large for the generic kernel");
  switch (dtype) {
    case MDHIP_F16: k_gemm_narrow_generic<_Float16, float><<<grid, 256, 0, md_stream()>>>(g); break;
    case MDHIP_I8: k_gemm_narrow_generic<int8_t, int32_t><<<grid, 256, 0, md_stream()>>>(g); break;
    default: k_gemm_narrow_generic<uint8_t, int32_t><<<grid, 256, 0, md_stream()>>>(g); break;
  }
  return MD_LAUNCH_CHECK("matmul(narrow generic)");
}
int md_gemm_widen_generic(const MdGemm &g, int dtype) {
  const dim3 grid((unsigned)((g.N + 15) / 16), (unsigned)((g.M + 15) / 16), (unsigned)g.batch);
  if (grid.y > 65535) return md_fail(MDHIP_EVALUE, "matmul: M too large for the generic kernel");
  switch (dtype) {
    case MDHIP_F16: k_gemm_widen_generic<_Float16, float><<<grid, 256, 0, md_stream()>>>(g); break;
    case MDHIP_I8: k_gemm_widen_generic<int8_t, int32_t><<<grid, 256, 0, md_stream()>>>(g); break;
    default: return md_fail(MDHIP_ETYPE, "matmul: no wide-output kernel for %s operands", md_dtype_name(dtype));
  }
  return MD_LAUNCH_CHECK("matmul(wide-output generic)");
}
