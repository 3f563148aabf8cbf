// skinny.hip — matrix products with one THIN side: matrix x vector, vector x matrix, up to eight columns / rows, and the
// bottom / right strips of a peeled ragged product (gemm.hip, plan_peeled).
//
// Serves reference minidiff/backend/numpy.py:84 (np.matmul) as called by minidiff/ops/definitions.py:487-492 when an operand is a
// vector or a few columns wide. Such a product is HBM-bound — 2 flop per 4-byte element of the big operand, which is read exactly
// once — so the matrix cores have nothing to offer: on the 64x64 MFMA tiles + split-K these shapes ran at 22-30 % of the 8 TB/s
// peak (8192^2 x vector: 111-150 us for 256 MiB). Two streaming kernels instead, both computing
//
//     out[r][c] = sum_k X[r][k] * Y[k][c]        r < R (large), c < NC <= 8
//
// for whichever operand is the big one (a thin-M product is the thin-N product of the transposed problem: X = B^T, Y = A^T, out = C^T,
// all by strides):
//   k_skinny_rowdot   X unit-stride along k: a wave owns RW rows, lanes stride k with 16-B loads (1 KiB per wave and row), the
//                     thin operand's k-chunk sits in LDS as [c][k]; lane partials -> wave shuffle tree -> one store per output.
//   k_skinny_colsum   X unit-stride along r: a weighted column sum — a lane owns V neighbouring r, the block's four waves take
//                     interleaved k rows of one of NB bands, Y[k][c] arrive as wave-uniform (scalar) loads; band partials are
//                     published write-through and the block that arrives LAST at the strip's ticket adds them in band order
//                     (md_ticket.h): one launch, fixed order, bit-identical run to run.
// Algorithmic bytes: R * K * sizeof(T) per launch (the thin operand and the result are noise). float32 and float64.
//
// float16 / int8 / uint8 (the storage-only dtypes, planned by gemm.hip plan_narrow) run on the same kernels with a STORAGE type beside
// the compute type: X is read as it lies (16-B loads: 8 float16 or 16 bytes per lane), sums and partials live in the carrier (float32 /
// int32), results are stored in the operands' type (float16: one rounding to nearest even, overflow to inf; integers: the low byte) or
// as the carrier itself (float16 -> float32, int8 -> int32). The kernels take such a product as T = MdThin<S, O>. Its multiply-adds are
// the packed dot instructions (v_dot2c_f32_f16, v_dot4c_i32_i8: one instruction per dword of X and column), with the thin operand kept
// packed in its own type beside X; at 16 B per lane load a convert + fma per element would be at (float16) or over (int8) the vector
// issue rate at 8 columns. uint8 @ uint8 -> uint8 runs as int8: the low byte of a sum of products does not depend on how the operands'
// top bit is read.
#include <type_traits>

#include "md_hip.h"
#include "md_strips.h"

namespace {

template <class S_, class O_> struct MdThin {};   // in place of a kernel's T: operands stored as S_, results as O_
template <class T> struct SkT {                   // S storage, C compute / partials, O output; NARROW: the packed-dot forms
  typedef T S; typedef T C; typedef T O;
  static constexpr bool NARROW = false;
};
template <class S_, class O_> struct SkT<MdThin<S_, O_>> {
  typedef S_ S; typedef typename std::conditional<std::is_same<S_, _Float16>::value, float, int32_t>::type C; typedef O_ O;
  static constexpr bool NARROW = true;
};
typedef uint32_t sk_u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 sk_h2 __attribute__((ext_vector_type(2)));
// one dword of X against one dword of the thin operand, both in the storage type: two float16 or four int8 products onto acc
// (float16: every product is exact in float32; int8: the sum wraps modulo 2^32, unclamped)
template <class S> __device__ __forceinline__ auto sk_dot(uint32_t x, uint32_t y, typename SkT<MdThin<S, S>>::C acc) {
  if constexpr (std::is_same<S, _Float16>::value) return __builtin_amdgcn_fdot2(__builtin_bit_cast(sk_h2, x), __builtin_bit_cast(sk_h2, y), acc, false);
  else return __builtin_amdgcn_sdot4((int)x, (int)y, acc, false);
}
template <class S> __device__ __forceinline__ uint32_t sk_bits(S v) {   // an element's bits, zero-extended
  if constexpr (sizeof(S) == 2) return (uint32_t)__builtin_bit_cast(uint16_t, v);
  else return (uint32_t)(uint8_t)v;
}

struct SkinnyArgs {
  const void *X, *Y;
  void *out;
  int64_t R, K;
  int64_t xr, xk, x_bs;   // element strides of X[r][k] (one of xr / xk is 1), batch stride
  int64_t yk, yc, y_bs;   // Y[k][c]
  int64_t o_r, o_c, o_bs; // out[r][c]
  int nc;                 // live columns (<= NCT)
};

template <class T> __device__ __forceinline__ T md_readlane(T v, int l) {   // l: compile-time constant after unrolling
  if constexpr (sizeof(T) == 8) {
    union { T t; int w[2]; } u;
    u.t = v;
    u.w[0] = __builtin_amdgcn_readlane(u.w[0], l);
    u.w[1] = __builtin_amdgcn_readlane(u.w[1], l);
    return u.t;
  } else {
    union { T t; int w; } u;
    u.t = v;
    u.w = __builtin_amdgcn_readlane(u.w, l);
    return u.t;
  }
}

// ------------------------------------------------------------------------------------------------ X k-contiguous
// The thin operand goes through LDS in k-chunks of KC elements, [c][k] so that a lane reads its V consecutive k of one column as one
// 16-B ds_read. Two buffers: the global loads of chunk i + 1 are issued (into registers) before chunk i is multiplied and stored
// behind it, so their latency hides under the X stream; one barrier per chunk.
template <class TS, int NCT, int RW>
__global__ void __launch_bounds__(256) k_skinny_rowdot(SkinnyArgs a) {
  typedef typename SkT<TS>::S S;
  typedef typename SkT<TS>::C T;
  typedef typename SkT<TS>::O O;
  constexpr bool NARROW = SkT<TS>::NARROW;
  constexpr int V = 16 / sizeof(S);
  constexpr int E = NARROW ? 4 / sizeof(S) : 1;   // elements per staged unit: the packed forms stage and store whole dwords
  constexpr int KC = 4096 / sizeof(S);          // 4 KiB of k per column and buffer
  constexpr int KU = KC / E;
  constexpr int PER = NCT * KU / 256;           // staged units per thread and chunk
  constexpr int STEPS = KC / (64 * V);          // 16-B steps of a lane per chunk (4)
  typedef MdVec<S, V> Vec;
  typedef typename std::conditional<NARROW, uint32_t, S>::type Unit;
  __shared__ __attribute__((aligned(16))) S Ys[2][NCT][KC + V];   // (+ 16 B per row: the stores of one k for all c fall into different banks)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const S *X = (const S *)a.X + (int64_t)blockIdx.z * a.x_bs;
  const S *Y = (const S *)a.Y + (int64_t)blockIdx.z * a.y_bs;
  O *out = (O *)a.out + (int64_t)blockIdx.z * a.o_bs;
  const int64_t r0 = ((int64_t)blockIdx.x * 4 + w) * RW;
  const S *xp[RW];
#pragma unroll
  for (int i = 0; i < RW; ++i) {
    const int64_t r = r0 + i < a.R ? r0 + i : a.R - 1;   // rows past the end re-read the last row and store nothing
    xp[i] = X + r * a.xr;
  }
  T acc[RW][NCT];
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int c = 0; c < NCT; ++c) acc[i][c] = (T)0;
  const bool y_along_k = a.yk == 1;   // Y rows contiguous along k (a vector, a few k-contiguous rows): threads run along k; else along c
  // (packed forms) columns of Y that lie as whole 16-B pieces along k: staged four dwords at a time instead of element by element
  const bool y_vec = NARROW && y_along_k && ((uintptr_t)Y & 15) == 0 && (a.nc == 1 || ((a.yc * (int64_t)sizeof(S)) & 15) == 0);
  Unit stage[PER];
  auto fetch = [&](int64_t k0) {
    if constexpr (NARROW) {
      if (y_vec) {
        static_assert(!NARROW || PER % 4 == 0, "a thread stages whole 16-B pieces");
#pragma unroll
        for (int u = 0; u < PER / 4; ++u) {
          const int idx = threadIdx.x + u * 256;
          const int c = idx / (KC / V), k = idx % (KC / V) * V;
          sk_u32x4 v = {0u, 0u, 0u, 0u};
          if (k0 + k < a.K && c < a.nc) v = *reinterpret_cast<const sk_u32x4 *>(Y + (k0 + k) + c * a.yc);   // (K % V == 0: whole pieces)
          stage[4 * u] = v.x; stage[4 * u + 1] = v.y; stage[4 * u + 2] = v.z; stage[4 * u + 3] = v.w;
        }
        return;
      }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * 256;
      const int c = y_along_k ? idx / KU : idx % NCT, k = y_along_k ? idx % KU : idx / NCT;
      if constexpr (NARROW) {
        uint32_t v = 0;
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (k0 + k * E + e < a.K && c < a.nc) v |= sk_bits(Y[(k0 + k * E + e) * a.yk + c * a.yc]) << (8 * sizeof(S) * e);
        stage[u] = v;
      } else {
        stage[u] = (k0 + k < a.K && c < a.nc) ? Y[(k0 + k) * a.yk + c * a.yc] : (T)0;
      }
    }
  };
  auto put = [&](int buf) {
    if constexpr (NARROW) {
      if (y_vec) {
#pragma unroll
        for (int u = 0; u < PER / 4; ++u) {
          const int idx = threadIdx.x + u * 256;
          const int c = idx / (KC / V), k = idx % (KC / V) * V;
          *reinterpret_cast<sk_u32x4 *>(&Ys[buf][c][k]) = sk_u32x4{stage[4 * u], stage[4 * u + 1], stage[4 * u + 2], stage[4 * u + 3]};
        }
        return;
      }
    }
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * 256;
      const int c = y_along_k ? idx / KU : idx % NCT, k = y_along_k ? idx % KU : idx / NCT;
      if constexpr (NARROW) *reinterpret_cast<uint32_t *>(&Ys[buf][c][k * E]) = stage[u];
      else Ys[buf][c][k] = stage[u];
    }
  };
  fetch(0);
  put(0);
  __syncthreads();
  int buf = 0;
  for (int64_t k0 = 0; k0 < a.K; k0 += KC, buf ^= 1) {
    const bool more = k0 + KC < a.K;
    if (more) fetch(k0 + KC);
    const int kn = (int)(a.K - k0 < KC ? a.K - k0 : KC);
    Vec x[STEPS][RW];
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int k = st * 64 * V + lane * V;
      const int kk = k < kn ? k : 0;     // past the end of the last chunk: a valid address, multiplied by the zeros of the staged Y
#pragma unroll
      for (int i = 0; i < RW; ++i) x[st][i] = *reinterpret_cast<const Vec *>(xp[i] + k0 + kk);
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
      const int k = st * 64 * V + lane * V;
      if constexpr (NARROW) {
        sk_u32x4 xw[RW];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
          xw[i] = __builtin_bit_cast(sk_u32x4, x[st][i]);
          if (k >= kn) xw[i] = sk_u32x4{0u, 0u, 0u, 0u};   // (an inf or a NaN read past the end must not meet the staged zeros)
        }
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
          const sk_u32x4 y = *reinterpret_cast<const sk_u32x4 *>(&Ys[buf][c][k]);
#pragma unroll
          for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][c] = sk_dot<S>(xw[i][j], y[j], acc[i][c]);
        }
      } else {
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
          const Vec y = *reinterpret_cast<const Vec *>(&Ys[buf][c][k]);
#pragma unroll
          for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int j = 0; j < V; ++j) acc[i][c] = fma(x[st][i].v[j], y.v[j], acc[i][c]);
        }
      }
    }
    if (more) put(buf ^ 1);
    __syncthreads();
  }
  // lane partials -> lane 0, fixed tree
#pragma unroll
  for (int i = 0; i < RW; ++i)
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      T v = acc[i][c];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) v = BAdd::apply(v, md_shfl_down(v, d));
      acc[i][c] = v;
    }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < RW; ++i)
      if (r0 + i < a.R) {
#pragma unroll
        for (int c = 0; c < NCT; ++c)
          if (c < a.nc) out[(r0 + i) * a.o_r + c * a.o_c] = (O)acc[i][c];
      }
  }
}

// ------------------------------------------------------------------------------------------------ X r-contiguous
// The packed forms (T = MdThin): a dot instruction multiplies E = 2 / 4 neighbours ALONG K, which lie in different rows of X here. A
// batch's RB rows are regrouped in registers (v_perm_b32) into one dword per r holding its E rows, against E values of a column of Y packed the
// same way: lane q * NCT + c loads and packs rows q * E .. q * E + E - 1 of column c, one v_readlane per group and column hands the
// dword to the whole wave. Rows past a wave's last whole batch run as one more batch with zeros for the missing rows.
template <class S, int E> __device__ __forceinline__ void sk_regroup(const sk_u32x4 *rows, uint32_t *xg) {   // rows[E] (16 B of r each) -> xg[16 / sizeof(S)]
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if constexpr (E == 2) {
      xg[2 * d] = __builtin_amdgcn_perm(rows[1][d], rows[0][d], 0x05040100u);
      xg[2 * d + 1] = __builtin_amdgcn_perm(rows[1][d], rows[0][d], 0x07060302u);
    } else {
      const uint32_t lo01 = __builtin_amdgcn_perm(rows[1][d], rows[0][d], 0x05010400u), hi01 = __builtin_amdgcn_perm(rows[1][d], rows[0][d], 0x07030602u);
      const uint32_t lo23 = __builtin_amdgcn_perm(rows[3][d], rows[2][d], 0x05010400u), hi23 = __builtin_amdgcn_perm(rows[3][d], rows[2][d], 0x07030602u);
      xg[4 * d] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
      xg[4 * d + 1] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
      xg[4 * d + 2] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
      xg[4 * d + 3] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
    }
  }
}
template <class TS, int NCT, int RB>
__global__ void __launch_bounds__(256) k_skinny_colsum(SkinnyArgs a, int NS, int NB, TS *partial_, unsigned *tickets) {   // (partial_: carriers — TS itself unless TS = MdThin)
  typedef typename SkT<TS>::S S;
  typedef typename SkT<TS>::C T;
  T *const partial = (T *)partial_;
  typedef typename SkT<TS>::O O;
  constexpr bool NARROW = SkT<TS>::NARROW;
  constexpr int V = 16 / sizeof(S);
  typedef MdVec<S, V> XVec;
  typedef MdVec<T, V> Vec;
  typedef MdVec<O, V> OVec;
  __shared__ Vec sm[NARROW ? 1 : 3][NCT][64];   // (the packed forms hold 32 / 64 B of sums per lane and column: one wave's at a time)
  __shared__ unsigned last_flag;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x % NS, b = blockIdx.x / NS;
  const S *X = (const S *)a.X + (int64_t)blockIdx.z * a.x_bs;
  const S *Y = (const S *)a.Y + (int64_t)blockIdx.z * a.y_bs;
  O *out = (O *)a.out + (int64_t)blockIdx.z * a.o_bs;
  const int64_t col_raw = ((int64_t)s * 64 + lane) * V;
  const bool col_ok = col_raw < a.R;
  const int64_t col = col_ok ? col_raw : a.R - V;   // lanes past the edge load a valid vector and store nothing (R % V == 0, R >= V)
  const int64_t first = b + (int64_t)NB * w, step = (int64_t)NB * 4;   // this wave's k rows: first + step * i (interleaved across bands and waves)
  const int64_t nrw = first < a.K ? (a.K - first + step - 1) / step : 0;
  const int64_t nb = nrw / RB;
  T acc[NCT][V];
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[c][j] = (T)0;
  const S *p = X + col + first * a.xk;
  const int64_t rstep = step * a.xk;
  const S *yq = Y + first * a.yk;          // wave-uniform: the Y reads below are scalar loads
  const int64_t ystep = step * a.yk;
  if constexpr (NARROW) {
    constexpr int E = 4 / sizeof(S), Q = RB / E;
    static_assert(RB % E == 0 && Q * NCT <= 64, "a batch's packed Y values must fit one wave-wide load");
    sk_u32x4 t[2][RB];
    uint32_t ty[2];
    const int yg = lane / NCT, yc_ = lane % NCT;
    const bool y_lane = lane < Q * NCT && yc_ < a.nc;
    // rows i0 .. i0 + RB - 1 of this wave; `part`: only rows below nrw exist (the others count as zeros)
    auto load = [&](int buf, int64_t i0, auto part) {
#pragma unroll
      for (int u = 0; u < RB; ++u) {
        if (!decltype(part)::value || i0 + u < nrw) t[buf][u] = *reinterpret_cast<const sk_u32x4 *>(p + (i0 + u) * rstep);
        else t[buf][u] = sk_u32x4{0u, 0u, 0u, 0u};
      }
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int64_t i = i0 + yg * E + e;
        if (y_lane && (!decltype(part)::value || i < nrw)) v |= sk_bits(yq[i * ystep + yc_ * a.yc]) << (8 * sizeof(S) * e);
      }
      ty[buf] = v;
    };
    auto mac = [&](int buf) {
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        uint32_t xg[V];
        sk_regroup<S, E>(&t[buf][q * E], xg);
#pragma unroll
        for (int c = 0; c < NCT; ++c) {
          const uint32_t yv = md_readlane(ty[buf], q * NCT + c);
#pragma unroll
          for (int j = 0; j < V; ++j) acc[c][j] = sk_dot<S>(xg[j], yv, acc[c][j]);
        }
      }
    };
    if (nb > 0) {
      load(0, 0, std::false_type{});
      int64_t bt = 0;
      for (; bt + 1 < nb; bt += 2) {
        load(1, (bt + 1) * RB, std::false_type{});
        __builtin_amdgcn_sched_barrier(0);
        mac(0);
        __builtin_amdgcn_sched_barrier(0);
        load(0, (bt + 2 < nb ? bt + 2 : nb - 1) * RB, std::false_type{});   // a prefetch past the end re-reads the last batch (discarded)
        __builtin_amdgcn_sched_barrier(0);
        mac(1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (bt < nb) mac(0);
    }
    if (nb * RB < nrw) {
      load(0, nb * RB, std::true_type{});
      mac(0);
    }
  } else {
  XVec t[2][RB];
  T ty[2];   // the batch's RB x NCT values of Y, one per lane (lane = u * NCT + c): ONE vector load per batch, broadcast by v_readlane
  static_assert(RB * NCT <= 64, "a batch's Y values must fit one wave-wide load");
  const int yu = lane / NCT, yc_ = lane % NCT;
  const bool y_lane = lane < RB * NCT && yc_ < a.nc;
  auto load = [&](int buf, int64_t bt) {
    const int64_t i0 = (bt < nb ? bt : nb - 1) * RB;   // a prefetch past the end re-reads the last batch (discarded)
#pragma unroll
    for (int u = 0; u < RB; ++u) t[buf][u] = *reinterpret_cast<const XVec *>(p + (i0 + u) * rstep);
    ty[buf] = y_lane ? yq[(i0 + yu) * ystep + yc_ * a.yc] : (T)0;
  };
  auto mac = [&](int buf, int64_t) {
#pragma unroll
    for (int u = 0; u < RB; ++u) {
#pragma unroll
      for (int c = 0; c < NCT; ++c) {
        const T yv = md_readlane(ty[buf], u * NCT + c);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[c][j] = fma(t[buf][u].v[j], yv, acc[c][j]);
      }
    }
  };
  if (nb > 0) {
    load(0, 0);
    int64_t bt = 0;
    for (; bt + 1 < nb; bt += 2) {
      load(1, bt + 1);
      __builtin_amdgcn_sched_barrier(0);
      mac(0, bt);
      __builtin_amdgcn_sched_barrier(0);
      load(0, bt + 2);
      __builtin_amdgcn_sched_barrier(0);
      mac(1, bt + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (bt < nb) mac(0, bt);
  }
  for (int64_t i = nb * RB; i < nrw; ++i) {
    const XVec tt = *reinterpret_cast<const XVec *>(p + i * rstep);
    const T *yr = yq + i * ystep;
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const T yv = c < a.nc ? yr[c * a.yc] : (T)0;
#pragma unroll
      for (int j = 0; j < V; ++j) acc[c][j] = fma(tt.v[j], yv, acc[c][j]);
    }
  }
  }
  // waves 1..3 -> wave 0, in wave order (the packed forms: through one wave's worth of LDS, a wave at a time)
  auto fold_packed = [&]() {
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      if (q > 1) __syncthreads();
      if (w == q) {
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
          for (int j = 0; j < V; ++j) sm[0][c][lane].v[j] = acc[c][j];
      }
      __syncthreads();
      if (w == 0) {
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
          for (int j = 0; j < V; ++j) acc[c][j] = BAdd::apply(acc[c][j], sm[0][c][lane].v[j]);
      }
    }
  };
  if constexpr (NARROW) {
    fold_packed();
  } else {
    if (w > 0) {
#pragma unroll
      for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) sm[w - 1][c][lane].v[j] = acc[c][j];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
          for (int j = 0; j < V; ++j) acc[c][j] += sm[q][c][lane].v[j];
    }
  }
  auto store_out = [&]() {   // out[r][c], r = col + j
#pragma unroll
    for (int c = 0; c < NCT; ++c)
      if (c < a.nc) {
        if (a.o_r == 1) {
          OVec o;
#pragma unroll
          for (int j = 0; j < V; ++j) o.v[j] = (O)acc[c][j];
          O *dst = out + col + c * a.o_c;
          if (((uintptr_t)dst & 15) == 0) { *reinterpret_cast<OVec *>(dst) = o; continue; }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) out[(col + j) * a.o_r + c * a.o_c] = (O)acc[c][j];
      }
  };
  if (NB == 1) {
    if (w == 0 && col_ok) store_out();
    return;
  }
  // partial[z][b][c][r]
  const int64_t plane = (int64_t)NCT * a.R;
  T *pz = partial + (int64_t)blockIdx.z * NB * plane;
  const __amdgpu_buffer_rsrc_t pr = md_rsrc(pz, (unsigned)((int64_t)NB * plane * (int64_t)sizeof(T)));
  if (w == 0 && col_ok) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      Vec o;
#pragma unroll
      for (int j = 0; j < V; ++j) o.v[j] = acc[c][j];
      md_st16_sc1(pr, (unsigned)(((int64_t)b * plane + (int64_t)c * a.R + col) * (int64_t)sizeof(T)), o);
    }
  }
  if (!md_ticket_last(tickets + ((int64_t)blockIdx.z * NS + s) * MD_TICKET_PAD, (unsigned)NB, &last_flag)) return;
  // the strip's NB partial planes, band order: wave w takes bands w, w + 4, .. then the waves combine in wave order
#pragma unroll
  for (int c = 0; c < NCT; ++c)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[c][j] = (T)0;
  for (int r = w; r < NB; r += 4) {
#pragma unroll
    for (int c = 0; c < NCT; ++c) {
      const Vec pt = md_ld16_sc1<Vec>(pr, (unsigned)(((int64_t)r * plane + (int64_t)c * a.R + col) * (int64_t)sizeof(T)));
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if constexpr (md_is_float<T>::value) acc[c][j] += pt.v[j];
        else acc[c][j] = BAdd::apply(acc[c][j], pt.v[j]);   // (integers wrap)
      }
    }
  }
  __syncthreads();
  if constexpr (NARROW) {
    fold_packed();
    if (w == 0 && col_ok) store_out();
  } else {
    if (w > 0) {
#pragma unroll
      for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int j = 0; j < V; ++j) sm[w - 1][c][lane].v[j] = acc[c][j];
    }
    __syncthreads();
    if (w == 0 && col_ok) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
          for (int j = 0; j < V; ++j) acc[c][j] += sm[q][c][lane].v[j];
      store_out();
    }
  }
}

template <class T, int NCT> int launch_rowdot(const SkinnyArgs &a, int64_t batch) {
  constexpr int RWMAX = SkT<T>::NARROW && sizeof(typename SkT<T>::S) == 2 && NCT == 8 ? 2 : 4;   // (float16, 8 columns: four rows per wave spill)
  const int rw = a.R >= 8192 && RWMAX == 4 ? 4 : a.R >= 4096 ? 2 : 1;
  const dim3 grid((unsigned)((a.R + 4 * rw - 1) / (4 * rw)), 1, (unsigned)batch);
  if (rw == 4) MD_LAUNCH((k_skinny_rowdot<T, NCT, RWMAX>), grid, 256, a);   // (rw == 4 only where RWMAX is)
  else if (rw == 2) MD_LAUNCH((k_skinny_rowdot<T, NCT, 2>), grid, 256, a);
  else MD_LAUNCH((k_skinny_rowdot<T, NCT, 1>), grid, 256, a);
  if (SkT<T>::NARROW) md_opt_table()[MD_OPT_GEMM_NARROW_THIN_RUNS] += 1;
  return MD_LAUNCH_CHECK("matmul(skinny, row dot)");
}

template <class TS, int NCT> int launch_colsum(const SkinnyArgs &a, int64_t batch) {
  typedef typename SkT<TS>::C T;   // (the partials' type)
  constexpr int V = 16 / sizeof(typename SkT<TS>::S);
  const int64_t NS = (a.R + 64 * V - 1) / (64 * V);
  int64_t NB = md_strips_bands(NS * batch, 1024, MD_CEIL, a.K, 32);   // ~1024 blocks
  if (NB > 1 && NS * batch * MD_TICKET_PAD > MD_TICKET_WORDS) NB = 1;
  while (NB > 1 && NB * NCT * a.R * (int64_t)sizeof(T) >= (1ll << 31)) NB /= 2;   // (32-bit byte offsets into a batch's partial planes)
  void *partial = nullptr;
  if (NB > 1) MD_TRY(mdhip_alloc((size_t)(batch * NB * NCT * a.R) * sizeof(T), &partial));
  const dim3 grid((unsigned)(NS * NB), 1, (unsigned)batch);
  MD_LAUNCH((k_skinny_colsum<TS, NCT, 8>), grid, 256, a, (int)NS, (int)NB, (TS *)partial, md_tickets());
  if (SkT<TS>::NARROW) md_opt_table()[MD_OPT_GEMM_NARROW_THIN_RUNS] += 1;
  int rc = MD_LAUNCH_CHECK("matmul(skinny, weighted column sum)");
  if (partial) mdhip_free(partial);   // stream-ordered
  return rc;
}

template <class T> int skinny_run(const SkinnyArgs &a, int64_t batch, bool rowdot) {
#define MD_SK(NCT) (rowdot ? launch_rowdot<T, NCT>(a, batch) : launch_colsum<T, NCT>(a, batch))
  if (a.nc == 1) return MD_SK(1);
  if (a.nc == 2) return MD_SK(2);
  if (a.nc <= 4) return MD_SK(4);
  return MD_SK(8);
#undef MD_SK
}

}  // namespace

// ---- few outputs, k long: a dot product, (1,K)@(K,1), a few rows times a few columns, (64,K)@(K,64) ----------------------------
// A product with at most a few thousand outputs and k in the millions gives a tile kernel ONE block (or a handful) that walks k
// alone: 27-80 ns per k — a 4-million-element np.dot took 115 ms, (16, 2^20) @ (2^20, 16) 39 ms. Here k is cut over up to ~2048
// blocks: a block owns an (up to) 8 x 8 patch of the output and a k range, a thread strides that range and keeps the patch's
// partial sums, the block folds them (wave shuffles, then LDS), and a second small launch adds the block partials in block order —
// fixed order, bit-identical run to run. float32 / float64 / int32 / int64 (integers wrap as NumPy's).
namespace {
struct LongKArgs {
  const void *A, *B;
  void *C, *partial;
  int64_t K, chunk;
  int64_t a_bs, a_ms, a_ks, b_bs, b_ks, b_ns, c_bs, c_ms, c_ns;
  int M, N, nb, tiles_m, tiles_n;
};
template <class T> __device__ __forceinline__ T longk_mac(T acc, T x, T y) {
  if constexpr (md_is_float<T>::value) return x * y + acc;   // (contracted to an fma)
  else return BAdd::apply(acc, BMul::apply(x, y));            // integers wrap, as NumPy's
}
template <class TS, int TM, int TN>
__global__ void __launch_bounds__(MD_BLOCK) k_longk_partial(LongKArgs g) {
  typedef typename SkT<TS>::S S;   // (float16 / int8 operands are read as they lie and widened in registers)
  typedef typename SkT<TS>::C T;
  __shared__ T red[MD_BLOCK / 64][TM * TN];
  const int tiles = g.tiles_m * g.tiles_n, bz = blockIdx.y / tiles, tile = blockIdx.y - bz * tiles;
  const int m0 = (tile / g.tiles_n) * TM, n0 = (tile % g.tiles_n) * TN;
  const S *A = (const S *)g.A + (int64_t)bz * g.a_bs + (int64_t)m0 * g.a_ms;
  const S *B = (const S *)g.B + (int64_t)bz * g.b_bs + (int64_t)n0 * g.b_ns;
  const int mm = g.M - m0, nn = g.N - n0;   // live rows / columns of this patch
  const int64_t k0 = (int64_t)blockIdx.x * g.chunk, k1 = k0 + g.chunk < g.K ? k0 + g.chunk : g.K;
  T acc[TM][TN];
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) acc[m][n] = T(0);
  for (int64_t k = k0 + threadIdx.x; k < k1; k += MD_BLOCK) {
    T a[TM], b[TN];
#pragma unroll
    for (int m = 0; m < TM; ++m) a[m] = m < mm ? (T)A[m * g.a_ms + k * g.a_ks] : T(0);
#pragma unroll
    for (int n = 0; n < TN; ++n) b[n] = n < nn ? (T)B[k * g.b_ks + n * g.b_ns] : T(0);
#pragma unroll
    for (int m = 0; m < TM; ++m)
#pragma unroll
      for (int n = 0; n < TN; ++n) acc[m][n] = longk_mac<T>(acc[m][n], a[m], b[n]);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < TM; ++m)
#pragma unroll
    for (int n = 0; n < TN; ++n) {
      T v = acc[m][n];
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) v = BAdd::apply(v, (T)__shfl_down(v, d, 64));
      if (lane == 0) red[w][m * TN + n] = v;
    }
  __syncthreads();
  if (threadIdx.x < TM * TN) {
    T v = red[0][threadIdx.x];
#pragma unroll
    for (int ww = 1; ww < MD_BLOCK / 64; ++ww) v = BAdd::apply(v, red[ww][threadIdx.x]);
    ((T *)g.partial)[((int64_t)blockIdx.y * g.nb + blockIdx.x) * (TM * TN) + threadIdx.x] = v;
  }
}
// one block per patch: the 256 threads split into G = 256 / (TM TN) groups, group q adds the partials of blocks q, q + G, q + 2G, ..
// for its output (independent loads; one thread walking 2048 dependent ones took 80 us), then the group sums are added in group
// order — a fixed order, so the result is bit-identical run to run
template <class TS, int TM, int TN>
__global__ void __launch_bounds__(MD_BLOCK) k_longk_finish(LongKArgs g) {
  typedef typename SkT<TS>::C T;
  typedef typename SkT<TS>::O O;
  constexpr int P = TM * TN, G = MD_BLOCK / P;
  __shared__ T sums[G][P];
  const int tiles = g.tiles_m * g.tiles_n, bz = blockIdx.x / tiles, tile = blockIdx.x - bz * tiles;
  const int p = threadIdx.x % P, q = threadIdx.x / P;
  const T *part = (const T *)g.partial + (int64_t)blockIdx.x * g.nb * P;
  if (q < G) {
    T v = T(0);
    for (int b = q; b < g.nb; b += G) v = BAdd::apply(v, part[(int64_t)b * P + p]);
    sums[q][p] = v;
  }
  __syncthreads();
  if (threadIdx.x < P) {
    const int m = (tile / g.tiles_n) * TM + threadIdx.x / TN, n = (tile % g.tiles_n) * TN + threadIdx.x % TN;
    if (m < g.M && n < g.N) {
      T v = sums[0][threadIdx.x];
      for (int qq = 1; qq < G; ++qq) v = BAdd::apply(v, sums[qq][threadIdx.x]);
      ((O *)g.C)[(int64_t)bz * g.c_bs + (int64_t)m * g.c_ms + (int64_t)n * g.c_ns] = (O)v;
    }
  }
}
template <class TS, int TM, int TN> int longk_run(LongKArgs a, int64_t batch) {
  typedef typename SkT<TS>::C T;
  a.tiles_m = (a.M + TM - 1) / TM;
  a.tiles_n = (a.N + TN - 1) / TN;
  const int64_t patches = batch * a.tiles_m * a.tiles_n;
  if (patches > 65535) return -1;
  // blocks of >= 4096 k each (sixteen trips of the 256 threads), about 1024 blocks in all (four per CU)
  int64_t nb = (a.K + 4095) / 4096;
  const int64_t cap = patches >= 1024 ? 1 : 1024 / patches;
  if (nb > cap) nb = cap;
  a.chunk = (a.K + nb - 1) / nb;
  a.nb = (int)((a.K + a.chunk - 1) / a.chunk);
  void *partial = nullptr;
  MD_TRY(mdhip_alloc((size_t)patches * a.nb * TM * TN * sizeof(T), &partial));
  a.partial = partial;
  hipStream_t st = md_stream();
  MD_LAUNCH((k_longk_partial<TS, TM, TN>), dim3((unsigned)a.nb, (unsigned)patches), MD_BLOCK, a);
  k_longk_finish<TS, TM, TN><<<(unsigned)patches, MD_BLOCK, 0, st>>>(a);
  if (SkT<TS>::NARROW) md_opt_table()[MD_OPT_GEMM_NARROW_THIN_RUNS] += 2;
  const int rc = MD_LAUNCH_CHECK("matmul(few outputs, long k)");
  mdhip_free(partial);
  return rc;
}
template <class T> int longk_dispatch(const LongKArgs &a, int64_t batch) {
  if (a.M == 1 && a.N == 1) return longk_run<T, 1, 1>(a, batch);
  if (a.M <= 2 && a.N <= 2) return longk_run<T, 2, 2>(a, batch);
  if (a.M <= 4 && a.N <= 4) return longk_run<T, 4, 4>(a, batch);
  if (a.N == 1) return longk_run<T, 8, 1>(a, batch);
  if (a.M == 1) return longk_run<T, 1, 8>(a, batch);
  return longk_run<T, 8, 8>(a, batch);
}
}  // namespace

// The element spec of a storage-only product: operands float16 / int8 / uint8, c of the same type or (wide_out) the carrier's.
// f(spec) for the four that exist; uint8 -> uint8 is int8 -> int8 (the same low byte), uint8 has no wide form.
template <class F> static int with_thin_spec(int dtype, bool wide_out, F &&f) {
  if (dtype == MDHIP_F16) return wide_out ? f(MdThin<_Float16, float>{}) : f(MdThin<_Float16, _Float16>{});
  if (dtype == MDHIP_I8) return wide_out ? f(MdThin<int8_t, int32_t>{}) : f(MdThin<int8_t, int8_t>{});
  if (dtype == MDHIP_U8 && !wide_out) return f(MdThin<int8_t, int8_t>{});
  return -1;
}
static bool md_thin_dtype(int dtype) { return dtype == MDHIP_F16 || dtype == MDHIP_I8 || dtype == MDHIP_U8; }

// -1: not such a product; otherwise the launch status. dtype: MDHIP_F32 / F64 / I32 / I64, or (plan_narrow) the operands' F16 / I8 /
// U8 with c of that type or, wide_out, of the carrier's (float32 / int32).
int md_gemm_longk(const MdGemm &g, int dtype, bool wide_out) {
  if (!md_opt(MD_OPT_GEMM_SKINNY) || g.M < 1 || g.N < 1 || g.M > 128 || g.N > 128 || g.batch < 1) return -1;
  if (md_thin_dtype(dtype) ? !md_opt(MD_OPT_GEMM_NARROW_SKINNY) : wide_out) return -1;
  const int64_t big = g.M > g.N ? g.M : g.N, small = g.M > g.N ? g.N : g.M;
  if (big <= 8) {
    if (g.K < 512) return -1;
  } else {
    // larger outputs: only while k dwarfs them (the tile kernels would leave most of the chip idle); float32 from 64 x 64 up has the
    // MFMA split-k path
    if (g.K < 8192 || g.K < 64 * big) return -1;
    if ((dtype == MDHIP_F32 || dtype == MDHIP_F16) && small >= 64) return -1;
  }
  LongKArgs a{};
  a.A = g.a; a.B = g.b; a.C = g.c;
  a.K = g.K;
  a.M = (int)g.M; a.N = (int)g.N;
  a.a_bs = g.a_bs; a.a_ms = g.a_ms; a.a_ks = g.a_ks;
  a.b_bs = g.b_bs; a.b_ks = g.b_ks; a.b_ns = g.b_ns;
  a.c_bs = g.c_bs; a.c_ms = g.c_ms; a.c_ns = g.c_ns;
  switch (dtype) {
    case MDHIP_F32: return longk_dispatch<float>(a, g.batch);
    case MDHIP_F64: return longk_dispatch<double>(a, g.batch);
    case MDHIP_I32: return longk_dispatch<int32_t>(a, g.batch);
    case MDHIP_I64: return longk_dispatch<int64_t>(a, g.batch);
  }
  return with_thin_spec(dtype, wide_out, [&](auto spec) { return longk_dispatch<decltype(spec)>(a, g.batch); });
}

// -1: not a product for these kernels (the caller goes on to the MFMA / generic paths); otherwise the launch status.
// dtype: MDHIP_F32 / MDHIP_F64, or (plan_narrow) the operands' F16 / I8 / U8 with c of that type or, wide_out, of the carrier's.
int md_gemm_skinny(const MdGemm &g, int dtype, bool wide_out) {
  const bool thin = md_thin_dtype(dtype);
  if (!md_opt(MD_OPT_GEMM_SKINNY) || (dtype != MDHIP_F32 && dtype != MDHIP_F64 && !thin) || g.batch < 1 || g.batch > 65535) return -1;
  if (thin ? !md_opt(MD_OPT_GEMM_NARROW_SKINNY) || (wide_out && dtype == MDHIP_U8) : wide_out) return -1;
  const int64_t esz = (int64_t)md_dtype_size(dtype), V = 16 / esz;
  SkinnyArgs a{};
  if (g.N <= 8 && g.M > 8) {          // thin N: X = A, Y = B, out = C
    a.X = g.a; a.Y = g.b; a.out = g.c;
    a.R = g.M; a.K = g.K; a.nc = (int)g.N;
    a.xr = g.a_ms; a.xk = g.a_ks; a.x_bs = g.a_bs;
    a.yk = g.b_ks; a.yc = g.b_ns; a.y_bs = g.b_bs;
    a.o_r = g.c_ms; a.o_c = g.c_ns; a.o_bs = g.c_bs;
  } else if (g.M <= 8 && g.N > 8) {   // thin M: the transposed problem, X = B^T, Y = A^T, out = C^T
    a.X = g.b; a.Y = g.a; a.out = g.c;
    a.R = g.N; a.K = g.K; a.nc = (int)g.M;
    a.xr = g.b_ns; a.xk = g.b_ks; a.x_bs = g.b_bs;
    a.yk = g.a_ks; a.yc = g.a_ms; a.y_bs = g.a_bs;
    a.o_r = g.c_ns; a.o_c = g.c_ms; a.o_bs = g.c_bs;
  } else {
    return -1;
  }
  // worth a streaming kernel: a big operand of at least 1 Mi elements per launch, long enough both ways to fill the chip
  if (a.R < 512 || a.K < 64 || a.R * a.K * g.batch < (1ll << 20)) return -1;
  if (((uintptr_t)a.X & 15) || (a.x_bs % V)) return -1;
  bool rowdot;
  if (a.xk == 1 && a.xr >= a.K && a.xr % V == 0 && a.K % V == 0) rowdot = true;
  else if (a.xr == 1 && a.xk >= a.R && a.xk % V == 0 && a.R % V == 0) rowdot = false;
  else return -1;
  if (thin) return with_thin_spec(dtype, wide_out, [&](auto spec) { return skinny_run<decltype(spec)>(a, g.batch, rowdot); });
  return dtype == MDHIP_F32 ? skinny_run<float>(a, g.batch, rowdot) : skinny_run<double>(a, g.batch, rowdot);
}
