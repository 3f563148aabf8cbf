// fusion.hip — one-pass evaluation of recorded elementwise expressions, with an
// optional reduction epilogue (mdhip_vm_eval / mdhip_vm_reduce in include/mdhip.h).
//
// What it replaces: the eager tape launches one kernel per backend call, so the
// backward of a chain such as sum((sin(x)*y)**2) streams every intermediate through
// HBM (100*N bytes for cfg3) and the bias gradient of cfg4 first
// writes g*mask (128 MiB) and then column-sums it. Here the chain is a postfix
// program interpreted per element (csrc/md_vm.h) — the leaves are read once, the
// result is written (or reduced) once: HBM-bound at the *fused* byte count.
//
// Interpreter kernels (all wave-uniform control flow; they serve arrays below the
// run-time-compilation threshold and are the fallback when hiprtc is unavailable —
// arrays of >= 2^18 elements run the specialised kernels of fusion_jit.inc):
//   k_vm_eval_fast     (rows, inner) geometry: leaves contiguous / row- or column-
//                      broadcast / stride-0, 16-B loads+stores
//   k_vm_eval_axes     three / four collapsed axes, inner stride 0 or 1 in every leaf (the
//                      broadcasts of a normalisation layer), 16-B loads+stores
//   k_vm_eval_generic  any <=8-D strides, one element per lane
//   k_vm_reduce_all    full reduction of the program's value (grid-strided sweep,
//                      block partials + finishing block) — fused "...sum()"
//   k_vm_reduce_cols   2-D program reduced over rows: lane owns 4 columns, rows
//                      split over gridDim.y — fused reduce-to-shape (bias gradient);
//                      batched on gridDim.z: a middle axis of an (outer, n_red, inner)
//                      program reduced (the gradient of a (B,1,C) scale)
//   k_vm_reduce_rows   program reduced over its trailing axes: a wave per row, lanes
//                      stride the row's vector groups — fused per-row statistics
//                      (softmax denominators, row-wise dots, the gradient of a (R,1) scale)
// Reductions are deterministic (no atomics).
//
// Host side (behind the kernels): plan_eval / plan_reduce / plan_eval_reduce_cols choose ONE launch form (enum VmForm) and its
// numbers into a VmLaunch — generated kernel or interpreter, geometry, grid, scratch bytes — without allocating or launching;
// reduce_axis, reduce_cols_2d and sweep_cols are rungs of plan_reduce's ladder, and the order of the tests is the route.
// run_eval<T, To> / run_reduce<R, T> are one switch over the form with the interpreter launches; run_generated (no template)
// launches every generated kernel.
#include <vector>

#include "md_hip.h"
#include "md_strips.h"
#include "md_vm.h"

namespace {

constexpr int VG = 1;        // 16-B vector groups per lane per interpreter pass (large arrays take the compiled path)
constexpr int VW = 4 * VG;   // lanes of the operand stack per thread

// A leaf is read in its OWN storage type and converted to the program's float type on load (NumPy's cast of an operand to the
// loop dtype; md_load's conversions): four elements per lane and group whatever the type — an 8-byte load for the 2-byte types,
// 4-byte for the 1-byte ones, 16-byte for the 4-byte ones, two 16-byte loads for the 8-byte ones.
struct u8v { uint8_t v; };   // a uint8 VALUE (plain uint8_t is bool storage here: it loads as x != 0)
template <class T, class S> __device__ __forceinline__ T vm_cvt(S x) {
  if constexpr (md_same<S, uint8_t>::value) return (T)(x != 0);
  else if constexpr (md_same<S, u8v>::value) return (T)x.v;
  else if constexpr (md_same<S, f16>::value) return md_cast<T>(x);   // exact: every binary16 value is a float
  else return (T)x;
}
// every storage type by name, the five compute dtypes first; NO default that reads: with a narrower leaf a widening default
// would run past the array. (An unknown code never gets here — md_vm_check refuses it — and would load nothing.)
#define MD_VM_LEAF_SWITCH(dt, V, NONE) \
  switch (dt) {                        \
    case MDHIP_F32: V(float); break;   \
    case MDHIP_F64: V(double); break;  \
    case MDHIP_BOOL: V(uint8_t); break; \
    case MDHIP_I32: V(int32_t); break; \
    case MDHIP_I64: V(int64_t); break; \
    case MDHIP_F16: V(f16); break;     \
    case MDHIP_I8: V(int8_t); break;   \
    case MDHIP_U8: V(u8v); break;      \
    case MDHIP_I16: V(int16_t); break; \
    case MDHIP_U16: V(uint16_t); break; \
    case MDHIP_U32: V(uint32_t); break; \
    case MDHIP_U64: V(uint64_t); break; \
    default: NONE; break;              \
  }

// leaf load for VG element groups of the (rows, inner) geometry: VG independent vector loads
struct VmBatch {  // batched column reductions: per leaf, the elements from one batch to the next
  int64_t bs[MDHIP_VM_MAX_LEAVES];
};
template <class T> struct FastLoader {
  const MdVmDev &P;
  int64_t row[VG], c[VG];
  const int64_t *bs = nullptr;  // batched launches only: VmBatch::bs and the block's batch
  int64_t batch = 0;
  template <class S> __device__ __forceinline__ void vec(const MdVmLeaf &L, int64_t bo, T (&d)[VW]) const {
    MdVec<S, 4> v[VG];
#pragma unroll
    for (int g = 0; g < VG; ++g) v[g] = *reinterpret_cast<const MdVec<S, 4> *>((const S *)L.p + bo + row[g] * L.os + c[g]);
#pragma unroll
    for (int g = 0; g < VG; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) d[4 * g + j] = vm_cvt<T, S>(v[g].v[j]);
  }
  __device__ __forceinline__ void none(T (&d)[VW]) const {
#pragma unroll
    for (int j = 0; j < VW; ++j) d[j] = (T)0;
  }
  __device__ __forceinline__ void operator()(int l, T (&d)[VW]) const {
    const MdVmLeaf &L = P.leaf[l];
    const int64_t bo = bs ? batch * bs[l] : 0;
    if (L.is) {
#define MD_VM_V(S) vec<S>(L, bo, d)
      MD_VM_LEAF_SWITCH(L.dtype, MD_VM_V, none(d))
#undef MD_VM_V
    } else {
#pragma unroll
      for (int g = 0; g < VG; ++g) {
        const T s = md_load<T>(L.p, L.dtype, bo + row[g] * L.os);
#pragma unroll
        for (int j = 0; j < 4; ++j) d[4 * g + j] = s;
      }
    }
  }
};
template <class T> struct ScalarLoader {  // one element: leaf offsets precomputed by the caller
  const MdVmDev &P;
  const int64_t *offs;
  __device__ __forceinline__ void operator()(int l, T (&d)[1]) const { d[0] = md_load<T>(P.leaf[l].p, P.leaf[l].dtype, offs[l]); }
};
template <class T> struct FastLoader1 {  // single element on the fast geometry (tails)
  const MdVmDev &P;
  int64_t row, c;
  __device__ __forceinline__ void operator()(int l, T (&d)[1]) const {
    const MdVmLeaf &L = P.leaf[l];
    d[0] = md_load<T>(L.p, L.dtype, row * L.os + (L.is ? c : 0));
  }
};

// Program staging: every block copies the (<= 48 x 16 B) program from the kernarg
// segment into LDS once (static kernarg offsets: the scalar loads overlap), then
// each interpreter step reads its instruction with one broadcast ds_read_b128 that
// was issued one instruction earlier.
__device__ __forceinline__ void vm_stage_program(const MdVmDev &P, MdVmInstr *prog) {
#pragma unroll
  for (int i = 0; i < MDHIP_VM_MAX_INSTR; ++i) {
    if (i < P.n_instr && threadIdx.x == (unsigned)i) prog[i] = P.code[i];
  }
  if (threadIdx.x == 0) { prog[MDHIP_VM_MAX_INSTR].ctrl = 0; prog[MDHIP_VM_MAX_INSTR].imm = 0.0; }
  __syncthreads();
}
struct LdsFetch {
  const MdVmInstr *prog;
  uint4 nxt;
  __device__ __forceinline__ void prefetch(int pc) { nxt = *reinterpret_cast<const uint4 *>(prog + pc); }
  __device__ __forceinline__ void operator()(int, uint32_t &c, double &imm) const {
    c = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt.x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt.z);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)nxt.w);
    imm = __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
  }
};
#define MD_VM_PROLOGUE                                         \
  __shared__ MdVmInstr s_prog[MDHIP_VM_MAX_INSTR + 1];         \
  vm_stage_program(P, s_prog);                                 \
  LdsFetch fetch{s_prog, uint4{0, 0, 0, 0}}

__device__ __forceinline__ void vm_row_col(int64_t v, int64_t nv, int64_t rows, int64_t &row, int64_t &cv) {
  if (rows == 1) { row = 0; cv = v; }
  else if ((uint64_t)v < 0x100000000ull && (uint64_t)nv < 0x100000000ull) {
    uint32_t q = (uint32_t)v / (uint32_t)nv;
    row = q; cv = (uint32_t)v - q * (uint32_t)nv;
  } else { row = v / nv; cv = v - row * nv; }
}

template <class T, class To>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_eval_fast(MdVmDev P, To *out, int64_t rows, int64_t inner) {
  MD_VM_PROLOGUE;
  const int64_t nv = inner >> 2, total = rows * nv;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
  for (int64_t v0 = gid; v0 < total; v0 += VG * gs) {
    FastLoader<T> ld{P, {}, {}};
    bool ok[VG];
    int64_t orow[VG], ocol[VG];
#pragma unroll
    for (int g = 0; g < VG; ++g) {
      const int64_t v = v0 + g * gs;
      ok[g] = v < total;
      int64_t row, cv;
      vm_row_col(ok[g] ? v : v0, nv, rows, row, cv);   // out-of-range groups recompute group 0, unstored
      ld.row[g] = orow[g] = row;
      ld.c[g] = ocol[g] = cv << 2;
    }
    T r[VW];
    md_vm_run<T, VW>(P.n_instr, fetch, ld, r);
#pragma unroll
    for (int g = 0; g < VG; ++g) {
      if (!ok[g]) continue;
      MdVec<To, 4> o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.v[j] = md_cast<To>(r[4 * g + j]);
      *reinterpret_cast<MdVec<To, 4> *>(out + orow[g] * inner + ocol[g]) = o;
    }
  }
  if (rows == 1) {
    const int64_t t0 = nv << 2;
    if (gid < inner - t0) {
      FastLoader1<T> ld{P, 0, t0 + gid};
      T r[1];
      md_vm_run<T, 1>(P.n_instr, fetch, ld, r);
      out[t0 + gid] = md_cast<To>(r[0]);
    }
  }
}

// Three / four collapsed axes with a contiguous (or broadcast) inner axis in every leaf — chains under the broadcasts of a
// normalisation layer, `(x * g[:, None, :] + h[None, :, None]) ** 2` — : a lane evaluates one vector of four, the outer position from
// two or three divisions (elementwise.hip's k_ew_axes is the eager counterpart). Interpreter only: was the one-element generic walk.
struct VmAxes {
  int64_t e0, e1, e2, nv, rows;
  int64_t st[MDHIP_VM_MAX_LEAVES][3];
};
template <class T> struct AxesLoader {
  const MdVmDev &P;
  const VmAxes &A;
  int64_t r0, r1, r2, c;
  template <class S> __device__ __forceinline__ void vec(const MdVmLeaf &L, int64_t off, T (&d)[4]) const {
    const MdVec<S, 4> v = *reinterpret_cast<const MdVec<S, 4> *>((const S *)L.p + off + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = vm_cvt<T, S>(v.v[j]);
  }
  __device__ __forceinline__ void none(T (&d)[4]) const {
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = (T)0;
  }
  __device__ __forceinline__ void operator()(int l, T (&d)[4]) const {
    const MdVmLeaf &L = P.leaf[l];
    const int64_t off = r0 * A.st[l][0] + r1 * A.st[l][1] + r2 * A.st[l][2];
    if (L.is) {
#define MD_VM_V(S) vec<S>(L, off, d)
      MD_VM_LEAF_SWITCH(L.dtype, MD_VM_V, none(d))
#undef MD_VM_V
    } else {
      const T s = md_load<T>(L.p, L.dtype, off);
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = s;
    }
  }
};
template <class T, class To>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_eval_axes(MdVmDev P, VmAxes A, To *out) {
  MD_VM_PROLOGUE;
  const int64_t total = A.rows * A.nv, gs = (int64_t)gridDim.x * blockDim.x;
  const bool narrow = total < (1ll << 31);
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < total; v += gs) {
    int64_t row, r0 = 0, r1, r2;
    if (narrow) {
      const uint32_t w = (uint32_t)v / (uint32_t)A.nv, q = w / (uint32_t)A.e2;
      row = w;
      r2 = w - q * (uint32_t)A.e2;
      r1 = q;
      if (A.e0 != 1) { const uint32_t t = q / (uint32_t)A.e1; r0 = t; r1 = q - t * (uint32_t)A.e1; }
    } else {
      row = v / A.nv;
      const int64_t q = row / A.e2;
      r2 = row - q * A.e2;
      r1 = q;
      if (A.e0 != 1) { r0 = q / A.e1; r1 = q - r0 * A.e1; }
    }
    const int64_t c = (v - row * A.nv) << 2;
    AxesLoader<T> ld{P, A, r0, r1, r2, c};
    T r[4];
    md_vm_run<T, 4>(P.n_instr, fetch, ld, r);
    MdVec<To, 4> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = md_cast<To>(r[j]);
    *reinterpret_cast<MdVec<To, 4> *>(out + row * (A.nv << 2) + c) = o;
  }
}

template <class T, class To>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_eval_generic(MdVmDev P, MdVmIter it, To *out) {
  MD_VM_PROLOGUE;
  const int64_t gs = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < it.total; i += gs) {
    int64_t offs[MDHIP_VM_MAX_LEAVES + 1];
    for (int l = 0; l <= MDHIP_VM_MAX_LEAVES; ++l) offs[l] = 0;
    int64_t lin = i;
    for (int d = it.ndim - 1; d >= 0; --d) {
      const int64_t e = it.shape[d], q = lin / e, r = lin - q * e;
      lin = q;
      for (int l = 0; l < P.n_leaves; ++l) offs[l] += r * it.strides[l][d];
      offs[MDHIP_VM_MAX_LEAVES] += r * it.strides[MDHIP_VM_MAX_LEAVES][d];
    }
    ScalarLoader<T> ld{P, offs};
    T r[1];
    md_vm_run<T, 1>(P.n_instr, fetch, ld, r);
    out[offs[MDHIP_VM_MAX_LEAVES]] = md_cast<To>(r[0]);
  }
}

// ------------------------------------------------------------------ reductions ----
template <class R, class T> __device__ __forceinline__ T vm_block_reduce(T v, T *smem) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = R::combine(v, md_shfl_down(v, d));
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) smem[w] = v;
  __syncthreads();
  if (w == 0) {
    v = lane < nw ? smem[lane] : R::template identity<T>();
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) v = R::combine(v, md_shfl_down(v, d));
  }
  return v;
}

template <class R, class T>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_reduce_all(MdVmDev P, int64_t rows, int64_t inner, T *partial, unsigned *tickets, T *out) {
  MD_VM_PROLOGUE;
  __shared__ T smem[MD_BLOCK / 64];
  __shared__ unsigned last_flag;
  const int64_t nv = inner >> 2, total = rows * nv;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gs = (int64_t)gridDim.x * blockDim.x;
  T a[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) a[j] = R::template identity<T>();
  for (int64_t v0 = gid; v0 < total; v0 += VG * gs) {
    FastLoader<T> ld{P, {}, {}};
    bool ok[VG];
#pragma unroll
    for (int g = 0; g < VG; ++g) {
      const int64_t v = v0 + g * gs;
      ok[g] = v < total;
      int64_t row, cv;
      vm_row_col(ok[g] ? v : v0, nv, rows, row, cv);
      ld.row[g] = row;
      ld.c[g] = cv << 2;
    }
    T r[VW];
    md_vm_run<T, VW>(P.n_instr, fetch, ld, r);
#pragma unroll
    for (int g = 0; g < VG; ++g)
      if (ok[g]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * g + j] = R::combine(a[4 * g + j], r[4 * g + j]);
      }
  }
  T acc = R::template identity<T>();
#pragma unroll
  for (int j = 0; j < VW; ++j) acc = R::combine(acc, a[j]);
  if (rows == 1) {
    const int64_t t0 = nv << 2;
    if (gid < inner - t0) {
      FastLoader1<T> ld{P, 0, t0 + gid};
      T r[1];
      md_vm_run<T, 1>(P.n_instr, fetch, ld, r);
      acc = R::combine(acc, r[0]);
    }
  }
  acc = vm_block_reduce<R>(acc, smem);
  // block partials -> the block that arrives last sums them in index order (md_ticket.h): no finishing launch
  if (threadIdx.x == 0) md_st_sc1(partial + blockIdx.x, acc);
  const bool last = gridDim.x >= 64 ? md_ticket_last2(tickets, blockIdx.x, gridDim.x, &last_flag) : md_ticket_last(tickets, gridDim.x, &last_flag);
  if (!last) return;
  acc = md_fold_partials<R>(partial, gridDim.x);
  acc = vm_block_reduce<R>(acc, smem);
  if (threadIdx.x == 0) out[0] = acc;
}

// 2-D program [n_red rows][n_out cols] reduced over rows; a lane owns 4 columns and
// takes rows r, r+4, r+8, r+12 per interpreter pass (four 16-B loads per leaf in flight).
// BATCH: gridDim.z independent problems of that shape (a middle axis reduced), unsplit; batch z reads leaf l from B.bs[l] * z on
// and writes row z of dst.
template <class R, class T, bool FINAL, bool BATCH = false>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_reduce_cols(MdVmDev P, int64_t n_out, int64_t n_red, int64_t chunk, T *dst, VmBatch B) {
  MD_VM_PROLOGUE;
  if constexpr (BATCH) dst += (int64_t)blockIdx.z * n_out;
  __shared__ T smem[3][64][4];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int64_t col = ((int64_t)blockIdx.x * 64 + cx) * 4;
  const int64_t s = blockIdx.y, r0 = s * chunk;
  int64_t r1 = r0 + chunk;
  if (r1 > n_red) r1 = n_red;
  T a[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) a[j] = R::template identity<T>();
  // every lane of a wave runs the interpreter together (uniform control flow); lanes past
  // the last column recompute column group 0 of their block and are never stored
  const int64_t lcol = col < n_out ? col : (int64_t)blockIdx.x * 256;
  for (int64_t r = r0 + ry; r < r1; r += 4 * VG) {
    FastLoader<T> ld{P, {}, {}};
    if constexpr (BATCH) { ld.bs = B.bs; ld.batch = blockIdx.z; }
    bool ok[VG];
#pragma unroll
    for (int g = 0; g < VG; ++g) {
      const int64_t rr = r + 4 * g;
      ok[g] = rr < r1;
      ld.row[g] = ok[g] ? rr : r;
      ld.c[g] = lcol;
    }
    T v[VW];
    md_vm_run<T, VW>(P.n_instr, fetch, ld, v);
#pragma unroll
    for (int g = 0; g < VG; ++g)
      if (ok[g]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[4 * g + j] = R::combine(a[4 * g + j], v[4 * g + j]);
      }
  }
  T tot[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    tot[j] = a[j];
#pragma unroll
    for (int g = 1; g < VG; ++g) tot[j] = R::combine(tot[j], a[4 * g + j]);
  }
  if (ry > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) smem[ry - 1][cx][j] = tot[j];
  }
  __syncthreads();
  if (ry == 0 && col < n_out) {
    MdVec<T, 4> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = R::combine(R::combine(tot[j], smem[0][cx][j]), R::combine(smem[1][cx][j], smem[2][cx][j]));
    T *d = FINAL ? dst + col : dst + s * n_out + col;
    *reinterpret_cast<MdVec<T, 4> *>(d) = o;
  }
}

// (n_out rows, n_red columns) program reduced over the columns — the trailing axes of the recorded shape. One form for every
// row length: a wave per row, four rows per block; lane l takes the row's vector groups l, l + 64, .. and alternates between two
// sets of four accumulators (even / odd trips: half the serial chain of additions — a row of 8196 passes 17 trips per set, not
// 33), then the sets and their four components merge and a 64-lane shuffle tree finishes; lane 0 stores. The order depends on
// (n_out, n_red) alone. Lanes past the last vector group re-evaluate group 0 of their row and waves past the last row the last
// row, both masked out of the combine / the store: every wave runs the interpreter in step (uniform control flow).
template <class R, class T>
__global__ void __launch_bounds__(MD_BLOCK) k_vm_reduce_rows(MdVmDev P, int64_t n_out, int64_t n_red, T *dst) {
  MD_VM_PROLOGUE;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row_raw = (int64_t)blockIdx.x * (MD_BLOCK / 64) + w;
  const bool row_ok = row_raw < n_out;
  const int64_t row = row_ok ? row_raw : n_out - 1;
  const int64_t nv = n_red >> 2;
  T a[VW], b[VW];
#pragma unroll
  for (int j = 0; j < VW; ++j) { a[j] = R::template identity<T>(); b[j] = a[j]; }
  bool odd = false;
  for (int64_t g0 = 0; g0 < nv; g0 += 64) {
    const int64_t g = g0 + lane;
    const bool ok = g < nv;
    FastLoader<T> ld{P, {}, {}};
    ld.row[0] = row;
    ld.c[0] = (ok ? g : 0) << 2;
    T r[VW];
    md_vm_run<T, VW>(P.n_instr, fetch, ld, r);
#pragma unroll
    for (int j = 0; j < VW; ++j) {
      const T c = R::combine(odd ? b[j] : a[j], r[j]);
      a[j] = (ok && !odd) ? c : a[j];
      b[j] = (ok && odd) ? c : b[j];
    }
    odd = !odd;
  }
#pragma unroll
  for (int j = 0; j < VW; ++j) a[j] = R::combine(a[j], b[j]);
  T acc = R::combine(R::combine(a[0], a[1]), R::combine(a[2], a[3]));
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) acc = R::combine(acc, md_shfl_down(acc, d));
  if (lane == 0 && row_ok) dst[row_raw] = acc;
}

}  // namespace
#include "fusion_jit.inc"
namespace {

// ------------------------------------------------------------------------ host ----
// plan_eval / plan_reduce choose ONE launch form (enum VmForm) and its numbers, without allocating or launching; run_eval /
// run_reduce are one switch over that form: the interpreter kernels there, every generated kernel through run_generated.
static void to_dev(const mdhip_vm_program *pr, MdVmDev *D) {
  memset(D, 0, sizeof *D);
  D->n_instr = pr->n_instr;
  D->n_leaves = pr->n_leaves;
  for (int i = 0; i < pr->n_instr; ++i) { D->code[i].ctrl = pr->ctrl[i]; D->code[i].imm = pr->imm[i]; }
  for (int l = 0; l < pr->n_leaves; ++l) {
    D->leaf[l].p = pr->leaves[l].data;
    D->leaf[l].dtype = pr->leaves[l].dtype;
  }
}
static bool al_for(const void *p, int dtype) {
  const uintptr_t al = md_dtype_size(dtype) * 4 > 16 ? 16 : md_dtype_size(dtype) * 4;
  return ((uintptr_t)p % al) == 0;
}
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
static int64_t elems_of(const mdhip_array *a) {
  int64_t n = 1;
  for (int d = 0; d < a->ndim; ++d) n *= a->shape[d];
  return n;
}
// (rows, inner) geometry usable by the vector kernels? fills leaf os/is.
static bool fast_geometry(const MdVmIter &it, int n_leaves, const mdhip_vm_program *pr, bool out_contig_required, MdVmDev *D,
                          int64_t *rows, int64_t *inner) {
  if (it.ndim < 1 || it.ndim > 2) return false;
  *inner = it.shape[it.ndim - 1];
  *rows = it.ndim == 2 ? it.shape[0] : 1;
  if (*rows > 1 && (*inner & 3)) return false;
  const int O = MDHIP_VM_MAX_LEAVES;
  if (out_contig_required) {
    if (it.strides[O][it.ndim - 1] != 1) return false;
    if (it.ndim == 2 && it.strides[O][0] != *inner) return false;
  }
  for (int l = 0; l < n_leaves; ++l) {
    const int64_t is = it.strides[l][it.ndim - 1], os = it.ndim == 2 ? it.strides[l][0] : 0;
    if (is != 0 && is != 1) return false;
    if (is == 1) {
      if (!al_for(pr->leaves[l].data, pr->leaves[l].dtype)) return false;
      if (*rows > 1 && (os & 3)) return false;
    }
    D->leaf[l].os = os;
    D->leaf[l].is = (int32_t)is;
  }
  return true;
}

// k_vm_eval_axes eligibility (the conditions of elementwise.hip's axes_geom, per leaf); fills leaf `is` and the stride table
static bool axes_geometry(const MdVmIter &it, const mdhip_vm_program *pr, const mdhip_array *out, MdVmDev *D, VmAxes *A) {
  if (it.ndim != 3 && it.ndim != 4) return false;
  const int nd = it.ndim, sh = 4 - nd, O = MDHIP_VM_MAX_LEAVES;
  const int64_t inner = it.shape[nd - 1];
  if ((inner & 3) || it.total < (1 << 16) || it.strides[O][nd - 1] != 1 || !al_for(out->data, out->dtype)) return false;
  int64_t dense = inner;
  for (int d = nd - 2; d >= 0; --d) {
    if (it.strides[O][d] != dense) return false;
    dense *= it.shape[d];
  }
  memset(A, 0, sizeof *A);
  A->e0 = nd == 4 ? it.shape[0] : 1;
  A->e1 = it.shape[1 - sh];
  A->e2 = it.shape[2 - sh];
  A->nv = inner >> 2;
  A->rows = A->e0 * A->e1 * A->e2;
  for (int l = 0; l < pr->n_leaves; ++l) {
    const int64_t is = it.strides[l][nd - 1];
    if (is != 0 && is != 1) return false;
    if (is == 1 && !al_for(pr->leaves[l].data, pr->leaves[l].dtype)) return false;
    for (int j = sh; j < 3; ++j) {
      const int64_t st = it.strides[l][j - sh];
      if (is == 1 && (st & 3)) return false;
      A->st[l][j] = st;
    }
    D->leaf[l].os = 0;
    D->leaf[l].is = (int32_t)is;
  }
  return true;
}

// ---- one launch, planned ----
enum VmForm {
  VM_NONE,          // nothing to launch: an empty evaluation, or programs that mdhip_vm_eval_multi evaluates one by one
  VM_EVAL_FAST,     // k_vm_eval_fast | generated EVAL on the (rows, inner) geometry
  VM_EVAL_AXES,     // k_vm_eval_axes | generated EVAL over three / four collapsed axes
  VM_EVAL_GENERIC,  // k_vm_eval_generic
  VM_RED_ALL,       // k_vm_reduce_all | generated RED_ALL: `grid` block partials, the last block finishes
  VM_COLS_STRIPS,   // generated SWEEP only: NS strips x NB row bands (x outer batches), with or without the evaluated value stored
  VM_COLS_TILED,    // k_vm_reduce_cols | generated RED_COLS: one pass (splits == 1), or `splits` partial rows and a second pass
  VM_COLS_BATCHED,  // .. with the batch on the grid: `outer` problems in one launch, unsplit
  VM_ROWS,          // k_vm_reduce_rows | generated RED_ROWS
  VM_ROWS_STAGED,   // generated ROWS_STAGED only: a staged program, every row held in registers across its stages
};
// plan_begin sets the scalars (0; outer = splits = 1); the four tables are NOT zeroed per call and hold something only where a
// planner filled them: D in every form but VM_NONE, `it` where md_vm_build_iter ran (not on reduce_axis's path), G and B as noted.
struct VmLaunch {
  VmForm form;
  hipFunction_t fn;          // the generated kernel; nullptr: the interpreter kernel of the form
  MdVmDev D;
  MdVmIter it;               // (VM_EVAL_GENERIC reads it in the kernel)
  VmAxes G;                  // VM_EVAL_AXES
  VmBatch B;                 // VM_COLS_BATCHED, VM_COLS_STRIPS with `batch`
  const double *imm;         // the immediates a generated kernel takes as arguments: n_imm of them
  int n_imm;
  int n;                     // outputs of an evaluation
  bool batch;
  int64_t rows, inner;       // the (rows, inner) geometry of D
  int64_t n_out, n_red, outer, chunk, splits, NS, NB;
  int64_t grid;              // blocks on x (the strips: NS * NB)
  size_t partial_bytes;      // scratch the launch needs (block partials, partial rows), in the compute type; 0: none
};

static int vm_unplanned(const VmLaunch &L) { return md_fail(MDHIP_ERUNTIME, "vm: launch form %d has no launcher here", (int)L.form); }

// blocks of the interpreter's streaming kernels (k_vm_eval_fast, k_vm_reduce_all)
static int interp_grid(int64_t rows, int64_t inner) { return md_grid_for((rows * (inner >> 2) + VG - 1) / VG + (rows == 1 ? 4 : 0)); }

// merge the leaf tables of n programs (identical descriptors share a slot) and give every
// immediate its slot in the shared array; false if the bounds of one launch are exceeded
static bool merge_programs(const mdhip_vm_program *progs, int n, jit::Spec *M, mdhip_vm_program *merged) {
  if (n < 2 || n > 4) return false;
  M->kind = jit::EVAL;
  M->n = n;
  M->n_leaves = 0;
  M->n_imm = 0;
  M->f32 = progs[0].compute_dtype == MDHIP_F32;
  memset(merged, 0, sizeof *merged);
  merged->compute_dtype = progs[0].compute_dtype;
  for (int k = 0; k < n; ++k) {
    const mdhip_vm_program *pr = &progs[k];
    if (pr->compute_dtype != progs[0].compute_dtype) return false;
    M->pr[k] = pr;
    for (int l = 0; l < pr->n_leaves; ++l) {
      const mdhip_array &a = pr->leaves[l];
      int slot = -1;
      for (int m = 0; m < M->n_leaves && slot < 0; ++m) {
        const mdhip_array &b = merged->leaves[m];
        bool same = a.data == b.data && a.dtype == b.dtype && a.ndim == b.ndim;
        for (int d = 0; same && d < a.ndim; ++d) same = a.shape[d] == b.shape[d] && a.strides[d] == b.strides[d];
        if (same) slot = m;
      }
      if (slot < 0) {
        if (M->n_leaves == MDHIP_VM_MAX_LEAVES) return false;
        slot = M->n_leaves++;
        merged->leaves[slot] = a;
        M->leaf_dtype[slot] = a.dtype;
      }
      M->leaf_map[k][l] = slot;
    }
    for (int pc = 0; pc < pr->n_instr; ++pc) {
      const uint32_t c = pr->ctrl[pc];
      const bool has_imm = MD_VM_KIND(c) != MDHIP_VM_UNARY && MD_VM_KIND(c) != MDHIP_VM_WHERE &&
                           (MD_VM_RS(c) == MDHIP_VM_SRC_CONST || (MD_VM_KIND(c) == MDHIP_VM_BINARY && MD_VM_LS(c) == MDHIP_VM_SRC_CONST));
      M->imm_slot[k][pc] = 0;
      if (has_imm) {
        if (M->n_imm == MDHIP_VM_MAX_INSTR) return false;
        merged->imm[M->n_imm] = pr->imm[pc];
        M->imm_slot[k][pc] = M->n_imm++;
      }
    }
  }
  merged->n_leaves = M->n_leaves;
  merged->n_instr = 1;  // a placeholder PUSH so that the merged table passes md_vm_build_iter
  merged->ctrl[0] = MDHIP_VM_CTRL(MDHIP_VM_PUSH, 0, 0, 0, MDHIP_VM_SRC_LEAF, 0);
  return M->n_leaves > 0;
}

// what every plan starts from: nothing to launch, the program's own immediates
static void plan_begin(VmLaunch *L, const mdhip_vm_program *pr) {
  L->form = VM_NONE;
  L->fn = nullptr;
  L->imm = pr->imm;
  L->n_imm = pr->n_instr;
  L->n = 1;
  L->batch = false;
  L->outer = L->splits = 1;
  L->rows = L->inner = L->n_out = L->n_red = L->chunk = L->NS = L->NB = L->grid = 0;
  L->partial_bytes = 0;
}

// Trailing-axis reductions (mdhip_vm_reduce's third form): rows up to 64 lanes x 8 groups x 4 elements go a wave per row in the
// generated kernels, longer ones a block per row; long rows need at least a row per CU (no cross-block split yet)
constexpr int64_t VM_ROWS_WAVE_MAX = 64 * 4 * 8;
constexpr int64_t VM_ROWS_MIN_OUT = MD_NUM_CUS;
// a staged program holds rows up to 256 lanes x 8 groups x 4 elements, a block per row above VM_ROWS_WAVE_MAX
constexpr int64_t VM_ROWS_STAGED_MAX = 256 * 4 * 8;
// vector groups per lane of the wave-per-row kernels (RED_ROWS, ROWS_STAGED) for a row of n_red <= VM_ROWS_WAVE_MAX elements
static int rows_wave_nv(int64_t n_red) {
  const int64_t nvec = n_red >> 2;
  return nvec <= 64 ? 1 : nvec <= 128 ? 2 : nvec <= 256 ? 4 : 8;
}
// vector groups per lane of the block-per-row staged kernel for a row of VM_ROWS_WAVE_MAX < n_red <= VM_ROWS_STAGED_MAX elements: 3 .. 8
static int rows_block_g(int64_t n_red) { return (int)md_ceil_div(n_red >> 2, (int64_t)256); }
// A staged kernel holds NV (a block per row: G) groups of every vector leaf in registers through all its stages: 4 NV registers
// per float32 leaf and lane, 8 NV per float64 one. Up to this many the compiled kernels use no scratch (DESIGN.md §4.7 has the figures); a program
// that would hold more is refused, and the caller composes.
constexpr int VM_STAGED_HELD_MAX = 256;
static int staged_held(const jit::Spec &S) {
  int vec = 0;
  for (int l = 0; l < S.n_leaves; ++l) vec += S.leaf_mode[l] == jit::LM_VEC;
  return vec * (S.G ? S.G : S.NV) * (S.f32 ? 4 : 8);
}

// A program whose operands are all dense or fully broadcast collapses to ONE axis; the column reductions want it as
// (R rows, C columns) again: dense leaves advance C elements per row, broadcast ones none.
static bool uncollapse_2d(const MdVmIter &it, int n_leaves, MdVmDev *D, int64_t R, int64_t C, int64_t *rows, int64_t *inner) {
  if (it.ndim == 2 && *rows == R && *inner == C) return true;
  if (it.ndim != 1 || *rows != 1 || *inner != R * C || (C & 3)) return false;
  for (int l = 0; l < n_leaves; ++l) D->leaf[l].os = D->leaf[l].is ? C : 0;
  *rows = R;
  *inner = C;
  return true;
}

// Plan a STAGED program (include/mdhip.h) into `out`: the (n_out, n_red) geometry of mdhip_vm_reduce's third form with rows a wave
// holds, or a block (then from VM_ROWS_MIN_OUT rows on: below that floor mdhip_vm_reduce refuses long rows, the composed route
// takes the eager kernels, whose order is another, and staged and composed would differ), generated kernel only.
// Every refusal is MDHIP_EVALUE: the caller composes the stages from mdhip_vm_reduce and mdhip_vm_eval.
static int plan_staged(const mdhip_vm_program *pr, const mdhip_array *out, int64_t n_red, VmLaunch *L) {
  if (out->dtype != pr->compute_dtype) return md_fail(MDHIP_EVALUE, "vm_eval: a staged program stores the compute dtype only");
  const int nd = out->ndim;
  if (nd < 1) return md_fail(MDHIP_EVALUE, "vm_eval: a staged program needs an axis to reduce");
  if (n_red == 0) n_red = out->shape[nd - 1];
  int64_t p = 1;
  for (int d = nd - 1; d >= 0 && p < n_red; --d) p *= out->shape[d];
  if (p != n_red || n_red < 4 || (n_red & 3)) return md_fail(MDHIP_EVALUE, "vm_eval: rows of %lld elements are not trailing axes of whole 16-byte groups", (long long)n_red);
  if (n_red > VM_ROWS_STAGED_MAX) return md_fail(MDHIP_EVALUE, "vm_eval: rows of %lld elements are longer than a block holds (%lld)", (long long)n_red, (long long)VM_ROWS_STAGED_MAX);
  const bool block = n_red > VM_ROWS_WAVE_MAX;   // a block per row
  MD_TRY(md_vm_build_iter(&L->it, pr, out, out));
  const int64_t total = L->it.total, n_out = total / n_red;
  if (n_out < 2 || n_out >= (1ll << 31)) return md_fail(MDHIP_EVALUE, "vm_eval: %lld rows are not staged", (long long)n_out);
  if (block && n_out < VM_ROWS_MIN_OUT) return md_fail(MDHIP_EVALUE, "vm_eval: %lld rows of %lld elements are not staged (a block per row from %lld rows on)", (long long)n_out, (long long)n_red, (long long)VM_ROWS_MIN_OUT);
  to_dev(pr, &L->D);
  if (!fast_geometry(L->it, pr->n_leaves, pr, true, &L->D, &L->rows, &L->inner) || !aligned16(out->data) ||
      !uncollapse_2d(L->it, pr->n_leaves, &L->D, n_out, n_red, &L->rows, &L->inner))
    return md_fail(MDHIP_EVALUE, "vm_eval: a staged program needs (rows, reduced) geometry with rows of whole, aligned 16-byte groups");
  jit::Spec S;
  if (!jit::spec_for(&S, jit::ROWS_STAGED, pr, L->D, L->rows, total)) return md_fail(MDHIP_EVALUE, "vm_eval: a staged program runs as a generated kernel only (options jit, jit_min)");
  if (block) S.G = rows_block_g(n_red);
  else S.NV = rows_wave_nv(n_red);
  if (staged_held(S) > VM_STAGED_HELD_MAX) return md_fail(MDHIP_EVALUE, "vm_eval: the staged program would hold %d registers per lane (max %d)", staged_held(S), VM_STAGED_HELD_MAX);
  // streamed: the stored value and the leaves that advance from row to row (a row-invariant vector is re-read from the caches)
  S.nt = total * (int64_t)md_dtype_size(out->dtype) + jit::streamed_bytes(L->D, total, true) > jit::NT_BYTES;
  L->fn = jit::get(S);
  if (!L->fn) return md_fail(MDHIP_EVALUE, "vm_eval: no run-time compiler for the staged program");
  L->form = VM_ROWS_STAGED;
  L->n_out = n_out; L->n_red = n_red;
  L->grid = block ? n_out : md_ceil_div(n_out, 4);
  return MDHIP_OK;
}

// Plan an evaluation into outs[0 .. n). n == 1 is mdhip_vm_eval: the fast, the axes or the generic form, each (but the generic one)
// generated from jit_min elements on and interpreted below. The output's dtype says what is stored — the compute type, b8 (truth
// values) or f16 (the chain's value rounded ONCE to binary16 in the same pass: astype(chain, float16)).
// n > 1 is mdhip_vm_eval_multi: the programs share ONE generated launch on the fast or the axes geometry (`merged`, the caller's,
// holds their common leaf table and immediates and lives as long as the plan), or the plan stays VM_NONE — declined, never an
// error: the caller evaluates them one by one.
static int plan_eval(const mdhip_vm_program *progs, const mdhip_array *outs, int n, mdhip_vm_program *merged, VmLaunch *L, int64_t staged_n_red = -1) {
  const bool multi = n > 1;
  const mdhip_vm_program *pr = progs;   // whose leaves give the geometry: the one program, or the merged table
  plan_begin(L, pr);
  if (staged_n_red >= 0) return plan_staged(pr, &outs[0], staged_n_red, L);   // a staged program, as mdhip_vm_eval's md_vm_check_staged found it
  jit::Spec S;
  if (multi) {
    if (!jit::enabled() || !merge_programs(progs, n, &S, merged)) return MDHIP_OK;
    for (int k = 0; k < n; ++k) {  // outputs: the compute dtype, contiguous, one shape
      if (outs[k].dtype != merged->compute_dtype || outs[k].ndim != outs[0].ndim) return MDHIP_OK;
      for (int d = 0; d < outs[0].ndim; ++d)
        if (outs[k].shape[d] != outs[0].shape[d] || outs[k].strides[d] != outs[0].strides[d]) return MDHIP_OK;
      if (!aligned16(outs[k].data)) return MDHIP_OK;
    }
    pr = merged;
    L->imm = merged->imm;   // (the merged program has n_instr == 1, but S.n_imm immediates)
    L->n_imm = S.n_imm;
    L->n = n;
  }
  const int rc = md_vm_build_iter(&L->it, pr, &outs[0], &outs[0]);
  if (rc != MDHIP_OK) return multi ? MDHIP_OK : rc;
  const int64_t total = L->it.total;
  if (multi ? total < jit::min_elems() : total == 0) return MDHIP_OK;
  to_dev(pr, &L->D);
  const int out_dtype = outs[0].dtype;
  const int64_t out_bytes = (int64_t)n * (int64_t)md_dtype_size(out_dtype);   // per element, all outputs together
  // the common part of the Spec; false: the interpreter runs. (Several programs: merge_programs began it, and only a generated kernel will do.)
  auto want_generated = [&](int64_t rows) {
    if (multi) jit::spec_modes(&S, L->D, rows);
    else if (!jit::spec_for(&S, jit::EVAL, pr, L->D, rows, total)) return false;
    S.out_bool = out_dtype == MDHIP_BOOL;
    S.out_f16 = out_dtype == MDHIP_F16;
    return true;
  };
  if (fast_geometry(L->it, pr->n_leaves, pr, true, &L->D, &L->rows, &L->inner) && (multi || al_for(outs[0].data, out_dtype))) {
    if (want_generated(L->rows)) {
      // the streamed bytes of this launch: outputs + vector leaves
      S.nt = total * out_bytes + jit::streamed_bytes(L->D, total, false) > jit::NT_BYTES;
      jit::eval_shape(&S);
      L->fn = jit::get(S);
      if (L->fn) L->grid = jit::stream_grid(L->rows, L->inner, jit::eval_blocks(S));
    }
    if (!L->fn) L->grid = interp_grid(L->rows, L->inner);
    if (L->fn || !multi) L->form = VM_EVAL_FAST;
    return MDHIP_OK;
  }
  // three / four collapsed axes: the axes form of the same kernels, still one launch
  if (axes_geometry(L->it, pr, &outs[0], &L->D, &L->G)) {
    if (want_generated(L->G.rows)) {
      jit::spec_axes(&S, L->D, L->G, out_bytes);
      L->fn = jit::get(S);
      if (L->fn) L->grid = jit::axes_grid(S, L->G);
    }
    if (!L->fn) L->grid = md_grid_for(total >> 2);
    if (L->fn || !multi) L->form = VM_EVAL_AXES;
    return MDHIP_OK;
  }
  if (multi) return MDHIP_OK;
  L->grid = md_grid_for(total);
  L->form = VM_EVAL_GENERIC;
  return MDHIP_OK;
}

// Strip geometry for a (n_red x n_out) program (the generated SWEEP kernel, fusion_jit.inc): NS strips of 256 columns x NB
// interleaved row bands, one block per CU, <= 64 bands (the last block of a strip holds its partial rows in registers).
// `outer` > 1: that many such problems in one launch (the batch on blockIdx.y, as reduce.hip's batched strips): the bands come
// from NS * outer blocks; where the batches' tickets (one per strip and batch) or a batch's partial rows (32-bit buffer offsets
// in the kernel) do not fit, every batch runs in one band.
static bool sweep_geometry(int64_t n_out, int64_t n_red, int ru, int64_t *NS, int64_t *NB, int64_t outer = 1) {
  if ((n_out & 3) || n_out < 4 || n_red < 512) return false;
  const int nb_force = (int)md_opt(MD_OPT_SWEEP_NB);
  const int64_t ns = (n_out + 255) / 256, nse = ns * outer;
  // one block per CU, as the column sums of reduce.hip; option sweep_nb forces the count (still clamped)
  int64_t nb = nb_force > 0 ? md_strips_bands(1, nb_force, MD_FLOOR, n_red, 4 * ru) : md_strips_bands(nse, MD_NUM_CUS, MD_FLOOR, n_red, 4 * ru);
  if (outer > 1 && nb > 1 && (nse * MD_TICKET_PAD > MD_TICKET_WORDS || nb * n_out * (int64_t)sizeof(double) >= (1ll << 32))) nb = 1;
  if (ns * nb >= (1ll << 31) || (nb > 1 && ns * MD_TICKET_PAD > MD_TICKET_WORDS)) return false;
  *NS = ns;
  *NB = nb;
  return true;
}

// Plan the reduction over axis 0 of the (n_red, n_out) program in L->D with the generated sweep kernel; `store`: the evaluated value
// is written as well (one pass for an elementwise product and its reduce-to-shape). false: not applicable, L is no further.
// `batch`: `outer` problems of that shape in one launch, leaf l of batch z read from L->B.bs[l] * z on, row z of the output written.
static bool sweep_cols(const mdhip_vm_program *pr, int rop, VmLaunch *L, int64_t n_red, int64_t n_out, bool store, int64_t outer = 1,
                       bool batch = false) {
  const int64_t elems = outer * n_red * n_out, tsize = (int64_t)md_dtype_size(pr->compute_dtype);
  jit::Spec S;
  if (!jit::spec_for(&S, jit::SWEEP, pr, L->D, n_red, elems, rop, batch)) return false;
  S.store = store;
  // rows per trip: ~128 B of loads in flight per lane (a bool leaf brings 4 B per row, a float leaf 16)
  int64_t row_bytes = 0;
  for (int l = 0; l < pr->n_leaves; ++l)
    if (S.leaf_mode[l] == jit::LM_VEC) row_bytes += 4 * (int64_t)md_dtype_size(pr->leaves[l].dtype);
  const int ru_env = (int)md_opt(MD_OPT_SWEEP_RU);
  S.RU = ru_env > 0 ? ru_env : (row_bytes > 0 ? (int)((128 + row_bytes - 1) / row_bytes) : 1);
  if (S.RU > 8) S.RU = 8;
  if (S.RU < 1) S.RU = 1;
  if (!sweep_geometry(n_out, n_red, S.RU, &L->NS, &L->NB, outer)) return false;
  // streamed: the stored value and the leaves that advance from row to row (n_red >= 512 here: exactly the LM_VEC ones)
  S.nt = (store ? elems * tsize : 0) + jit::streamed_bytes(L->D, elems, true) > jit::NT_BYTES;
  // the evaluated value of a one-pass eval + column reduce is a large write next to (often much smaller) reads, and its
  // reader is whatever needed it in memory (cfg4: the weight-gradient GEMM, which is not bandwidth-bound): written around
  // the caches the pass ran 32.9 -> 26.3 us on the cfg4 shape (128 MiB out, 32 MiB mask in), the GEMM behind it unchanged (option sweep_nt_store = 0 disables)
  const int nt_store = (int)md_opt(MD_OPT_SWEEP_NT_STORE);
  S.nt_store = nt_store && store && n_red * n_out * tsize >= ((int64_t)64 << 20);
  L->fn = jit::get(S);
  if (!L->fn) return false;
  L->form = VM_COLS_STRIPS;
  L->n_red = n_red; L->n_out = n_out; L->outer = outer; L->batch = batch;
  L->grid = L->NS * L->NB;
  L->partial_bytes = L->NB > 1 ? (size_t)(outer * L->NB * n_out) * (size_t)tsize : 0;
  return true;
}

// (n_red, n_out) program reduced over its rows: the generated strips kernel, else the tiled kernels (generated or interpreted)
// with the rows split over gridDim.y and a second pass over the partial rows
static void reduce_cols_2d(const mdhip_vm_program *pr, int rop, VmLaunch *L, int64_t n_red, int64_t n_out) {
  if (sweep_cols(pr, rop, L, n_red, n_out, false)) return;
  const int64_t bx = md_ceil_div(n_out, 256);
  int64_t splits = 1024 / bx;
  if (splits > n_red / 32) splits = n_red / 32;
  if (splits > 65535) splits = 65535;
  if (splits < 1) splits = 1;
  L->form = VM_COLS_TILED;
  L->n_red = n_red; L->n_out = n_out;
  L->grid = bx;
  L->chunk = md_ceil_div(md_ceil_div(n_red, splits), 16) * 16;
  L->splits = md_ceil_div(n_red, L->chunk);
  jit::Spec S;
  if (jit::spec_for(&S, jit::RED_COLS, pr, L->D, n_red, n_red * n_out, rop)) L->fn = jit::get(S);
  L->partial_bytes = L->splits > 1 ? (size_t)(L->splits * n_out) * md_dtype_size(pr->compute_dtype) : 0;
}

// The fourth form of mdhip_vm_reduce — ONE run of adjacent reduced axes with kept axes behind it: the program seen as
// (outer, n_red, inner), inner > 1. Extent-1 axes separate nothing. false: the mask is another form's (or none).
struct VmAxisForm {
  int first, last;  // the run: axes first .. last
  int64_t outer, n_red, inner;
};
static bool axis_form(const mdhip_array *sl, uint32_t mask, VmAxisForm *F) {
  const int nd = sl->ndim;
  if (mask == 0 || nd < 2 || (mask >> nd) != 0) return false;
  int first = 0, last = nd - 1;
  while (!((mask >> first) & 1u)) ++first;
  while (!((mask >> last) & 1u)) --last;
  F->outer = F->n_red = F->inner = 1;
  for (int d = 0; d < nd; ++d) {
    const int64_t e = sl->shape[d];
    if (d < first) F->outer *= e;
    else if (d > last) F->inner *= e;
    else if (((mask >> d) & 1u) || e == 1) F->n_red *= e;
    else return false;  // a kept axis inside the run: two separated runs
  }
  F->first = first;
  F->last = last;
  return F->inner > 1;
}
// one stride for the axes [d0, d1) of a leaf (extent-1 axes skipped; 0 when there is none): false if they do not collapse
static bool group_stride(const mdhip_array &a, int d0, int d1, int64_t *stride) {
  int64_t expect = 0;
  bool have = false;
  *stride = 0;
  for (int d = d1 - 1; d >= d0; --d) {
    const int64_t e = a.shape[d];
    if (e == 1) continue;
    if (!have) { *stride = a.strides[d]; expect = a.strides[d] * e; have = true; }
    else if (a.strides[d] != expect) return false;
    else expect *= e;
  }
  return true;
}

// plan the (outer, n_red, inner) form F: the 2-D column problem, or the batched column kernels
static int reduce_axis(const mdhip_vm_program *pr, int rop, const mdhip_array *shape_like, const mdhip_array *out, const VmAxisForm &F, VmLaunch *L) {
  if (F.outer * F.n_red * F.inner == 0) return md_fail(MDHIP_EVALUE, "vm_reduce: empty operand");
  if (F.inner & 3) return md_fail(MDHIP_EVALUE, "vm_reduce: %lld kept elements behind the reduced axes are not whole 16-byte groups", (long long)F.inner);
  if (F.outer > 65535) return md_fail(MDHIP_EVALUE, "vm_reduce: %lld batches in front of the reduced axes exceed the grid (65535)", (long long)F.outer);
  if (F.inner >= (1ll << 31) || F.n_red >= (1ll << 31)) return md_fail(MDHIP_EVALUE, "vm_reduce: extents of 2^31 and more are not fused over a middle axis");
  if (!aligned16(out->data)) return md_fail(MDHIP_EVALUE, "vm_reduce: unaligned output");
  const int64_t out_elems = elems_of(out);
  if (out_elems != F.outer * F.inner)
    return md_fail(MDHIP_EVALUE, "vm_reduce: out holds %lld elements for %lld x %lld kept ones", (long long)out_elems, (long long)F.outer, (long long)F.inner);
  MdVmDev &D = L->D;
  to_dev(pr, &D);
  VmBatch &B = L->B;
  memset(&B, 0, sizeof B);
  // per leaf (s_o, s_r, s_i) from its OWN descriptor (broadcast to the program's shape already): the jointly collapsed iteration
  // merges axes across the reduced / kept boundaries when every leaf is dense
  const int nd = shape_like->ndim;
  for (int l = 0; l < pr->n_leaves; ++l) {
    const mdhip_array &a = pr->leaves[l];
    if (a.is_scalar || a.ndim != nd) return md_fail(MDHIP_EVALUE, "vm_reduce: leaf %d is not broadcast to the program's shape", l);
    for (int d = 0; d < nd; ++d)
      if (a.shape[d] != shape_like->shape[d]) return md_fail(MDHIP_EVALUE, "vm_reduce: leaf %d shape mismatch on axis %d", l, d);
    int64_t so, sr, si;
    if (!group_stride(a, 0, F.first, &so) || !group_stride(a, F.first, F.last + 1, &sr) || !group_stride(a, F.last + 1, nd, &si))
      return md_fail(MDHIP_EVALUE, "vm_reduce: leaf %d does not collapse to (outer, reduced, inner) strides", l);
    if (si != 0 && si != 1) return md_fail(MDHIP_EVALUE, "vm_reduce: leaf %d has inner stride %lld (0 or 1 are fused)", l, (long long)si);
    if (si == 1 && (!al_for(a.data, a.dtype) || (so & 3) || (sr & 3)))
      return md_fail(MDHIP_EVALUE, "vm_reduce: leaf %d is not aligned to whole 16-byte groups", l);
    D.leaf[l].os = sr;
    D.leaf[l].is = (int32_t)si;
    B.bs[l] = so;
  }
  // leading axes reduced: the 2-D column problem (n_red, inner) itself
  if (F.outer == 1) {
    reduce_cols_2d(pr, rop, L, F.n_red, F.inner);
    return MDHIP_OK;
  }
  // The batched column kernels, by size: generated strips (n_red >= 512), generated tiled, interpreter — always ONE launch, unsplit
  // over n_red except for the strips' row bands. D holds the 2-D geometry of one batch (os = the stride over n_red), B the batch strides.
  if (sweep_cols(pr, rop, L, F.n_red, F.inner, false, F.outer, true)) return MDHIP_OK;
  L->form = VM_COLS_BATCHED;
  L->n_red = F.n_red; L->n_out = F.inner; L->outer = F.outer;
  L->chunk = F.n_red;
  L->grid = md_ceil_div(F.inner, 256);
  jit::Spec S;
  if (jit::spec_for(&S, jit::RED_COLS, pr, D, F.n_red, F.outer * F.n_red * F.inner, rop, true)) L->fn = jit::get(S);
  return MDHIP_OK;
}

// Plan mdhip_vm_reduce: the program's value over `shape_like`, reduced with `rop` over the axes of `mask`
static int plan_reduce(const mdhip_vm_program *pr, int rop, const mdhip_array *shape_like, const mdhip_array *out, uint32_t mask, VmLaunch *L) {
  plan_begin(L, pr);
  const int nd = shape_like->ndim;
  const uint32_t all = nd ? ((1u << nd) - 1u) : 0u;
  VmAxisForm F;
  if (!(nd == 2 && mask == 1u) && axis_form(shape_like, mask, &F)) return reduce_axis(pr, rop, shape_like, out, F, L);
  MdVmIter &it = L->it;
  MD_TRY(md_vm_build_iter(&it, pr, shape_like, nullptr));
  if (it.total == 0) return md_fail(MDHIP_EVALUE, "vm_reduce: empty operand");
  MdVmDev &D = L->D;
  to_dev(pr, &D);
  int64_t &rows = L->rows, &inner = L->inner;
  if (!fast_geometry(it, pr->n_leaves, pr, false, &D, &rows, &inner)) return md_fail(MDHIP_EVALUE, "vm_reduce: geometry not supported");
  if (!aligned16(out->data)) return md_fail(MDHIP_EVALUE, "vm_reduce: unaligned output");
  if (mask == all) {
    jit::Spec S;
    if (jit::spec_for(&S, jit::RED_ALL, pr, D, rows, it.total, rop)) {
      S.nt = jit::streamed_bytes(D, it.total, false) > jit::NT_BYTES;
      L->fn = jit::get(S);
    }
    // read-only streams: 4 blocks per CU (cfg3 loss pass 137-143 -> 126 us)
    L->grid = L->fn ? jit::stream_grid(rows, inner, 4) : interp_grid(rows, inner);
    L->form = VM_RED_ALL;
    L->partial_bytes = (size_t)L->grid * md_dtype_size(pr->compute_dtype);
    return MDHIP_OK;
  }
  // reduce over axis 0 of a 2-D program that did NOT collapse to 1-D
  if (nd == 2 && mask == 1u && uncollapse_2d(it, pr->n_leaves, &D, shape_like->shape[0], shape_like->shape[1], &rows, &inner)) {
    reduce_cols_2d(pr, rop, L, rows, inner);
    return MDHIP_OK;
  }
  // reduce over the TRAILING axes: every axis behind the first reduced one is reduced or has extent 1, some kept axis is longer
  // than 1. The iteration is (n_out, n_red) as it stands, or one axis (all leaves dense or fully broadcast) taken apart again.
  int first = 0;
  while (first < nd && !((mask >> first) & 1u)) ++first;
  bool trailing = mask != 0 && (mask >> nd) == 0;
  int64_t n_red = 1;
  for (int d = first; d < nd; ++d) {
    if ((mask >> d) & 1u) n_red *= shape_like->shape[d];
    else trailing = trailing && shape_like->shape[d] == 1;
  }
  if (trailing && it.total / n_red > 1) {
    const int64_t n_out = it.total / n_red;
    if (!uncollapse_2d(it, pr->n_leaves, &D, n_out, n_red, &rows, &inner))
      return md_fail(MDHIP_EVALUE, "vm_reduce: a trailing-axis reduction needs (rows, reduced) geometry with rows of whole 16-byte groups");
    const int64_t out_elems = elems_of(out);
    if (out_elems != n_out) return md_fail(MDHIP_EVALUE, "vm_reduce: out holds %lld elements for %lld rows", (long long)out_elems, (long long)n_out);
    if (n_out >= (1ll << 31)) return md_fail(MDHIP_EVALUE, "vm_reduce: %lld rows exceed the grid of the row kernels", (long long)n_out);
    // long rows are walked by ONE block (generated) or wave (interpreter) each: fewer rows than CUs would leave the chip idle
    // where the eager route splits rows over blocks
    if (n_red > VM_ROWS_WAVE_MAX && n_out < VM_ROWS_MIN_OUT)
      return md_fail(MDHIP_EVALUE, "vm_reduce: %lld rows of %lld elements are too few to fill the device without splitting rows", (long long)n_out, (long long)n_red);
    L->form = VM_ROWS;
    L->n_out = n_out; L->n_red = n_red;
    L->chunk = 0;
    L->grid = md_ceil_div(n_out, MD_BLOCK / 64);
    jit::Spec S;
    if (jit::spec_for(&S, jit::RED_ROWS, pr, D, rows, it.total, rop)) {
      // streamed: the leaves that advance from row to row (a row-invariant vector is re-read from the caches)
      S.nt = jit::streamed_bytes(D, it.total, true) > jit::NT_BYTES;
      S.NV = n_red > VM_ROWS_WAVE_MAX ? 0 : rows_wave_nv(n_red);   // wave per row: 1 / 2 / 4 / 8 vector groups per lane; block per row (NV 0) above
      L->fn = jit::get(S);
      if (L->fn) L->grid = S.NV ? md_ceil_div(n_out, 4) : n_out;
    }
    return MDHIP_OK;
  }
  return md_fail(MDHIP_EVALUE, "vm_reduce: only full reductions and reductions over one run of adjacent axes are fused");
}

// Plan mdhip_vm_eval_reduce_cols: out_eval[r][c] = program(r, c) and out_red[c] = reduce over r, ONE pass (generated sweep kernel only)
static int plan_eval_reduce_cols(const mdhip_vm_program *pr, int rop, const mdhip_array *out_eval, const mdhip_array *out_red, VmLaunch *L) {
  plan_begin(L, pr);
  MD_TRY(md_vm_build_iter(&L->it, pr, out_eval, out_eval));
  if (L->it.total == 0 || out_eval->ndim != 2) return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: a non-empty 2-D program is required");
  to_dev(pr, &L->D);
  if (!fast_geometry(L->it, pr->n_leaves, pr, true, &L->D, &L->rows, &L->inner) ||
      !uncollapse_2d(L->it, pr->n_leaves, &L->D, out_eval->shape[0], out_eval->shape[1], &L->rows, &L->inner))
    return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: geometry not supported");
  if (!aligned16(out_eval->data) || !aligned16(out_red->data)) return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: unaligned output");
  if (sweep_cols(pr, rop, L, L->rows, L->inner, true)) return MDHIP_OK;
  return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: shape not covered by the one-pass kernel");
}

// ---- the runners ----
// Launch the generated kernel of a plan: nothing here depends on the reduce functor or the compute type. `out`: where a reduction
// writes (its result, or the partial rows of a split tiled pass); `outs`: what an evaluation writes (nullptr: nothing);
// `partial`: the plan's scratch where the kernel itself folds it (RED_ALL, SWEEP).
static int run_generated(const VmLaunch &L, void *out, void *const *outs, void *partial) {
  if (L.form == VM_EVAL_AXES) {
    jit::JAxArgs A;
    jit::fill_args(&A, L.D, L.imm, L.n_imm);
    for (int l = 0; l < L.D.n_leaves; ++l)
      for (int j = 0; j < 3; ++j) A.st[l][j] = L.G.st[l][j];
    for (int k = 0; k < L.n; ++k) A.outs[k] = outs[k];
    A.rows = L.G.rows;
    A.inner = L.G.nv << 2;
    A.e1 = L.G.e1;
    A.e2 = L.G.e2;
    return jit::launch(L.fn, A, dim3((unsigned)L.grid));
  }
  jit::JArgs A;
  jit::fill_args(&A, L.D, L.imm, L.n_imm);
  A.out = out;
  A.partial = partial;
  dim3 grid((unsigned)L.grid);
  switch (L.form) {
    case VM_EVAL_FAST:
      jit::args_stream(&A, L.rows, L.inner, (int)L.grid);
      for (int k = 0; k < L.n; ++k) A.outs[k] = outs[k];
      break;
    case VM_RED_ALL:
      jit::args_stream(&A, L.rows, L.inner, (int)L.grid);
      A.tickets = md_tickets();
      break;
    case VM_COLS_STRIPS:
      jit::args_shape(&A, L.n_red, L.n_out, L.n_out, L.n_red, L.NB);
      if (outs) A.outs[0] = outs[0];
      A.tickets = md_tickets();
      if (L.batch) jit::args_batch(&A, L.B, L.D.n_leaves);
      grid.y = (unsigned)L.outer;
      break;
    case VM_COLS_TILED:
      jit::args_shape(&A, L.n_red, L.n_out, L.n_out, L.n_red, L.chunk);
      grid.y = (unsigned)L.splits;
      break;
    case VM_COLS_BATCHED:
      jit::args_shape(&A, L.n_red, L.n_out, L.n_out, L.n_red, L.chunk);
      jit::args_batch(&A, L.B, L.D.n_leaves);
      grid.y = (unsigned)L.outer;
      break;
    case VM_ROWS:
      jit::args_shape(&A, L.rows, L.inner, L.n_out, L.n_red, L.chunk);
      break;
    case VM_ROWS_STAGED:
      jit::args_shape(&A, L.rows, L.inner, L.n_out, L.n_red, 0);
      A.outs[0] = outs[0];
      break;
    default:
      return vm_unplanned(L);
  }
  return jit::launch(L.fn, A, grid);
}

// the strips form: generated only, so with nothing of <R, T>. `eval_out` != nullptr: where the evaluated value goes.
static int run_strips(const VmLaunch &L, void *out, void *eval_out) {
  MdScratch scratch;
  void *partial;
  MD_TRY(scratch.get(L.partial_bytes, &partial));
  void *outs[1] = {eval_out};
  return run_generated(L, out, outs, partial);
}

template <class T, class To> static int run_eval(const VmLaunch &L, const mdhip_array *out) {
  if (L.form == VM_NONE) return MDHIP_OK;
  if (L.fn) { void *outs[1] = {out->data}; return run_generated(L, nullptr, outs, nullptr); }
  hipStream_t st = md_stream();
  To *o = (To *)out->data;
  switch (L.form) {
    case VM_EVAL_FAST:
      k_vm_eval_fast<T, To><<<(unsigned)L.grid, MD_BLOCK, 0, st>>>(L.D, o, L.rows, L.inner);
      return MD_LAUNCH_CHECK("vm_eval(fast)");
    case VM_EVAL_AXES:
      k_vm_eval_axes<T, To><<<(unsigned)L.grid, MD_BLOCK, 0, st>>>(L.D, L.G, o);
      return MD_LAUNCH_CHECK("vm_eval(axes)");
    case VM_EVAL_GENERIC:
      k_vm_eval_generic<T, To><<<(unsigned)L.grid, MD_BLOCK, 0, st>>>(L.D, L.it, o);
      return MD_LAUNCH_CHECK("vm_eval(generic)");
    default:
      return vm_unplanned(L);
  }
}

template <class R, class T> static int run_reduce(const VmLaunch &L, const mdhip_array *out) {
  if (L.form == VM_COLS_STRIPS) return run_strips(L, out->data, nullptr);
  MdScratch scratch;
  void *partial;
  MD_TRY(scratch.get(L.partial_bytes, &partial));
  hipStream_t st = md_stream();
  T *o = (T *)out->data;
  const unsigned bx = (unsigned)L.grid;
  switch (L.form) {
    case VM_RED_ALL:
      if (L.fn) return run_generated(L, o, nullptr, partial);
      k_vm_reduce_all<R, T><<<bx, MD_BLOCK, 0, st>>>(L.D, L.rows, L.inner, (T *)partial, md_tickets(), o);
      return MD_LAUNCH_CHECK("vm_reduce(all)");
    case VM_COLS_TILED: {
      if (L.splits == 1) {
        if (L.fn) return run_generated(L, o, nullptr, nullptr);
        k_vm_reduce_cols<R, T, true><<<dim3(bx, 1), MD_BLOCK, 0, st>>>(L.D, L.n_out, L.n_red, L.chunk, o, VmBatch{});
        return MD_LAUNCH_CHECK("vm_reduce(cols)");
      }
      if (L.fn) MD_TRY(run_generated(L, partial, nullptr, nullptr));
      else k_vm_reduce_cols<R, T, false><<<dim3(bx, (unsigned)L.splits), MD_BLOCK, 0, st>>>(L.D, L.n_out, L.n_red, L.chunk, (T *)partial, VmBatch{});
      // second pass: a one-instruction program over the partial buffer
      MdVmDev F;
      memset(&F, 0, sizeof F);
      F.n_instr = 1; F.n_leaves = 1;
      F.code[0].ctrl = MDHIP_VM_CTRL(MDHIP_VM_PUSH, 0, 0, 0, MDHIP_VM_SRC_LEAF, 0);
      F.leaf[0].p = partial; F.leaf[0].os = L.n_out; F.leaf[0].is = 1; F.leaf[0].dtype = md_dtype_of<T>::value;
      const int64_t chunk2 = md_ceil_div(L.splits, 16) * 16;
      k_vm_reduce_cols<R, T, true><<<dim3(bx, 1), MD_BLOCK, 0, st>>>(F, L.n_out, L.splits, chunk2, o, VmBatch{});
      return MD_LAUNCH_CHECK("vm_reduce(cols,split)");
    }
    case VM_COLS_BATCHED:
      if (L.fn) return run_generated(L, o, nullptr, nullptr);
      k_vm_reduce_cols<R, T, true, true><<<dim3(bx, 1, (unsigned)L.outer), MD_BLOCK, 0, st>>>(L.D, L.n_out, L.n_red, L.chunk, o, L.B);
      return MD_LAUNCH_CHECK("vm_reduce(cols,batched)");
    case VM_ROWS:
      if (L.fn) return run_generated(L, o, nullptr, nullptr);
      k_vm_reduce_rows<R, T><<<bx, MD_BLOCK, 0, st>>>(L.D, L.n_out, L.n_red, o);
      return MD_LAUNCH_CHECK("vm_reduce(rows)");
    default:
      return vm_unplanned(L);
  }
}

static bool rop_fused(int op) { return op == MDHIP_R_SUM || op == MDHIP_R_PROD || op == MDHIP_R_MAX || op == MDHIP_R_MIN; }

// compile-only probes have no launch geometry: read modes from the leaf descriptors as given
static void probe_modes(jit::Spec *S, const mdhip_vm_program *pr) {
  for (int l = 0; l < pr->n_leaves; ++l) {
    const mdhip_array &a = pr->leaves[l];
    bool all0 = true;
    for (int d = 0; d < a.ndim; ++d) all0 = all0 && (a.strides[d] == 0 || a.shape[d] == 1);
    const bool inner0 = a.ndim == 0 || a.strides[a.ndim - 1] == 0;
    const int slot = S->leaf_map[0][l];
    if (all0) S->leaf_mode[slot] = jit::LM_CONST;
    else if (inner0) S->leaf_mode[slot] = jit::LM_ROWB;
    else if (S->kind == jit::SWEEP && a.ndim == 2 && a.strides[0] == 0) S->leaf_mode[slot] = jit::LM_ROWINV;
    else S->leaf_mode[slot] = jit::LM_VEC;
  }
}

// .. of the batched column reductions (probe kinds 8, 9): a 3-D program whose axis 1 is the reduced one — the modes spec_modes
// gives the 2-D problem of one batch, from the strides over axes 1 and 2
static bool probe_modes_axis(jit::Spec *S, const mdhip_vm_program *pr) {
  for (int l = 0; l < pr->n_leaves; ++l) {
    const mdhip_array &a = pr->leaves[l];
    if (a.ndim != 3) return false;
    const int64_t sr = a.shape[1] == 1 ? 0 : a.strides[1], si = a.shape[2] == 1 ? 0 : a.strides[2];
    const int slot = S->leaf_map[0][l];
    if (si) S->leaf_mode[slot] = (S->kind == jit::SWEEP && sr == 0) ? jit::LM_ROWINV : jit::LM_VEC;
    else S->leaf_mode[slot] = sr == 0 ? jit::LM_CONST : jit::LM_ROWB;
  }
  return true;
}

// .. and the form of an EVAL: the axes form when the leaves, over a dense output of their shape, keep three or four collapsed
// axes (`force`: whatever they collapse to — probe kind 5); index width from the vector count
static void probe_axes(jit::Spec *S, const mdhip_vm_program *pr, bool force) {
  int nd = 0;
  int64_t total = 0;
  if (pr->n_leaves > 0) {
    mdhip_array o = pr->leaves[0];
    int64_t dense = 1;
    for (int d = o.ndim - 1; d >= 0; --d) { o.strides[d] = dense; dense *= o.shape[d]; }
    MdVmIter it;
    if (md_vm_build_iter(&it, pr, &o, &o) == MDHIP_OK) { nd = it.ndim; total = it.total; }
  }
  if (nd != 3 && nd != 4) {
    if (!force) return;
    nd = 3;
  }
  S->axes = nd;
  S->wide = (total >> 2) >= (1ll << 31) || md_opt(MD_OPT_JIT_AXES_WIDE) == 1;
}

// the end of both probes: compile the kernel of S, hand the log back
static int probe_compile(const jit::Spec &S, char *log, size_t log_cap) {
  std::vector<char> code;
  std::string l;
  const std::string name = jit::make_name(S, jit::make_key(S));
  const int rc = jit::compile(jit::gen_source(S, name), &code, &l);
  if (rc == 0) l = name + "\n" + l;  // the log of a successful probe starts with the kernel's name: which form was generated
  if (log && log_cap) { strncpy(log, l.c_str(), log_cap - 1); log[log_cap - 1] = 0; }
  if (rc != 0) return md_fail(MDHIP_ERUNTIME, "fused-kernel compilation failed: %.300s", l.c_str());
  return MDHIP_OK;
}

}  // namespace

extern "C" {

int mdhip_vm_eval(const mdhip_vm_program *pr, const mdhip_array *out) {
  int64_t staged_n_red = -1;   // >= 0: a staged program (rows kept in registers across the stages: plan_staged, or MDHIP_EVALUE and the caller composes)
  if (md_vm_is_staged(pr)) {
    MD_TRY(md_vm_check_staged(pr, nullptr, &staged_n_red));
  } else {
    MD_TRY(md_vm_check(pr));
  }
  MD_TRY(md_check_any_array(out, "vm out"));
  const bool f32 = pr->compute_dtype == MDHIP_F32;
  if (out->dtype != MDHIP_BOOL && out->dtype != MDHIP_F16 && out->dtype != pr->compute_dtype)
    return md_fail(MDHIP_ETYPE, "vm_eval: out dtype must be the compute dtype, bool or float16");
  VmLaunch L;
  MD_TRY(plan_eval(pr, out, 1, nullptr, &L, staged_n_red));
  if (out->dtype == MDHIP_BOOL) return f32 ? run_eval<float, b8>(L, out) : run_eval<double, b8>(L, out);
  if (out->dtype == MDHIP_F16) return f32 ? run_eval<float, f16>(L, out) : run_eval<double, f16>(L, out);
  return f32 ? run_eval<float, float>(L, out) : run_eval<double, double>(L, out);
}

int mdhip_vm_eval_multi(const mdhip_vm_program *progs, const mdhip_array *outs, int n) {
  if (n < 1) return md_fail(MDHIP_EVALUE, "vm_eval_multi: no programs");
  for (int k = 0; k < n; ++k) {
    MD_TRY(md_vm_check(&progs[k]));
    if (outs[k].dtype == MDHIP_F16) return md_fail(MDHIP_EVALUE, "vm_eval_multi: float16 outputs are stored by mdhip_vm_eval only");
    MD_TRY(md_check_array(&outs[k], "vm out"));
  }
  if (n > 1) {
    VmLaunch L;
    mdhip_vm_program merged;
    MD_TRY(plan_eval(progs, outs, n, &merged, &L));
    if (L.form != VM_NONE) {   // one launch for all (generated only)
      void *po[4] = {};
      for (int k = 0; k < n; ++k) po[k] = outs[k].data;
      return run_generated(L, nullptr, po, nullptr);
    }
  }
  for (int k = 0; k < n; ++k) MD_TRY(mdhip_vm_eval(&progs[k], &outs[k]));  // same results, one pass each
  return MDHIP_OK;
}

int mdhip_vm_jit_probe_multi(const mdhip_vm_program *progs, int n, char *log, size_t log_cap) {
  for (int k = 0; k < n; ++k) MD_TRY(md_vm_check(&progs[k]));
  jit::Spec M;
  mdhip_vm_program merged;
  if (!merge_programs(progs, n, &M, &merged)) return md_fail(MDHIP_EVALUE, "jit probe: programs cannot share one launch");
  for (int k = 0; k < n; ++k) {
    jit::Spec one;
    one.kind = jit::EVAL;
    for (int l = 0; l < progs[k].n_leaves; ++l) one.leaf_map[0][l] = M.leaf_map[k][l];
    probe_modes(&one, &progs[k]);
    for (int l = 0; l < progs[k].n_leaves; ++l) M.leaf_mode[M.leaf_map[k][l]] = one.leaf_mode[M.leaf_map[k][l]];
  }
  probe_axes(&M, &merged, false);
  return probe_compile(M, log, log_cap);
}

int mdhip_vm_jit_probe(const mdhip_vm_program *pr, int kind, int reduce_op, int out_is_bool, char *log, size_t log_cap) {
  if (kind == 10) {   // a staged program: NV from the row length its ROWREDs name, else from the last extent of its first leaf
    if (!md_vm_is_staged(pr)) return md_fail(MDHIP_EVALUE, "jit probe: kind 10 takes a staged program (one with a ROWRED)");
    int64_t n_red;
    MD_TRY(md_vm_check_staged(pr, nullptr, &n_red));
    if (n_red == 0 && pr->n_leaves > 0 && pr->leaves[0].ndim > 0) n_red = pr->leaves[0].shape[pr->leaves[0].ndim - 1];
    if (n_red < 4 || (n_red & 3) || n_red > VM_ROWS_STAGED_MAX) return md_fail(MDHIP_EVALUE, "jit probe: rows of %lld elements are not staged", (long long)n_red);
    jit::Spec S;
    S.kind = jit::ROWS_STAGED;
    jit::spec_single(&S, pr);
    probe_modes(&S, pr);
    if (n_red > VM_ROWS_WAVE_MAX) S.G = rows_block_g(n_red);   // a block per row
    else S.NV = rows_wave_nv(n_red);
    if (staged_held(S) > VM_STAGED_HELD_MAX) return md_fail(MDHIP_EVALUE, "jit probe: the staged program would hold %d registers per lane (max %d)", staged_held(S), VM_STAGED_HELD_MAX);
    return probe_compile(S, log, log_cap);
  }
  MD_TRY(md_vm_check(pr));
  if (kind < 0 || kind > 9)
    return md_fail(MDHIP_EVALUE, "jit probe: kind must be 0 (eval), 1 (reduce all), 2 (reduce columns, tiled), 3 (reduce columns, sweep), 4 (eval + reduce columns), 5 (eval over three / four axes), 6 (reduce rows, a wave per row), 7 (reduce rows, a block per row), 8 (reduce a middle axis, batched sweep) or 9 (reduce a middle axis, batched tiled)");
  jit::Spec S;
  S.kind = kind == 9 ? jit::RED_COLS : kind == 8 ? jit::SWEEP : kind >= 6 ? jit::RED_ROWS : kind == 5 ? jit::EVAL : kind >= 3 ? jit::SWEEP : kind;
  S.NV = kind == 6 ? 2 : 0;
  S.batch = kind >= 8;
  jit::spec_single(&S, pr);
  if (kind < 8) probe_modes(&S, pr);
  else if (!probe_modes_axis(&S, pr)) return md_fail(MDHIP_EVALUE, "jit probe: kinds 8 and 9 take a 3-D program (its axis 1 is the reduced one)");
  if (kind == 5) probe_axes(&S, pr, true);
  S.rop = reduce_op;
  S.out_bool = out_is_bool != 0 && out_is_bool != 2 && (kind == 0 || kind == 5);
  S.out_f16 = out_is_bool == 2 && (kind == 0 || kind == 5);   // (2: the float16 store of mdhip_vm_eval)
  S.store = kind == 4;
  S.Q = 4;
  S.RU = 2;
  return probe_compile(S, log, log_cap);
}

int mdhip_vm_eval_reduce_cols(const mdhip_vm_program *pr, int op, const mdhip_array *out_eval, const mdhip_array *out_red) {
  MD_TRY(md_vm_check(pr));
  if (out_eval->dtype == MDHIP_F16 || out_red->dtype == MDHIP_F16)
    return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: float16 outputs are stored by mdhip_vm_eval only");
  MD_TRY(md_check_array(out_eval, "vm out"));
  MD_TRY(md_check_array(out_red, "vm out"));
  if (out_eval->dtype != pr->compute_dtype || out_red->dtype != pr->compute_dtype)
    return md_fail(MDHIP_ETYPE, "vm_eval_reduce_cols: both outputs must have the compute dtype");
  if (!rop_fused(op)) return md_fail(MDHIP_EVALUE, "vm_eval_reduce_cols: reduce op %d is not fused", op);
  VmLaunch L;
  MD_TRY(plan_eval_reduce_cols(pr, op, out_eval, out_red, &L));
  return run_strips(L, out_red->data, out_eval->data);
}

int mdhip_vm_jit_stats(int64_t stats[2]) {
  stats[0] = jit::g_compiled;
  stats[1] = jit::g_launched;
  return MDHIP_OK;
}

int mdhip_vm_reduce(const mdhip_vm_program *pr, int op, const mdhip_array *shape_like, const mdhip_array *out, uint32_t mask) {
  MD_TRY(md_vm_check(pr));
  MD_TRY(md_check_array(shape_like, "vm shape"));
  MD_TRY(md_check_array(out, "vm out"));
  if (out->dtype != pr->compute_dtype) return md_fail(MDHIP_ETYPE, "vm_reduce: out dtype must be the compute dtype");
  if (!rop_fused(op)) return md_fail(MDHIP_EVALUE, "vm_reduce: reduce op %d is not fused", op);
  VmLaunch L;
  MD_TRY(plan_reduce(pr, op, shape_like, out, mask, &L));
#define MD_VMR(R) return pr->compute_dtype == MDHIP_F32 ? run_reduce<R, float>(L, out) : run_reduce<R, double>(L, out)
  switch (op) {
    case MDHIP_R_SUM: MD_VMR(RSum);
    case MDHIP_R_PROD: MD_VMR(RProd);
    case MDHIP_R_MAX: MD_VMR(RMax);
    default: MD_VMR(RMin);
  }
#undef MD_VMR
}

}  // extern "C"
