// moments.hip — variance / standard deviation along one axis in ONE entry point (mdhip_var).
//
// Serves reference minidiff/backend/numpy.py:57 (np.std) as called by minidiff/ops/definitions.py:209-221 (forward AND the vjp,
// which evaluates std(x) again). NumPy's _methods._var is mean -> x - mean -> square -> sum -> divide (-> sqrt): composed from the
// other entry points that is four reads and two writes of the array (977 GB/s of algorithmic bytes on 8192 x 4096 float32). Here:
//   rows    (the reduced axis is the contiguous one): a row of up to 16 Ki elements is read ONCE into registers — sum, mean (a true
//           division, as NumPy), centred squares, all from the registers; longer rows are read twice (the second time from cache);
//   columns (axis 0 of a row-major matrix): the column sums by mdhip_reduce's strips kernel, then one more strips walk that adds
//           (x - mean)^2 — two reads, the last block of a strip folds the band partials in band order and finishes the division
//           (the band count is md_strips.h's, as for every strips walk; the scratch blocks live in an MdScratch);
//   a middle axis ((outer, n, inner) with inner contiguous: the statistics of a normalisation over the sequence axis): `outer`
//           independent column problems — the batched column sums of mdhip_reduce, then ONE batched launch of the same second walk
//           (the batch on blockIdx.y, per-batch offsets into x, the sums, the partial rows, the ticket words and out).
// Same arithmetic as NumPy up to the order of the two sums (no Welford update, no E[x^2] - mean^2 cancellation). HBM-bound:
// algorithmic bytes = one read of x.
// x may also have a storage-only dtype (float16, int8/16, uint8/16/32/64): every kernel carries a storage type S beside the carrier T —
// 16-B loads of S (16 / sizeof(S) elements), each element converted in registers: float16 -> float (the result rounded to float16
// once), the integers -> double straight from their own type (uint64: its whole range; the result is float64). The first pass of
// the column forms is then mdhip_reduce's strips kernel with the same S. Option var_narrow 0 refuses such x (A/B).
#include "md_hip.h"
#include "md_narrow.h"
#include "md_strips.h"

extern "C" int mdhip_reduce(int op, const mdhip_array *x, const mdhip_array *out, uint32_t axis_mask);

namespace {

template <class T> __device__ __forceinline__ T md_shfl_xor_t(T v, int m) {
  if constexpr (sizeof(T) == 8) {
    union { T t; int w[2]; } u;
    u.t = v;
    u.w[0] = __shfl_xor(u.w[0], m, 64);
    u.w[1] = __shfl_xor(u.w[1], m, 64);
    return u.t;
  } else {
    union { T t; int w; } u;
    u.t = v;
    u.w = __shfl_xor(u.w, m, 64);
    return u.t;
  }
}
template <class T> __device__ __forceinline__ T wave_sum_all(T v) {   // every lane gets the sum (fixed butterfly)
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += md_shfl_xor_t(v, m);
  return v;
}

// The compiler may not carry anything it derived from this 16-B vector across this point (the bits themselves stay in their registers).
template <class Vec> __device__ __forceinline__ void md_opaque16(Vec &v) {
  static_assert(sizeof(Vec) == 16, "one 16-B vector");
  md_i32x4 t;
  __builtin_memcpy(&t, &v, 16);
  asm volatile("" : "+v"(t));
  __builtin_memcpy(&v, &t, 16);
}

// One row per GROUP of G lanes-worth of threads: G = 64 (a wave, four rows per block) or 256 (the block). NV: 16-B vectors of the
// row cached per thread (0: the row does not fit, read it twice).
// S: the row's storage type — T itself, or a storage-only dtype (float16 with T = float, the small integers with T = double): the
// 16-B vectors are loaded and CACHED in S (16 / sizeof(S) elements each: a cached row of int8 is 16 x the elements of a double one in
// the same registers), every element converted to T in registers where it is used. To: the result's type (float16 for float16 x —
// the float value rounded once; otherwise T).
template <class T, int G, int NV, class S = T, class To = T>
__global__ void __launch_bounds__(256) k_var_rows(const S *__restrict__ x, int64_t n_rows, int64_t n, To *__restrict__ out, T denom, int take_sqrt) {
  constexpr int V = 16 / sizeof(S);
  typedef MdVec<S, V> Vec;
  __shared__ T red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = G == 64 ? (int64_t)blockIdx.x * 4 + w : (int64_t)blockIdx.x;
  const int tig = G == 64 ? lane : (int)threadIdx.x;   // thread in group
  const bool live = row < n_rows;
  const Vec *p = reinterpret_cast<const Vec *>(x + (live ? row : 0) * n);
  const int64_t nvec = n / V;
  auto group_sum = [&](T v) -> T {
    v = wave_sum_all(v);
    if constexpr (G == 256) {
      __syncthreads();   // (red is reused)
      if (lane == 0) red[w] = v;
      __syncthreads();
      v = (red[0] + red[1]) + (red[2] + red[3]);
    }
    return v;
  };
  T s = (T)0;
  if constexpr (NV > 0) {
    Vec c[NV];
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int64_t i = tig + (int64_t)g * G;
      if (i < nvec) c[g] = p[i];
      else c[g] = Vec{};   // (zeros of S)
    }
#pragma unroll
    for (int g = 0; g < NV; ++g)
#pragma unroll
      for (int j = 0; j < V; ++j) s += md_cast<T>(c[g].v[j]);
    const T mean = group_sum(s) / (T)n;
    if constexpr (!md_same<S, T>::value) {
      // the second walk converts the cached vectors AGAIN: left alone the compiler keeps every converted element of the first walk
      // alive — NV x V values of T, 512 registers for sixteen vectors of int8 — and spills
#pragma unroll
      for (int g = 0; g < NV; ++g) md_opaque16(c[g]);
    }
    T q = (T)0;
#pragma unroll
    for (int g = 0; g < NV; ++g) {
      const int64_t i = tig + (int64_t)g * G;
      if (i < nvec) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const T d = md_cast<T>(c[g].v[j]) - mean;
          q = fma(d, d, q);
        }
      }
    }
    q = group_sum(q);
    if (live && tig == 0) {
      const T v = q / denom;
      out[row] = md_cast<To>(take_sqrt ? sqrt(v) : v);
    }
  } else {
    for (int64_t i = tig; i < nvec; i += G) {
      const Vec t = p[i];
#pragma unroll
      for (int j = 0; j < V; ++j) s += md_cast<T>(t.v[j]);
    }
    const T mean = group_sum(s) / (T)n;
    T q = (T)0;
    for (int64_t i = tig; i < nvec; i += G) {
      const Vec t = p[i];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T d = md_cast<T>(t.v[j]) - mean;
        q = fma(d, d, q);
      }
    }
    q = group_sum(q);
    if (live && tig == 0) {
      const T v = q / denom;
      out[row] = md_cast<To>(take_sqrt ? sqrt(v) : v);
    }
  }
}

// Second pass of the column form: out[c] = f( sum_r (x[r][c] - csum[c] / n)^2 / denom ). The walk of k_reduce_cols_strips (reduce.hip):
// NS strips x NB bands, rows interleaved across bands and waves, batches of RB rows double-buffered, ticket finish.
// blockIdx.y: one of several independent (n_red x n_out) problems (a MIDDLE axis reduced) — x_bs elements apart in x, o_bs in csum and
// out, p_bs in the partial rows; each has its own strip tickets. The 2-D form is the one-batch launch (strides 0).
// S, To: as in k_var_rows — x is loaded in its storage type, one 16-B vector = V = 16 / sizeof(S) columns per lane (16 of int8);
// the means, the accumulators, the LDS rows, the band partials and the sums are T's (V of them per lane: 16 doubles are eight
// 16-B words per partial row and lane), the result is To's.
template <class T, int RB, class S = T, class To = T>
__global__ void __launch_bounds__(256) k_var_cols(const S *__restrict__ x, const T *__restrict__ csum, int64_t n_out, int64_t n_red, int NS, int NB,
                                                  T *partial, unsigned *tickets, To *__restrict__ out, T denom, int take_sqrt,
                                                  int64_t x_bs, int64_t o_bs, int64_t p_bs) {
  constexpr int V = 16 / sizeof(S);
  typedef MdVec<S, V> XVec;     // one 16-B load of x
  typedef MdVec<T, V> Vec;      // the same columns in the carrier type
  typedef MdVec<To, V> OVec;
  __shared__ Vec sm[3][64];
  __shared__ unsigned last_flag;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int s = blockIdx.x % NS, b = blockIdx.x / NS;
  x += (int64_t)blockIdx.y * x_bs;
  csum += (int64_t)blockIdx.y * o_bs;
  out += (int64_t)blockIdx.y * o_bs;
  if (NB > 1) partial += (int64_t)blockIdx.y * p_bs;
  tickets += (int64_t)blockIdx.y * NS * MD_TICKET_PAD;
  const int64_t col_raw = ((int64_t)s * 64 + lane) * V;
  const bool col_ok = col_raw < n_out;
  const int64_t col = col_ok ? col_raw : n_out - V;
  const int64_t first = b + (int64_t)NB * w, step = (int64_t)NB * 4;
  const int64_t nrw = first < n_red ? (n_red - first + step - 1) / step : 0;
  const int64_t nb = nrw / RB;
  const Vec cs = *reinterpret_cast<const Vec *>(csum + col);
  T mean[V], acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { mean[j] = cs.v[j] / (T)n_red; acc[j] = (T)0; }
  const S *p = x + col + first * n_out;
  const int64_t rstep = step * n_out;
  XVec t[2][RB];
  auto load = [&](int buf, int64_t bt) {
    const int64_t i0 = (bt < nb ? bt : nb - 1) * RB;
#pragma unroll
    for (int u = 0; u < RB; ++u) t[buf][u] = *reinterpret_cast<const XVec *>(p + (i0 + u) * rstep);
  };
  auto add = [&](int buf) {
#pragma unroll
    for (int u = 0; u < RB; ++u)
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const T d = md_cast<T>(t[buf][u].v[j]) - mean[j];
        acc[j] = fma(d, d, acc[j]);
      }
  };
  if (nb > 0) {
    load(0, 0);
    int64_t bt = 0;
    for (; bt + 1 < nb; bt += 2) {
      load(1, bt + 1);
      __builtin_amdgcn_sched_barrier(0);
      add(0);
      __builtin_amdgcn_sched_barrier(0);
      load(0, bt + 2);
      __builtin_amdgcn_sched_barrier(0);
      add(1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (bt < nb) add(0);
  }
  for (int64_t i = nb * RB; i < nrw; ++i) {
    const XVec tt = *reinterpret_cast<const XVec *>(p + i * rstep);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const T d = md_cast<T>(tt.v[j]) - mean[j];
      acc[j] = fma(d, d, acc[j]);
    }
  }
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) sm[w - 1][lane].v[j] = acc[j];
  }
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += sm[k][lane].v[j];
  }
  auto finish = [&]() {
    OVec o;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const T v = acc[j] / denom;
      o.v[j] = md_cast<To>(take_sqrt ? sqrt(v) : v);
    }
    *reinterpret_cast<OVec *>(out + col) = o;
  };
  if (NB == 1) {
    if (w == 0 && col_ok) finish();
    return;
  }
  const __amdgpu_buffer_rsrc_t pr = md_rsrc(partial, (unsigned)((int64_t)NB * n_out * (int64_t)sizeof(T)));
  if (w == 0 && col_ok) {
    Vec o;
#pragma unroll
    for (int j = 0; j < V; ++j) o.v[j] = acc[j];
    md_st16_sc1(pr, (unsigned)(((int64_t)b * n_out + col) * (int64_t)sizeof(T)), o);
  }
  if (!md_ticket_last(tickets + s * MD_TICKET_PAD, (unsigned)NB, &last_flag)) return;
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = (T)0;
  for (int r = w; r < NB; r += 4) {
    const Vec pt = md_ld16_sc1<Vec>(pr, (unsigned)(((int64_t)r * n_out + col) * (int64_t)sizeof(T)));
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] += pt.v[j];
  }
  __syncthreads();
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < V; ++j) sm[w - 1][lane].v[j] = acc[j];
  }
  __syncthreads();
  if (w == 0 && col_ok) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += sm[k][lane].v[j];
    finish();
  }
}

// The form is chosen by 16-B vectors per row, whatever the element size: what a thread caches is NV vectors = 4 NV registers, and the
// converted values live only while they are added. In elements the thresholds therefore scale with V = 16 / sizeof(S): a wave caches
// rows of up to 512 vectors (2048 float32, 4096 float16, 8192 int8), a block up to 4096 vectors (64 KiB: 65536 int8), longer rows
// are read twice.
template <class T, class S = T, class To = T> int var_rows(const S *x, int64_t n_rows, int64_t n, To *out, T denom, int take_sqrt) {
  constexpr int V = 16 / sizeof(S);
  const int64_t nvec = n / V;
  if (n_rows > (1ll << 31) - 8) return md_fail(MDHIP_EVALUE, "var: too many rows for one launch");
  if (nvec <= 64 * 8) {
    const unsigned grid = (unsigned)((n_rows + 3) / 4);
    if (nvec <= 64 * 2) MD_LAUNCH((k_var_rows<T, 64, 2, S, To>), grid, 256, x, n_rows, n, out, denom, take_sqrt);
    else if (nvec <= 64 * 4) MD_LAUNCH((k_var_rows<T, 64, 4, S, To>), grid, 256, x, n_rows, n, out, denom, take_sqrt);
    else MD_LAUNCH((k_var_rows<T, 64, 8, S, To>), grid, 256, x, n_rows, n, out, denom, take_sqrt);
  } else if (nvec <= 256 * 4) {
    MD_LAUNCH((k_var_rows<T, 256, 4, S, To>), (unsigned)n_rows, 256, x, n_rows, n, out, denom, take_sqrt);
  } else if (nvec <= 256 * 16) {
    MD_LAUNCH((k_var_rows<T, 256, 16, S, To>), (unsigned)n_rows, 256, x, n_rows, n, out, denom, take_sqrt);
  } else {
    MD_LAUNCH((k_var_rows<T, 256, 0, S, To>), (unsigned)n_rows, 256, x, n_rows, n, out, denom, take_sqrt);
  }
  return MD_LAUNCH_CHECK("var(rows)");
}

// `outer` column problems of n_red x n_out, n_red * n_out elements apart (outer == 1: the 2-D form). x has dtype `xdtype` (S), the
// sums and partial rows the carrier's `cdtype` (T).
template <class T, class S = T, class To = T>
int var_cols(const void *xdata, int64_t outer, int64_t n_red, int64_t n_out, To *out, T denom, int take_sqrt, int xdtype, int cdtype) {
  constexpr int V = 16 / sizeof(S);
  MdScratch scratch;   // (freed on every way out, stream-ordered behind the launches)
  void *csum, *partial;
  MD_TRY(scratch.get((size_t)(outer * n_out) * sizeof(T), &csum));
  mdhip_array xd{}, sd{};
  xd.data = const_cast<void *>(xdata); xd.dtype = xdtype;
  sd.data = csum; sd.dtype = cdtype;
  uint32_t mask;
  if (outer == 1) {
    xd.ndim = 2; xd.shape[0] = n_red; xd.shape[1] = n_out; xd.strides[0] = n_out; xd.strides[1] = 1;
    sd.ndim = 2; sd.shape[0] = 1; sd.shape[1] = n_out; sd.strides[0] = n_out; sd.strides[1] = 1;
    mask = 1u;
  } else {   // (the batched strips launch of reduce.hip; whichever kernel it picks, csum holds the column sums)
    xd.ndim = 3; xd.shape[0] = outer; xd.shape[1] = n_red; xd.shape[2] = n_out; xd.strides[0] = n_red * n_out; xd.strides[1] = n_out; xd.strides[2] = 1;
    sd.ndim = 3; sd.shape[0] = outer; sd.shape[1] = 1; sd.shape[2] = n_out; sd.strides[0] = n_out; sd.strides[1] = n_out; sd.strides[2] = 1;
    mask = 1u << 1;
  }
  MD_TRY(mdhip_reduce(MDHIP_R_SUM, &xd, &sd, mask));
  const int64_t NS = (n_out + 64 * V - 1) / (64 * V);
  // 2-D: ~1024 blocks (rounded up); batched: one block per CU (rounded down), as the batched column sums
  int64_t NB = outer == 1 ? md_strips_bands(NS, 1024, MD_CEIL, n_red, 32) : md_strips_bands(NS * outer, MD_NUM_CUS, MD_FLOOR, n_red, 32);
  if (NS * outer * MD_TICKET_PAD > MD_TICKET_WORDS) NB = 1;   // more strips than ticket words: one band (a plain column sum declines instead)
  while (NB > 1 && NB * n_out * (int64_t)sizeof(T) >= (1ll << 31)) NB /= 2;   // (32-bit byte offsets into a batch's partial rows of T)
  MD_TRY(scratch.get(NB > 1 ? (size_t)(outer * NB * n_out) * sizeof(T) : 0, &partial));
  // from one batch to the next: elements in x, in the sums and out, in the partial rows (2-D: one batch, no steps)
  struct { int64_t x, o, p; } step = {0, 0, 0};
  if (outer > 1) step = {n_red * n_out, n_out, NB * n_out};
  const dim3 grid((unsigned)(NS * NB), (unsigned)outer);
  MD_LAUNCH((k_var_cols<T, 8, S, To>), grid, 256, (const S *)xdata, (const T *)csum, n_out, n_red, (int)NS, (int)NB, (T *)partial, md_tickets(), out, denom, take_sqrt,
            step.x, step.o, step.p);
  return MD_LAUNCH_CHECK(outer == 1 ? "var(cols)" : "var(cols,batched)");
}

// rows (inner == 1) or columns of one (carrier, storage, result) triple; the floors were checked by the caller
template <class T, class S, class To>
int var_run(const mdhip_array *x, const mdhip_array *out, int64_t outer, int64_t n, int64_t inner, double denom, int take_sqrt, int cdtype) {
  if (inner == 1) return var_rows<T, S, To>((const S *)x->data, outer, n, (To *)out->data, (T)denom, take_sqrt);
  return var_cols<T, S, To>(x->data, outer, n, inner, (To *)out->data, (T)denom, take_sqrt, x->dtype, cdtype);
}

}  // namespace

extern "C" int mdhip_var(const mdhip_array *x, const mdhip_array *out, int32_t axis, int64_t ddof, int take_sqrt) {
  MD_TRY(md_check_any_array(x, "var x"));
  MD_TRY(md_check_any_array(out, "var out"));
  // storage-only x (float16, int8/16, uint8/16/32/64): read in its own type. (A/B: option var_narrow 0 refuses it — the caller promotes)
  const bool narrow = md_is_narrow(x->dtype);
  if (narrow && !md_opt(MD_OPT_VAR_NARROW)) return md_fail(MDHIP_EVALUE, "var: storage-only x and option var_narrow is 0 (the caller promotes and composes)");
  if (!narrow && x->dtype != MDHIP_F32 && x->dtype != MDHIP_F64)
    return md_fail(MDHIP_EVALUE, "var: float32 / float64 / storage-only dtypes only (the caller composes the rest)");
  // NumPy's result dtype: the float's own (float16: float32 arithmetic, rounded once), float64 for the integers
  const int want = !narrow ? x->dtype : x->dtype == MDHIP_F16 ? MDHIP_F16 : MDHIP_F64;
  if (out->dtype != want) return md_fail(MDHIP_ETYPE, "var: out dtype must be %s for x of %s", md_dtype_name(want), md_dtype_name(x->dtype));
  if (axis < 0 || axis >= x->ndim) return md_fail(MDHIP_EVALUE, "var: axis out of range");
  // x must be C-contiguous: viewed as (outer, n, inner)
  int64_t acc = 1, outer = 1, inner = 1;
  for (int d = x->ndim - 1; d >= 0; --d) {
    if (x->shape[d] != 1 && x->strides[d] != acc) return md_fail(MDHIP_EVALUE, "var: x is not C-contiguous");
    acc *= x->shape[d];
    if (d > axis) inner *= x->shape[d];
    if (d < axis) outer *= x->shape[d];
  }
  const int64_t n = x->shape[axis];
  if (n - ddof <= 0 || n < 2 || outer * inner == 0) return md_fail(MDHIP_EVALUE, "var: degenerate count (the caller composes NumPy's nan / inf)");
  int64_t osz = 1, oacc = 1;
  for (int d = out->ndim - 1; d >= 0; --d) {
    if (out->shape[d] != 1 && out->strides[d] != oacc) return md_fail(MDHIP_EVALUE, "var: out is not C-contiguous");
    oacc *= out->shape[d];
    osz *= out->shape[d];
  }
  if (osz != outer * inner) return md_fail(MDHIP_EVALUE, "var: out has %lld elements, expected %lld", (long long)osz, (long long)(outer * inner));
  // (A/B: with option var_batched 0 only the last axis and the first of a 2-D array are served, as before the batched column form)
  if (!md_opt(MD_OPT_VAR_BATCHED) && !(axis == x->ndim - 1 || (axis == 0 && x->ndim == 2)))
    return md_fail(MDHIP_EVALUE, "var: neither the last axis nor the first of a 2-D array, and option var_batched is 0 (the caller composes)");
  const int64_t V = 16 / (int64_t)md_dtype_size(x->dtype);   // elements of x per 16-B vector: 2 .. 16
  if (((uintptr_t)x->data & 15) || ((uintptr_t)out->data & 15)) return md_fail(MDHIP_EVALUE, "var: unaligned operands");
  const double denom = (double)(n - ddof);
  if (inner == 1) {
    if (n % V) return md_fail(MDHIP_EVALUE, "var: row length not a multiple of the 16-B vector");
    // a row is one wave's / one block's work: a few very long rows would leave the chip idle (the composed passes use all of it).
    // Storage-only x: a row longer than the block's register cache (4096 vectors = 64 KiB) — the same 16384 elements in float32
    if (outer < 256 && n > (narrow ? 4096 * V : 16384)) return md_fail(MDHIP_EVALUE, "var: few long rows (the caller composes)");
  } else {
    // (a lane owns V columns and the last strip is clamped to col = inner - V: inner >= V, which 256 covers — V <= 16)
    if ((inner % V) || n < 64 || inner < 256) return md_fail(MDHIP_EVALUE, "var: column form needs >= 256 aligned columns and >= 64 rows");
    // outer > 1: `outer` column problems in one launch (the batch rides on blockIdx.y)
    if (outer > 65535) return md_fail(MDHIP_EVALUE, "var: reduced axis in the middle of more than 65535 batches (the caller composes)");
  }
  switch (x->dtype) {
    case MDHIP_F32: return var_run<float, float, float>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F32);
    case MDHIP_F64: return var_run<double, double, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    case MDHIP_F16: return var_run<float, f16, f16>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F32);
    case MDHIP_I8: return var_run<double, int8_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    case MDHIP_I16: return var_run<double, int16_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    case MDHIP_U8: return var_run<double, uint8_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    case MDHIP_U16: return var_run<double, uint16_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    case MDHIP_U32: return var_run<double, uint32_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);
    default: return var_run<double, uint64_t, double>(x, out, outer, n, inner, denom, take_sqrt, MDHIP_F64);   // uint64
  }
}

