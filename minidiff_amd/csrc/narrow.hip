// narrow.hip — elementwise kernels for the storage-only dtypes (int8/16, uint8/16/32/64, float16) and for mixed calls that
// involve one: ONE launch, every operand read once in its own storage type, the result written once in its own
// (round 3 ran these as promote -> wide kernel -> demote: three launches and >= 3x the algorithmic traffic).
//
// Serves the same backend names as elementwise.hip (reference minidiff/backend/numpy.py:19-95) for the dtypes of
// numpy.py:188-200 beyond bool / int32 / int64 / float32 / float64. Semantics and the carrier types: md_narrow.h.
//
// Two kernel families:
//  * stream  — every array operand contiguous, of ONE storage type S (the loop dtype's), the other operand possibly a scalar;
//              output contiguous of type S (arithmetic) or bool (comparisons). 16 B per lane and load — 16 int8, 8 float16 /
//              int16, 4 uint32, 2 uint64 elements — two vectors per lane and trip, grid-stride, non-temporal above the
//              Infinity Cache. HBM-bound at (operand bytes + result bytes): int8 * int8 moves 3 bytes per element.
//  * generic — any strides, any mix of the twelve dtypes: wave-uniform dtype switches around a div/mod walk.
// Between them: 16-B vector kernels under a broadcast (k_nw_binary_axes, k_nw_where_axes), and mdhip_convert's vector kernels
// (k_nw_convert, k_nw_convert_axes: astype and every copy of a storage-only array, any pair of the twelve dtypes).
#include "md_hip.h"
#include "md_narrow.h"

namespace {

enum { NM_VEC = 1, NM_SCAL = 2 };

template <bool NT, class V> __device__ __forceinline__ V nw_ld(const V *p) {
  if constexpr (sizeof(V) == 16 && NT) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4 t = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(p));
    V v;
    __builtin_memcpy(&v, &t, 16);
    return v;
  } else {
    return *p;
  }
}
template <bool NT, class V> __device__ __forceinline__ void nw_st(V *p, const V &v) {
  if constexpr (sizeof(V) == 16 && NT) {
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    i32x4 t;
    __builtin_memcpy(&t, &v, 16);
    __builtin_nontemporal_store(t, reinterpret_cast<i32x4 *>(p));
  } else if constexpr (sizeof(V) == 8 && NT) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    i32x2 t;
    __builtin_memcpy(&t, &v, 8);
    __builtin_nontemporal_store(t, reinterpret_cast<i32x2 *>(p));
  } else {
    *p = v;
  }
}

// result storage of functor F over carrier Tc for loop storage S: S itself, or bool for the comparison / logical family
template <class F, class Tc, class S> struct nw_out {
  using R = decltype(F::apply(Tc(), Tc()));
  using type = typename md_cond<md_same<R, b8>::value, b8, S>::type;
};
template <class F, class Tc, class S> struct nw_out1 {
  using R = decltype(F::apply(Tc()));
  using type = typename md_cond<md_same<R, b8>::value, b8, S>::type;
};

// The scalar elements behind the last vector round float32 -> float16 with the bit routine: a plain conversion next to the float32
// multiply was selected together with it as v_fma_mixlo_f16 x, y, +0 — fma(x, y, +0) is x * y except for a product of -0.0, which came
// out +0.0 (k_nw_binary<BMul, float, f16> with a scalar operand; found by tests/test_elementwise_paths.py). The vectors of the main
// loops convert in pairs (v_cvt_pk_f16_f32) and are not affected.
template <class So, class R> __device__ __forceinline__ So nw_tail_cast(R r) {
  if constexpr (md_same<So, f16>::value && md_same<R, float>::value) {
    f16 h;
    h.bits = md_double_to_half((double)r);
    return h;
  } else {
    return md_cast<So>(r);
  }
}

// ------------------------------------------------------- broadcasts, 16-B vectors ----
// Two to four collapsed axes with the inner axis contiguous or broadcast in every operand ((R, C) + (C,), (B, R, C) * (B, 1, C) in
// float16 / int8 ..): a lane owns one 16-B vector of the OUTPUT's storage type count (8 float16, 16 int8 ..); the scheme of
// elementwise.hip's k_ew_axes. Was the one-element generic kernel (~350 GB/s).
struct NwAxes {
  int64_t e0, e1, e2, nv, rows;
  int64_t st[2][3];
  int in[2];
};
template <class F, class Tc, class S>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_binary_axes(NwAxes g, const S *__restrict__ a, const S *__restrict__ b, Tc sa, Tc sb,
                                                            typename nw_out<F, Tc, S>::type *__restrict__ out) {
  using So = typename nw_out<F, Tc, S>::type;
  constexpr int E = 16 / sizeof(S);
  typedef MdVec<S, E> Vin;
  typedef MdVec<So, E> Vout;
  const int64_t total = g.rows * g.nv, gs = (int64_t)gridDim.x * MD_BLOCK;
  auto load = [&](const S *p, Tc s, int in, int64_t off, int64_t c, Tc (&r)[E]) {
    if (p == nullptr) {
#pragma unroll
      for (int j = 0; j < E; ++j) r[j] = s;
    } else if (in) {
      const Vin t = *reinterpret_cast<const Vin *>(p + off + c);
#pragma unroll
      for (int j = 0; j < E; ++j) r[j] = md_cast<Tc>(t.v[j]);
    } else {
      const Tc t = md_cast<Tc>(p[off]);
#pragma unroll
      for (int j = 0; j < E; ++j) r[j] = t;
    }
  };
  for (int64_t v = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x; v < total; v += gs) {
    const int64_t row = v / g.nv, q = row / g.e2, r2 = row - q * g.e2;
    int64_t r0 = 0, r1 = q;
    if (g.e0 != 1) { r0 = q / g.e1; r1 = q - r0 * g.e1; }
    const int64_t c = (v - row * g.nv) * E;
    Tc x[E], y[E];
    load(a, sa, g.in[0], r0 * g.st[0][0] + r1 * g.st[0][1] + r2 * g.st[0][2], c, x);
    load(b, sb, g.in[1], r0 * g.st[1][0] + r1 * g.st[1][1] + r2 * g.st[1][2], c, y);
    Vout o;
#pragma unroll
    for (int j = 0; j < E; ++j) o.v[j] = md_cast<So>(F::apply(x[j], y[j]));
    *reinterpret_cast<Vout *>(out + row * (g.nv * E) + c) = o;
  }
}

// ------------------------------------------------------------------- stream ----
template <class F, class Tc, class S, int MA, int MB, bool NT>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_binary(const S *__restrict__ a, const S *__restrict__ b, Tc sa, Tc sb,
                                                       typename nw_out<F, Tc, S>::type *__restrict__ out, int64_t n) {
  using So = typename nw_out<F, Tc, S>::type;
  constexpr int E = 16 / sizeof(S);
  typedef MdVec<S, E> Vin;
  typedef MdVec<So, E> Vout;
  const int64_t nv = n / E, gs = (int64_t)gridDim.x * MD_BLOCK, gid = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  const Vin *pa = reinterpret_cast<const Vin *>(a), *pb = reinterpret_cast<const Vin *>(b);
  Vout *po = reinterpret_cast<Vout *>(out);
  auto one = [&](const Vin &va, const Vin &vb, int64_t i) {
    Vout o;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const Tc x = MA == NM_VEC ? md_cast<Tc>(va.v[j]) : sa, y = MB == NM_VEC ? md_cast<Tc>(vb.v[j]) : sb;
      o.v[j] = md_cast<So>(F::apply(x, y));
    }
    nw_st<NT>(po + i, o);
  };
  int64_t i = gid;
  // two vectors per operand in flight on the cached path, ONE on the non-temporal path (as the wide kernels, elementwise.hip
  // MD_EW_UNROLL_NT: more in flight ran slower on streams that bypass the caches — here 59.5 -> 6x % for int8 * int8 on 2**30 elements)
  if constexpr (!NT) {
    for (; i + gs < nv; i += 2 * gs) {
      Vin a0, a1, b0, b1;
      if constexpr (MA == NM_VEC) { a0 = nw_ld<NT>(pa + i); a1 = nw_ld<NT>(pa + i + gs); }
      if constexpr (MB == NM_VEC) { b0 = nw_ld<NT>(pb + i); b1 = nw_ld<NT>(pb + i + gs); }
      one(a0, b0, i);
      one(a1, b1, i + gs);
    }
  }
  for (; i < nv; i += gs) {
    Vin a0, b0;
    if constexpr (MA == NM_VEC) a0 = nw_ld<NT>(pa + i);
    if constexpr (MB == NM_VEC) b0 = nw_ld<NT>(pb + i);
    one(a0, b0, i);
  }
  const int64_t t = nv * E + gid;   // the up-to-(E-1) elements behind the last whole vector
  if (t < n) {
    const Tc x = MA == NM_VEC ? md_cast<Tc>(a[t]) : sa, y = MB == NM_VEC ? md_cast<Tc>(b[t]) : sb;
    out[t] = nw_tail_cast<So>(F::apply(x, y));
  }
}

template <class F, class Tc, class S, bool NT>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_unary(const S *__restrict__ x, typename nw_out1<F, Tc, S>::type *__restrict__ out, int64_t n) {
  using So = typename nw_out1<F, Tc, S>::type;
  constexpr int E = 16 / sizeof(S);
  typedef MdVec<S, E> Vin;
  typedef MdVec<So, E> Vout;
  const int64_t nv = n / E, gs = (int64_t)gridDim.x * MD_BLOCK, gid = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  const Vin *px = reinterpret_cast<const Vin *>(x);
  Vout *po = reinterpret_cast<Vout *>(out);
  auto one = [&](const Vin &v, int64_t i) {
    Vout o;
#pragma unroll
    for (int j = 0; j < E; ++j) o.v[j] = md_cast<So>(F::apply(md_cast<Tc>(v.v[j])));
    nw_st<NT>(po + i, o);
  };
  int64_t i = gid;
  if constexpr (!NT) {
    for (; i + gs < nv; i += 2 * gs) {
      const Vin v0 = nw_ld<NT>(px + i), v1 = nw_ld<NT>(px + i + gs);
      one(v0, i);
      one(v1, i + gs);
    }
  }
  for (; i < nv; i += gs) one(nw_ld<NT>(px + i), i);
  const int64_t t = nv * E + gid;
  if (t < n) out[t] = nw_tail_cast<So>(F::apply(md_cast<Tc>(x[t])));
}

// ------------------------------------------------------------------ generic ----
template <class F, class Tc>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_unary_generic(MdIter it, const void *x, int xdt, int x_scalar, Tc sx, void *out, int odt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < it.total; i += stride) {
    int64_t offs[MD_MAX_OPS];
    md_iter_offsets(it, i, offs);
    const Tc v = x_scalar ? sx : md_load<Tc>(x, xdt, offs[0]);
    md_store_as(out, odt, offs[1], F::apply(v));
  }
}
template <class F, class Tc>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_binary_generic(MdIter it, const void *a, int adt, int a_scalar, Tc sa, const void *b, int bdt,
                                                               int b_scalar, Tc sb, void *out, int odt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < it.total; i += stride) {
    int64_t offs[MD_MAX_OPS];
    md_iter_offsets(it, i, offs);
    const Tc va = a_scalar ? sa : md_load<Tc>(a, adt, offs[0]);
    const Tc vb = b_scalar ? sb : md_load<Tc>(b, bdt, offs[1]);
    md_store_as(out, odt, offs[2], F::apply(va, vb));
  }
}
template <class Tc>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_where_generic(MdIter it, const void *c, int cdt, int c_scalar, uint8_t sc, const void *a, int adt,
                                                              int a_scalar, Tc sa, const void *b, int bdt, int b_scalar, Tc sb, void *out, int odt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < it.total; i += stride) {
    int64_t offs[MD_MAX_OPS];
    md_iter_offsets(it, i, offs);
    const uint8_t vc = c_scalar ? sc : md_load<uint8_t>(c, cdt, offs[0]);
    const Tc va = a_scalar ? sa : md_load<Tc>(a, adt, offs[1]);
    const Tc vb = b_scalar ? sb : md_load<Tc>(b, bdt, offs[2]);
    md_store_as(out, odt, offs[3], vc ? va : vb);
  }
}

// ------------------------------------------------------ conversion, 16-B vectors ----
// mdhip_convert (astype, every copy of a storage-only array) for dense and sliced operands from 2**14 elements on. The contract is
// k_convert's (elementwise.hip), bit for bit on every input pattern: source -> the carrier the SOURCE picks (int64: bool and the
// signed integers, uint64: the unsigned ones, double: the floats; md_load_any) -> destination (md_store_any). nw_cv states that
// chain per typed pair and lets the compiler fold what folds exactly (integer moves, int8 -> float32 ..); where it is not folded:
//  * float -> integer: the double goes through a 64-bit integer, then truncates — out-of-range values wrap from 64 bits. The double
//    passes an empty asm so that the fptosi stays the DOUBLE's (fptosi(fpext float) would be narrowed to the float's own expansion,
//    which differs out of range);
//  * float32 -> float32 the same way (cvt_f64_f32 + cvt_f32_f64 quiet a signalling NaN; the folded move would not);
//  * float64 / 32- and 64-bit integers -> float16: ONE rounding from the double, by md_double_to_half;
//  * float16 sources: the hardware conversion is exact; a NaN becomes the canonical one of md_half_to_double (sign kept);
//  * float32 / 8- and 16-bit integers -> float16: v_cvt_f16_f32 is the same single rounding (the float is exact in double);
//    a NaN becomes md_double_to_half's sign | 0x7E00.
// An integer destination is written in the unsigned type of its size (truncation does not see the sign).
template <class S> struct nw_cv_carrier { using type = int64_t; };
template <> struct nw_cv_carrier<uint8_t> { using type = uint64_t; };
template <> struct nw_cv_carrier<uint16_t> { using type = uint64_t; };
template <> struct nw_cv_carrier<uint32_t> { using type = uint64_t; };
template <> struct nw_cv_carrier<uint64_t> { using type = uint64_t; };
template <> struct nw_cv_carrier<f16> { using type = double; };
template <> struct nw_cv_carrier<float> { using type = double; };
template <> struct nw_cv_carrier<double> { using type = double; };

// elements per lane and trip: 16 B of the narrower side, at most 8 elements where one side is 8 bytes wide
template <class S, class D> struct nw_cv_e {
  static constexpr int lo = sizeof(S) < sizeof(D) ? sizeof(S) : sizeof(D), hi = sizeof(S) < sizeof(D) ? sizeof(D) : sizeof(S);
  static constexpr int value = (hi == 8 && 16 / lo > 8) ? 8 : 16 / lo;
};
// E elements of T: 16-B pieces, or one smaller vector
template <class T, int E> struct NwPack {
  static constexpr int P = sizeof(T) * E > 16 ? (int)sizeof(T) * E / 16 : 1, EP = E / P;
  typedef MdVec<T, EP> V;
  V p[P];
  __device__ __forceinline__ T &at(int j) { return p[j / EP].v[j % EP]; }
  __device__ __forceinline__ const T &at(int j) const { return p[j / EP].v[j % EP]; }
};
template <bool NT, class T, int E> __device__ __forceinline__ NwPack<T, E> nw_ldp(const T *p) {
  typedef typename NwPack<T, E>::V V;
  NwPack<T, E> r;
#pragma unroll
  for (int j = 0; j < NwPack<T, E>::P; ++j) r.p[j] = nw_ld<NT>(reinterpret_cast<const V *>(p) + j);
  return r;
}
template <bool NT, class T, int E> __device__ __forceinline__ void nw_stp(T *p, const NwPack<T, E> &v) {
  typedef typename NwPack<T, E>::V V;
#pragma unroll
  for (int j = 0; j < NwPack<T, E>::P; ++j) nw_st<NT>(reinterpret_cast<V *>(p) + j, v.p[j]);
}

__device__ __forceinline__ double nw_cv_keep(double d) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+v"(d));
#endif
  return d;
}
// float16 -> float32 with md_half_to_double's NaN
__device__ __forceinline__ float nw_cv_half(f16 h) {
  float f = md_f16_to_float(h);
  if ((h.bits & 0x7FFFu) > 0x7C00u) {
    const uint32_t b = ((uint32_t)(h.bits & 0x8000u) << 16) | 0x7FC00000u;
    __builtin_memcpy(&f, &b, 4);
  }
  return f;
}
// float32 (exact in double) -> float16 with md_double_to_half's NaN
__device__ __forceinline__ f16 nw_cv_to_half(float x) {
  f16 h = md_float_to_f16(x);
  if (x != x) {
    uint32_t b;
    __builtin_memcpy(&b, &x, 4);
    h.bits = (uint16_t)(((b >> 16) & 0x8000u) | 0x7E00u);
  }
  return h;
}
template <class S, class D> __device__ __forceinline__ D nw_cv(S x) {
  using C = typename nw_cv_carrier<S>::type;
  constexpr bool src_float = md_same<C, double>::value;
  constexpr bool dst_int = !md_same<D, b8>::value && !md_same<D, f16>::value && !md_is_float<D>::value;
  constexpr bool small_int = !src_float && sizeof(S) <= 2;   // bool, int8 / 16, uint8 / 16: exact in float32
  if constexpr (md_same<S, f16>::value && md_same<D, f16>::value) {
    if ((x.bits & 0x7FFFu) > 0x7C00u) x.bits = (uint16_t)((x.bits & 0x8000u) | 0x7E00u);
    return x;
  } else if constexpr (md_same<S, float>::value && md_same<D, f16>::value) {
    return nw_cv_to_half(x);
  } else if constexpr (small_int && md_same<D, f16>::value) {
    if constexpr (md_same<S, b8>::value) return md_float_to_f16((float)(x.v != 0));
    else return md_float_to_f16((float)x);
  } else {
    C c;
    if constexpr (md_same<S, b8>::value) c = (C)(x.v != 0);
    else if constexpr (md_same<S, f16>::value) c = (C)nw_cv_half(x);
    else c = (C)x;
    if constexpr (src_float && (dst_int || (md_same<S, float>::value && md_same<D, float>::value))) c = nw_cv_keep(c);
    if constexpr (md_same<D, b8>::value) {
      return b8{(uint8_t)(c != (C)0)};
    } else if constexpr (md_same<D, f16>::value) {
      f16 h;
      h.bits = md_double_to_half((double)c);
      return h;
    } else if constexpr (md_is_float<D>::value) {
      return (D)c;
    } else {
      int64_t i;
      if constexpr (src_float) i = md_carrier_to_i64(c);
      else i = (int64_t)c;
      return (D)i;
    }
  }
}

template <class S, class D, bool NT> __global__ void __launch_bounds__(MD_BLOCK) k_nw_convert(const S *x, D *out, int64_t n) {
  constexpr int E = nw_cv_e<S, D>::value;
  const int64_t nv = n / E, gs = (int64_t)gridDim.x * MD_BLOCK, gid = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  auto one = [&](const NwPack<S, E> &v, int64_t i) {
    NwPack<D, E> o;
#pragma unroll
    for (int j = 0; j < E; ++j) o.at(j) = nw_cv<S, D>(v.at(j));
    nw_stp<NT>(out + i * E, o);
  };
  int64_t i = gid;
  if constexpr (!NT) {   // (two in flight on the cached path, one on the non-temporal: as k_nw_binary)
    for (; i + gs < nv; i += 2 * gs) {
      const NwPack<S, E> v0 = nw_ldp<NT, S, E>(x + i * E), v1 = nw_ldp<NT, S, E>(x + (i + gs) * E);
      one(v0, i);
      one(v1, i + gs);
    }
  }
  for (; i < nv; i += gs) one(nw_ldp<NT, S, E>(x + i * E), i);
  const int64_t t = nv * E + gid;   // the up-to-(E-1) elements behind the last whole group
  if (t < n) out[t] = nw_cv<S, D>(x[t]);
}

// Two to four collapsed axes, both sides unit-stride along the inner one (astype / a dense copy of x16[:, :480], a copy into a
// slice): a lane owns one group of E elements; the outer position as in k_nw_binary_axes.
struct NwCvAxes {
  int64_t e0, e1, e2, nv, rows;
  int64_t st[2][3];
};
template <class S, class D> __global__ void __launch_bounds__(MD_BLOCK) k_nw_convert_axes(NwCvAxes g, const S *x, D *out) {
  constexpr int E = nw_cv_e<S, D>::value;
  const int64_t total = g.rows * g.nv, gs = (int64_t)gridDim.x * MD_BLOCK;
  for (int64_t v = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x; v < total; v += gs) {
    const int64_t row = v / g.nv, q = row / g.e2, r2 = row - q * g.e2;
    int64_t r0 = 0, r1 = q;
    if (g.e0 != 1) { r0 = q / g.e1; r1 = q - r0 * g.e1; }
    const int64_t c = (v - row * g.nv) * E;
    const NwPack<S, E> s = nw_ldp<false, S, E>(x + r0 * g.st[0][0] + r1 * g.st[0][1] + r2 * g.st[0][2] + c);
    NwPack<D, E> o;
#pragma unroll
    for (int j = 0; j < E; ++j) o.at(j) = nw_cv<S, D>(s.at(j));
    nw_stp<false>(out + r0 * g.st[1][0] + r1 * g.st[1][1] + r2 * g.st[1][2] + c, o);
  }
}

// ------------------------------------------------------------ where, 16-B vectors ----
// out = cond ? a : b under a dense bool condition, the branches arrays of the ONE storage-only type S (or a scalar, converted to S
// once on the host), out of type S: a selection of the STORED bits — nothing passes the carrier, NaN payloads and -0.0 come out
// as they went in (np.where moves values). E = 16 / sizeof(S) elements per lane, cond read as E bytes.
template <class S, int MA, int MB, bool NT>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_where(const uint8_t *__restrict__ c, const S *__restrict__ a, const S *__restrict__ b, S sa, S sb,
                                                      S *__restrict__ out, int64_t n) {
  constexpr int E = 16 / sizeof(S);
  typedef MdVec<S, E> V;
  typedef MdVec<uint8_t, E> Vc;
  const int64_t nv = n / E, gs = (int64_t)gridDim.x * MD_BLOCK, gid = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x;
  const Vc *pc = reinterpret_cast<const Vc *>(c);
  const V *pa = reinterpret_cast<const V *>(a), *pb = reinterpret_cast<const V *>(b);
  V *po = reinterpret_cast<V *>(out);
  auto one = [&](const Vc &vc, const V &va, const V &vb, int64_t i) {
    V o;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const S x = MA == NM_VEC ? va.v[j] : sa, y = MB == NM_VEC ? vb.v[j] : sb;
      o.v[j] = vc.v[j] ? x : y;
    }
    nw_st<NT>(po + i, o);
  };
  int64_t i = gid;
  if constexpr (!NT) {
    for (; i + gs < nv; i += 2 * gs) {
      const Vc c0 = nw_ld<NT>(pc + i), c1 = nw_ld<NT>(pc + i + gs);
      V a0, a1, b0, b1;
      if constexpr (MA == NM_VEC) { a0 = nw_ld<NT>(pa + i); a1 = nw_ld<NT>(pa + i + gs); }
      if constexpr (MB == NM_VEC) { b0 = nw_ld<NT>(pb + i); b1 = nw_ld<NT>(pb + i + gs); }
      one(c0, a0, b0, i);
      one(c1, a1, b1, i + gs);
    }
  }
  for (; i < nv; i += gs) {
    const Vc c0 = nw_ld<NT>(pc + i);
    V a0, b0;
    if constexpr (MA == NM_VEC) a0 = nw_ld<NT>(pa + i);
    if constexpr (MB == NM_VEC) b0 = nw_ld<NT>(pb + i);
    one(c0, a0, b0, i);
  }
  const int64_t t = nv * E + gid;
  if (t < n) {
    const S x = MA == NM_VEC ? a[t] : sa, y = MB == NM_VEC ? b[t] : sb;
    out[t] = c[t] ? x : y;
  }
}

// .. under a broadcast: two to four collapsed axes, cond and each branch contiguous or broadcast along the inner one (a (B, R, C)
// condition over a (B, 1, C) or (C,) branch, a sliced view); operand 0 is cond. The scheme of k_nw_binary_axes.
struct NwWhAxes {
  int64_t e0, e1, e2, nv, rows;
  int64_t st[3][3];
  int in[3];
};
template <class S>
__global__ void __launch_bounds__(MD_BLOCK) k_nw_where_axes(NwWhAxes g, const uint8_t *__restrict__ c, const S *__restrict__ a, const S *__restrict__ b, S sa,
                                                           S sb, S *__restrict__ out) {
  constexpr int E = 16 / sizeof(S);
  typedef MdVec<S, E> V;
  typedef MdVec<uint8_t, E> Vc;
  const int64_t total = g.rows * g.nv, gs = (int64_t)gridDim.x * MD_BLOCK;
  auto load = [&](const S *p, S s, int in, int64_t off, int64_t col, V &r) {
    if (p == nullptr) {
#pragma unroll
      for (int j = 0; j < E; ++j) r.v[j] = s;
    } else if (in) {
      r = *reinterpret_cast<const V *>(p + off + col);
    } else {
      const S t = p[off];
#pragma unroll
      for (int j = 0; j < E; ++j) r.v[j] = t;
    }
  };
  for (int64_t v = (int64_t)blockIdx.x * MD_BLOCK + threadIdx.x; v < total; v += gs) {
    const int64_t row = v / g.nv, q = row / g.e2, r2 = row - q * g.e2;
    int64_t r0 = 0, r1 = q;
    if (g.e0 != 1) { r0 = q / g.e1; r1 = q - r0 * g.e1; }
    const int64_t col = (v - row * g.nv) * E;
    const int64_t oc = r0 * g.st[0][0] + r1 * g.st[0][1] + r2 * g.st[0][2];
    Vc m;
    if (g.in[0]) {
      m = *reinterpret_cast<const Vc *>(c + oc + col);
    } else {
      const uint8_t t = c[oc];
#pragma unroll
      for (int j = 0; j < E; ++j) m.v[j] = t;
    }
    V x, y, o;
    load(a, sa, g.in[1], r0 * g.st[1][0] + r1 * g.st[1][1] + r2 * g.st[1][2], col, x);
    load(b, sb, g.in[2], r0 * g.st[2][0] + r1 * g.st[2][1] + r2 * g.st[2][2], col, y);
#pragma unroll
    for (int j = 0; j < E; ++j) o.v[j] = m.v[j] ? x.v[j] : y.v[j];
    *reinterpret_cast<V *>(out + row * (g.nv * E) + col) = o;
  }
}

// ---------------------------------------------------------------- eligibility ----
// the whole call as ONE contiguous run: every array operand dense over the collapsed 1-D space, 16-B aligned
static bool nw_contiguous(const MdIter &it, int nops, const mdhip_array *const *ops) {
  if (it.ndim != 1) return false;
  for (int k = 0; k < nops; ++k) {
    if (ops[k]->is_scalar) continue;
    if (it.strides[k][0] != 1) return false;
    if ((uintptr_t)ops[k]->data & 15) return false;
  }
  return true;
}
static bool nw_nt(int64_t bytes) {
  const int mode = (int)md_opt(MD_OPT_NT);
  if (mode >= 0) return mode != 0;
  return bytes > ((int64_t)320 << 20);
}
static int nw_grid(int64_t vectors, int per_cu) { return md_grid_for(vectors + 1, MD_BLOCK, MD_NUM_CUS * per_cu); }
// .. of the conversion and `where` streams: option max_blocks reaches it (tests meet a grid trip at a few thousand vectors)
static int nw_grid_opt(int64_t vectors, int per_cu) {
  const int n = (int)md_opt(MD_OPT_MAX_BLOCKS);
  return md_grid_for(vectors + 1, MD_BLOCK, n > 0 ? n : MD_NUM_CUS * per_cu);
}

// storage type of a loop dtype, as a type
template <int DT> struct nw_storage;
template <> struct nw_storage<MDHIP_I8> { using type = int8_t; };
template <> struct nw_storage<MDHIP_I16> { using type = int16_t; };
template <> struct nw_storage<MDHIP_U8> { using type = uint8_t; };
template <> struct nw_storage<MDHIP_U16> { using type = uint16_t; };
template <> struct nw_storage<MDHIP_U32> { using type = uint32_t; };
template <> struct nw_storage<MDHIP_U64> { using type = uint64_t; };
template <> struct nw_storage<MDHIP_F16> { using type = f16; };

struct HipExecN {
  // -------------------------------------------------------------------- unary ----
  template <class F, class Tc, int DT> static int unary_stream(const mdhip_array *x, const mdhip_array *out, int64_t n) {
    using S = typename nw_storage<DT>::type;
    using So = typename nw_out1<F, Tc, S>::type;
    const bool nt = nw_nt(n * (int64_t)(sizeof(S) + sizeof(So)));
    const int grid = nw_grid(n / (16 / (int64_t)sizeof(S)), 8);
    if (nt) MD_LAUNCH((k_nw_unary<F, Tc, S, true>), grid, MD_BLOCK, (const S *)x->data, (So *)out->data, n);
    else MD_LAUNCH((k_nw_unary<F, Tc, S, false>), grid, MD_BLOCK, (const S *)x->data, (So *)out->data, n);
    return MD_LAUNCH_CHECK("unary(narrow, stream)");
  }
  template <class F, class Tc> static int nunary(const MdIter &it, const mdhip_array *x, const mdhip_array *out) {
    using R = decltype(F::apply(Tc()));
    const mdhip_array *ops[2] = {x, out};
    // stream form: x and out of the same storage-only type (or out bool), dense
    if (!x->is_scalar && md_is_narrow(x->dtype) && nw_contiguous(it, 2, ops) && (md_same<R, b8>::value ? out->dtype == MDHIP_BOOL : out->dtype == x->dtype)) {
      switch (x->dtype) {
#define MD_NW_U(DT)                                                                                                          \
  case DT:                                                                                                                   \
    if constexpr (md_same<Tc, typename md_carrier_type<DT>::type>::value) return unary_stream<F, Tc, DT>(x, out, it.total);  \
    break;
        MD_NW_U(MDHIP_I8) MD_NW_U(MDHIP_I16) MD_NW_U(MDHIP_U8) MD_NW_U(MDHIP_U16) MD_NW_U(MDHIP_U32) MD_NW_U(MDHIP_U64) MD_NW_U(MDHIP_F16)
#undef MD_NW_U
      }
    }
    const Tc sx = x->is_scalar ? md_scalar_as<Tc>(x) : Tc();
    k_nw_unary_generic<F, Tc><<<md_grid_for(it.total), MD_BLOCK, 0, md_stream()>>>(it, x->data, x->dtype, x->is_scalar, sx, out->data, out->dtype);
    return MD_LAUNCH_CHECK("unary(narrow, generic)");
  }

  // ------------------------------------------------------------------- binary ----
  template <class F, class Tc, int DT, int MA, int MB>
  static int binary_stream(const mdhip_array *a, const mdhip_array *b, Tc sa, Tc sb, const mdhip_array *out, int64_t n) {
    using S = typename nw_storage<DT>::type;
    using So = typename nw_out<F, Tc, S>::type;
    const int64_t bytes = n * (int64_t)(sizeof(So) + (MA == NM_VEC ? sizeof(S) : 0) + (MB == NM_VEC ? sizeof(S) : 0));
    const bool nt = nw_nt(bytes);
    const int grid = nw_grid(n / (16 / (int64_t)sizeof(S)), MA == NM_VEC && MB == NM_VEC ? 4 : 8);   // (as the wide kernels: three streams want fewer resident waves)
    if (nt) MD_LAUNCH((k_nw_binary<F, Tc, S, MA, MB, true>), grid, MD_BLOCK, (const S *)a->data, (const S *)b->data, sa, sb, (So *)out->data, n);
    else MD_LAUNCH((k_nw_binary<F, Tc, S, MA, MB, false>), grid, MD_BLOCK, (const S *)a->data, (const S *)b->data, sa, sb, (So *)out->data, n);
    return MD_LAUNCH_CHECK("binary(narrow, stream)");
  }
  template <class F, class Tc, int DT>
  static int binary_stream_modes(const mdhip_array *a, const mdhip_array *b, Tc sa, Tc sb, const mdhip_array *out, int64_t n) {
    if (!a->is_scalar && !b->is_scalar) return binary_stream<F, Tc, DT, NM_VEC, NM_VEC>(a, b, sa, sb, out, n);
    if (!a->is_scalar) return binary_stream<F, Tc, DT, NM_VEC, NM_SCAL>(a, b, sa, sb, out, n);
    return binary_stream<F, Tc, DT, NM_SCAL, NM_VEC>(a, b, sa, sb, out, n);
  }
  // -1: the iteration space does not fit k_nw_binary_axes (the caller goes on to the generic kernel)
  template <class F, class Tc, int DT>
  static int binary_axes(const MdIter &it, const mdhip_array *a, const mdhip_array *b, Tc sa, Tc sb, const mdhip_array *out) {
    using S = typename nw_storage<DT>::type;
    using So = typename nw_out<F, Tc, S>::type;
    constexpr int E = 16 / sizeof(S);
    const int nd = it.ndim, sh = 4 - nd;
    const int64_t inner = it.shape[nd - 1];
    if ((inner % E) || it.strides[2][nd - 1] != 1 || ((uintptr_t)out->data % (sizeof(So) * E)) != 0) return -1;
    int64_t dense = inner;
    for (int d = nd - 2; d >= 0; --d) {
      if (it.strides[2][d] != dense) return -1;
      dense *= it.shape[d];
    }
    NwAxes g{};
    g.e0 = nd == 4 ? it.shape[0] : 1;
    g.e1 = nd >= 3 ? it.shape[nd - 3] : 1;
    g.e2 = it.shape[nd - 2];
    g.nv = inner / E;
    g.rows = g.e0 * g.e1 * g.e2;
    const mdhip_array *ops[2] = {a, b};
    for (int k = 0; k < 2; ++k) {
      if (ops[k]->is_scalar) continue;
      const int64_t is = it.strides[k][nd - 1];
      if (is != 0 && is != 1) return -1;
      g.in[k] = (int)is;
      for (int j = sh; j < 3; ++j) {
        const int64_t st = it.strides[k][j - sh];
        if (is == 1 && (st % E)) return -1;
        g.st[k][j] = st;
      }
      if (is == 1 && ((uintptr_t)ops[k]->data & 15)) return -1;
    }
    MD_LAUNCH((k_nw_binary_axes<F, Tc, S>), md_grid_for(g.rows * g.nv), MD_BLOCK, g, a->is_scalar ? nullptr : (const S *)a->data,
              b->is_scalar ? nullptr : (const S *)b->data, sa, sb, (So *)out->data);
    return MD_LAUNCH_CHECK("binary(narrow, axes)");
  }
  template <class F, class Tc> static int nbinary(const MdIter &it, const mdhip_array *a, const mdhip_array *b, const mdhip_array *out) {
    using R = decltype(F::apply(Tc(), Tc()));
    const Tc sa = a->is_scalar ? md_scalar_as<Tc>(a) : Tc(), sb = b->is_scalar ? md_scalar_as<Tc>(b) : Tc();
    const mdhip_array *ops[3] = {a, b, out};
    // stream form: the array operand(s) of ONE storage-only type, out of that type (arithmetic) or bool (comparisons), all dense
    const int sdt = !a->is_scalar ? a->dtype : b->dtype;
    const bool same = (a->is_scalar || a->dtype == sdt) && (b->is_scalar || b->dtype == sdt) && !(a->is_scalar && b->is_scalar);
    if (same && md_is_narrow(sdt) && nw_contiguous(it, 3, ops) && (md_same<R, b8>::value ? out->dtype == MDHIP_BOOL : out->dtype == sdt)) {
      switch (sdt) {
#define MD_NW_B(DT)                                                                                                                   \
  case DT:                                                                                                                            \
    if constexpr (md_same<Tc, typename md_carrier_type<DT>::type>::value) return binary_stream_modes<F, Tc, DT>(a, b, sa, sb, out, it.total); \
    break;
        MD_NW_B(MDHIP_I8) MD_NW_B(MDHIP_I16) MD_NW_B(MDHIP_U8) MD_NW_B(MDHIP_U16) MD_NW_B(MDHIP_U32) MD_NW_B(MDHIP_U64) MD_NW_B(MDHIP_F16)
#undef MD_NW_B
      }
    }
    if (same && md_is_narrow(sdt) && (md_same<R, b8>::value ? out->dtype == MDHIP_BOOL : out->dtype == sdt) && it.ndim >= 2 && it.ndim <= 4 &&
        it.total >= (1 << 14)) {
      switch (sdt) {
#define MD_NW_BA(DT)                                                                                                                  \
  case DT:                                                                                                                            \
    if constexpr (md_same<Tc, typename md_carrier_type<DT>::type>::value) {                                                           \
      int rc = binary_axes<F, Tc, DT>(it, a, b, sa, sb, out);                                                                         \
      if (rc != -1) return rc;                                                                                                        \
    }                                                                                                                                 \
    break;
        MD_NW_BA(MDHIP_I8) MD_NW_BA(MDHIP_I16) MD_NW_BA(MDHIP_U8) MD_NW_BA(MDHIP_U16) MD_NW_BA(MDHIP_U32) MD_NW_BA(MDHIP_U64) MD_NW_BA(MDHIP_F16)
#undef MD_NW_BA
      }
    }
    k_nw_binary_generic<F, Tc><<<md_grid_for(it.total), MD_BLOCK, 0, md_stream()>>>(it, a->data, a->dtype, a->is_scalar, sa, b->data, b->dtype,
                                                                                  b->is_scalar, sb, out->data, out->dtype);
    return MD_LAUNCH_CHECK("binary(narrow, generic)");
  }

  // -------------------------------------------------------------------- where ----
  // a scalar branch in the storage type, converted once: what md_store_as makes of the carrier value
  template <class S, class Tc> static S where_scalar(Tc v) {
    if constexpr (md_same<S, f16>::value) return md_cast<f16>(v);
    else return (S)md_cast<int64_t>(v);
  }
  template <class S, int MA, int MB>
  static int where_stream(const mdhip_array *c, const mdhip_array *a, const mdhip_array *b, S sa, S sb, const mdhip_array *out, int64_t n) {
    const int64_t bytes = n * (int64_t)(1 + sizeof(S) * (1 + (MA == NM_VEC) + (MB == NM_VEC)));
    const bool nt = nw_nt(bytes);
    const int grid = nw_grid_opt(n / (16 / (int64_t)sizeof(S)), MA == NM_VEC && MB == NM_VEC ? 4 : 8);   // (four streams: fewer resident waves, as binary_stream)
    md_opt_table()[MD_OPT_WHERE_VEC_RUNS] += 1;
    if (nt) MD_LAUNCH((k_nw_where<S, MA, MB, true>), grid, MD_BLOCK, (const uint8_t *)c->data, (const S *)a->data, (const S *)b->data, sa, sb, (S *)out->data, n);
    else MD_LAUNCH((k_nw_where<S, MA, MB, false>), grid, MD_BLOCK, (const uint8_t *)c->data, (const S *)a->data, (const S *)b->data, sa, sb, (S *)out->data, n);
    return MD_LAUNCH_CHECK("where(narrow, stream)");
  }
  // -1: not a call of the vector forms (the caller goes on to the generic kernel)
  template <class S, class Tc>
  static int where_vec(const MdIter &it, const mdhip_array *c, const mdhip_array *a, const mdhip_array *b, Tc ca, Tc cb, const mdhip_array *out) {
    constexpr int E = 16 / sizeof(S);
    const S sa = a->is_scalar ? where_scalar<S>(ca) : S(), sb = b->is_scalar ? where_scalar<S>(cb) : S();
    const mdhip_array *br[2] = {a, b};
    const int nd = it.ndim;
    if (nd == 1) {
      if (it.strides[0][0] != 1 || it.strides[3][0] != 1 || ((uintptr_t)c->data % E) || ((uintptr_t)out->data & 15)) return -1;
      for (int k = 0; k < 2; ++k)
        if (!br[k]->is_scalar && (it.strides[1 + k][0] != 1 || ((uintptr_t)br[k]->data & 15))) return -1;
      if (!a->is_scalar && !b->is_scalar) return where_stream<S, NM_VEC, NM_VEC>(c, a, b, sa, sb, out, it.total);
      if (!a->is_scalar) return where_stream<S, NM_VEC, NM_SCAL>(c, a, b, sa, sb, out, it.total);
      return where_stream<S, NM_SCAL, NM_VEC>(c, a, b, sa, sb, out, it.total);
    }
    if (nd > 4) return -1;
    const int sh = 4 - nd;
    const int64_t inner = it.shape[nd - 1];
    if ((inner % E) || it.strides[3][nd - 1] != 1 || ((uintptr_t)out->data & 15)) return -1;
    int64_t dense = inner;
    for (int d = nd - 2; d >= 0; --d) {
      if (it.strides[3][d] != dense) return -1;
      dense *= it.shape[d];
    }
    NwWhAxes g{};
    g.e0 = nd == 4 ? it.shape[0] : 1;
    g.e1 = nd >= 3 ? it.shape[nd - 3] : 1;
    g.e2 = it.shape[nd - 2];
    g.nv = inner / E;
    g.rows = g.e0 * g.e1 * g.e2;
    const mdhip_array *ops[3] = {c, a, b};
    for (int k = 0; k < 3; ++k) {
      if (ops[k]->is_scalar) continue;
      const int64_t is = it.strides[k][nd - 1];
      if (is != 0 && is != 1) return -1;
      g.in[k] = (int)is;
      for (int j = sh; j < 3; ++j) {
        const int64_t st = it.strides[k][j - sh];
        if (is == 1 && (st % E)) return -1;
        g.st[k][j] = st;
      }
      // (a unit-stride operand is read E elements at a time: cond on E bytes, a branch on 16)
      if (is == 1 && ((uintptr_t)ops[k]->data % (k == 0 ? E : 16))) return -1;
    }
    md_opt_table()[MD_OPT_WHERE_VEC_RUNS] += 1;
    MD_LAUNCH((k_nw_where_axes<S>), md_grid_for(g.rows * g.nv), MD_BLOCK, g, (const uint8_t *)c->data, a->is_scalar ? nullptr : (const S *)a->data,
              b->is_scalar ? nullptr : (const S *)b->data, sa, sb, (S *)out->data);
    return MD_LAUNCH_CHECK("where(narrow, axes)");
  }
  template <class Tc> static int nwhere(const MdIter &it, const mdhip_array *c, const mdhip_array *a, const mdhip_array *b, const mdhip_array *out) {
    const uint8_t sc = c->is_scalar ? md_scalar_as<uint8_t>(c) : 0;
    const Tc sa = a->is_scalar ? md_scalar_as<Tc>(a) : Tc(), sb = b->is_scalar ? md_scalar_as<Tc>(b) : Tc();
    // vector forms: a bool array condition, the branches arrays of out's storage-only type or scalars (not both), 2**14 elements and
    // more, one to four collapsed axes. A non-bool condition, branches of two dtypes, a wide out: the generic kernel.
    const int odt = out->dtype;
    if (md_opt(MD_OPT_WHERE_VEC) && md_is_narrow(odt) && !c->is_scalar && c->dtype == MDHIP_BOOL && (a->is_scalar || a->dtype == odt) &&
        (b->is_scalar || b->dtype == odt) && !(a->is_scalar && b->is_scalar) && it.ndim >= 1 && it.total >= (1 << 14)) {
      switch (odt) {
#define MD_NW_W(DT)                                                                                       \
  case DT:                                                                                                \
    if constexpr (md_same<Tc, typename md_carrier_type<DT>::type>::value) {                               \
      int rc = where_vec<typename nw_storage<DT>::type, Tc>(it, c, a, b, sa, sb, out);                    \
      if (rc != -1) return rc;                                                                            \
    }                                                                                                     \
    break;
        MD_NW_W(MDHIP_I8) MD_NW_W(MDHIP_I16) MD_NW_W(MDHIP_U8) MD_NW_W(MDHIP_U16) MD_NW_W(MDHIP_U32) MD_NW_W(MDHIP_U64) MD_NW_W(MDHIP_F16)
#undef MD_NW_W
      }
    }
    k_nw_where_generic<Tc><<<md_grid_for(it.total), MD_BLOCK, 0, md_stream()>>>(it, c->data, c->dtype, c->is_scalar, sc, a->data, a->dtype, a->is_scalar, sa,
                                                                                b->data, b->dtype, b->is_scalar, sb, out->data, out->dtype);
    return MD_LAUNCH_CHECK("where(narrow, generic)");
  }
};

// --------------------------------------------------------------- conversion ----
// -1: declined (mdhip_convert goes on to k_convert). it: operand 0 = x, operand 1 = out.
template <class S, class D> static int nw_convert_pair(const MdIter &it, const mdhip_array *x, const mdhip_array *out) {
  constexpr int E = nw_cv_e<S, D>::value;
  constexpr int64_t AX = sizeof(S) * E > 16 ? 16 : sizeof(S) * E, AO = sizeof(D) * E > 16 ? 16 : sizeof(D) * E;   // each side's own vector
  const int nd = it.ndim;
  if (nd < 1 || nd > 4 || it.strides[0][nd - 1] != 1 || it.strides[1][nd - 1] != 1) return -1;
  if (((uintptr_t)x->data % AX) || ((uintptr_t)out->data % AO)) return -1;
  if (nd == 1) {
    const int64_t n = it.total;
    const bool nt = nw_nt(n * (int64_t)(sizeof(S) + sizeof(D)));
    const int grid = nw_grid_opt(n / E, 8);
    md_opt_table()[MD_OPT_CONVERT_VEC_RUNS] += 1;
    if (nt) MD_LAUNCH((k_nw_convert<S, D, true>), grid, MD_BLOCK, (const S *)x->data, (D *)out->data, n);
    else MD_LAUNCH((k_nw_convert<S, D, false>), grid, MD_BLOCK, (const S *)x->data, (D *)out->data, n);
    return MD_LAUNCH_CHECK("convert(stream)");
  }
  const int sh = 4 - nd;
  const int64_t inner = it.shape[nd - 1];
  if (inner % E) return -1;
  NwCvAxes g{};
  g.e0 = nd == 4 ? it.shape[0] : 1;
  g.e1 = nd >= 3 ? it.shape[nd - 3] : 1;
  g.e2 = it.shape[nd - 2];
  g.nv = inner / E;
  g.rows = g.e0 * g.e1 * g.e2;
  for (int k = 0; k < 2; ++k)
    for (int j = sh; j < 3; ++j) {
      const int64_t st = it.strides[k][j - sh];
      if ((st * (int64_t)(k == 0 ? sizeof(S) : sizeof(D))) % (k == 0 ? AX : AO)) return -1;
      g.st[k][j] = st;
    }
  md_opt_table()[MD_OPT_CONVERT_VEC_RUNS] += 1;
  MD_LAUNCH((k_nw_convert_axes<S, D>), md_grid_for(g.rows * g.nv), MD_BLOCK, g, (const S *)x->data, (D *)out->data);
  return MD_LAUNCH_CHECK("convert(axes)");
}
template <class S> static int nw_convert_from(const MdIter &it, const mdhip_array *x, const mdhip_array *out) {
  switch (out->dtype) {
    case MDHIP_BOOL: return nw_convert_pair<S, b8>(it, x, out);
    case MDHIP_I8: case MDHIP_U8: return nw_convert_pair<S, uint8_t>(it, x, out);
    case MDHIP_I16: case MDHIP_U16: return nw_convert_pair<S, uint16_t>(it, x, out);
    case MDHIP_I32: case MDHIP_U32: return nw_convert_pair<S, uint32_t>(it, x, out);
    case MDHIP_I64: case MDHIP_U64: return nw_convert_pair<S, uint64_t>(it, x, out);
    case MDHIP_F16: return nw_convert_pair<S, f16>(it, x, out);
    case MDHIP_F32: return nw_convert_pair<S, float>(it, x, out);
    case MDHIP_F64: return nw_convert_pair<S, double>(it, x, out);
  }
  return -1;
}

}  // namespace

// mdhip_convert asks here first: the vector kernels from 2**14 elements on (below, a call is launch latency), -1 = declined
int md_narrow_convert(const MdIter &it, const mdhip_array *x, const mdhip_array *out) {
  if (!md_opt(MD_OPT_CONVERT_VEC) || it.total < (1 << 14)) return -1;
  switch (x->dtype) {
    case MDHIP_BOOL: return nw_convert_from<b8>(it, x, out);
    case MDHIP_I8: return nw_convert_from<int8_t>(it, x, out);
    case MDHIP_I16: return nw_convert_from<int16_t>(it, x, out);
    case MDHIP_I32: return nw_convert_from<int32_t>(it, x, out);
    case MDHIP_I64: return nw_convert_from<int64_t>(it, x, out);
    case MDHIP_U8: return nw_convert_from<uint8_t>(it, x, out);
    case MDHIP_U16: return nw_convert_from<uint16_t>(it, x, out);
    case MDHIP_U32: return nw_convert_from<uint32_t>(it, x, out);
    case MDHIP_U64: return nw_convert_from<uint64_t>(it, x, out);
    case MDHIP_F16: return nw_convert_from<f16>(it, x, out);
    case MDHIP_F32: return nw_convert_from<float>(it, x, out);
    case MDHIP_F64: return nw_convert_from<double>(it, x, out);
  }
  return -1;
}

// entry points of elementwise.hip hand over here when a storage-only dtype takes part
int md_narrow_unary(int op, const mdhip_array *x, const mdhip_array *out) { return md_narrow_unary_dispatch<HipExecN>(op, x, out); }
int md_narrow_binary(int op, const mdhip_array *a, const mdhip_array *b, const mdhip_array *out, int cdt) {
  return md_narrow_binary_dispatch<HipExecN>(op, a, b, out, cdt);
}
int md_narrow_where(const mdhip_array *c, const mdhip_array *a, const mdhip_array *b, const mdhip_array *out) {
  return md_narrow_where_dispatch<HipExecN>(c, a, b, out);
}
