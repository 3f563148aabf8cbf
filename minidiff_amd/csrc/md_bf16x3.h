// md_bf16x3.h — the exact three-way split of a float32 into bfloat16 planes, and (at the end) the rounding split into one or two
// planes of the reduced products (gemm_bf16x3.hip; host-testable).
//
// A plane is a float32 bit pattern whose low 16 bits are clear: its high half IS the bfloat16.
//   p1 = bits(x) & 0xFFFF0000        the top 8 significand bits of x (truncated: never overflows)
//   r  = x - p1                      exact (at most 16 significant bits are left)
//   p2 = bits(r) & 0xFFFF0000
//   p3 = bits(r - p2) & 0xFFFF0000   r - p2 is exact and has at most 8 significant bits
// (p1 + p2) + p3 == x exactly while every plane is a normal number, i.e. for |x| >= 2^-102. Below that a tail may be subnormal, and a
// subnormal's bits under 2^-133 (bfloat16's smallest step) go with the last mask: the planes then sum to x within 2^-133.
// A non-finite x gives (x, 0, 0) — a NaN keeps a set quiet bit, so that the plane is a NaN too — and `true`: products with such an
// operand are not formed on the planes (inf x a zero tail would give NaN where the fma chain gives inf).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_BF16X3_HD __host__ __device__
#else
#define MD_BF16X3_HD
#endif

MD_BF16X3_HD inline uint32_t md_bf16x3_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
MD_BF16X3_HD inline float md_bf16x3_float(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// planes as float32 bit patterns (low halves clear); true: x is inf or NaN
MD_BF16X3_HD inline bool md_bf16x3_split(float x, uint32_t *p1, uint32_t *p2, uint32_t *p3) {
  const uint32_t u = md_bf16x3_bits(x);
  if ((u & 0x7F800000u) == 0x7F800000u) {
    *p1 = (u & 0xFFFF0000u) | ((u & 0x007FFFFFu) ? 0x00400000u : 0u);
    *p2 = *p3 = 0;
    return true;
  }
  const uint32_t a = u & 0xFFFF0000u;
  const float r = x - md_bf16x3_float(a);
  const uint32_t b = md_bf16x3_bits(r) & 0xFFFF0000u;
  const float r2 = r - md_bf16x3_float(b);
  *p1 = a;
  *p2 = b;
  *p3 = md_bf16x3_bits(r2) & 0xFFFF0000u;
  return false;
}

// The ROUNDING split of the reduced products (option gemm_products 3 / 1: gemm_bf16x3.hip's k_gemm_bf16xp), nplanes 1 or 2:
//   p1 = RN_even_bf16(x)             on the bit pattern: + 0x7FFF + the kept half's last bit, low half cleared (subnormals included)
//   p2 = RN_even_bf16(x - p1)        x - p1 is exact in float32 (at most 16 significant bits, |x - p1| <= half a step of p1)
// Rounded, not truncated as above: a truncated plane is never larger in magnitude than x, so a product of truncated planes leans
// towards zero by up to 2^-8 (one plane) / 2^-16 (two) of every term; a rounded plane errs to either side. |x - p1| <= 2^-9 |x| and
// |x - p1 - p2| <= 2^-18 |x| while p2 is a normal number. true, and the product is not formed on the planes: inf and NaN (planes as
// above), and a finite x that rounds up to inf (|x| >= 0x7F7F8000: p1 = the inf, p2 = 0).
MD_BF16X3_HD inline uint32_t md_bf16x3_rn(uint32_t u) { return (u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u; }
MD_BF16X3_HD inline bool md_bf16x3_split_rn(float x, int nplanes, uint32_t *p1, uint32_t *p2) {
  const uint32_t u = md_bf16x3_bits(x);
  *p2 = 0;
  if ((u & 0x7F800000u) == 0x7F800000u) {
    *p1 = (u & 0xFFFF0000u) | ((u & 0x007FFFFFu) ? 0x00400000u : 0u);
    return true;
  }
  const uint32_t a = md_bf16x3_rn(u);
  *p1 = a;
  if ((a & 0x7F800000u) == 0x7F800000u) return true;
  if (nplanes > 1) *p2 = md_bf16x3_rn(md_bf16x3_bits(x - md_bf16x3_float(a)));
  return false;
}
