// md_hip.h — device-side helpers shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdlib.h>

#include "md_dispatch.h"

#include "md_ticket.h"

hipStream_t md_stream();
struct MdGemm;
// skinny.hip: thin products (matrix x vector ..) / both sides thin, k long (a dot product ..); -1 = not applicable. dtype: the
// operands'; wide_out: float16 / int8 operands with a float32 / int32 c
int md_gemm_skinny(const MdGemm &g, int dtype, bool wide_out = false);
int md_gemm_longk(const MdGemm &g, int dtype, bool wide_out = false);
// gemm_narrow.hip: float16 / int8 / uint8 products planned by gemm.hip (plan_narrow). mfma: a_kc / b_kc = the operand's k axis is
// unit-stride (else its row axis is), edge = ragged tiles (zero: 16-B aligned zeros for the lanes outside the operands)
int md_gemm_narrow_mfma(const MdGemm &g, int dtype, bool a_kc, bool b_kc, bool edge, const void *zero);
int md_gemm_narrow_generic(const MdGemm &g, int dtype);
// the same with the accumulators stored as they are: float16 operands -> float32 c, int8 -> int32 (`dtype`: the operands')
int md_gemm_widen_mfma(const MdGemm &g, int dtype, bool a_kc, bool b_kc, bool edge, const void *zero);
int md_gemm_widen_generic(const MdGemm &g, int dtype);
// gemm_bf16x3.hip: float32 products on the bf16 matrix cores, planned by gemm.hip (plan_bf16x3). split: a rows x K operand (k_contig:
// `stride` floats between rows, else between k-rows) -> three rows x K bfloat16 planes at `planes`, ORs 1 into *flag on an inf / NaN;
// the product: C (M x N, c_ms floats between rows) from the planes, nothing when *flag != 0. layout: the plane image, the same for
// the split passes and the product of one plan (md_bf16x3_layout.h: 0 [rows][K] | 1 k-tile-major); band: option gemm_bf16x3_band.
// products: 6 (nplanes 3, the exact split) or the reduced forms 3 (nplanes 2) / 1 (nplanes 1) over rounded planes (option
// gemm_products), which also raise the flag for a finite element that rounds to inf. stamp: null, or (option gemm_stamp, six
// products only) 16 bytes per block for the diagnostic instantiation's clock stamps
int md_gemm_bf16x3_split(const float *src, bool k_contig, int64_t rows, int64_t K, int64_t stride, void *planes, unsigned *flag, int layout, int nplanes);
int md_gemm_bf16x3(const void *a_planes, const void *b_planes, float *c, int64_t M, int64_t N, int64_t K, int64_t c_ms, const unsigned *flag, int loop,
                   int layout, int band, int products, unsigned long long *stamp);
unsigned *md_tickets();                                   // MD_TICKET_WORDS zeroed counters (md_ticket.h)
bool md_capturing();                                      // a stream capture is recording (mdhip_graph_begin .. _end)
int *md_sticky();                                         // host-mapped word a CAPTURED gather / scatter sets on an out-of-bounds index
int md_sticky_check();                                    // after a synchronisation: MDHIP_EINDEX (and clear) if a replay set it
bool md_prof_take(hipEvent_t *start, hipEvent_t *stop);   // bench timing: events for the next main kernel (MD_LAUNCH, the GEMM launchers), if any were attached
int md_hip_check(hipError_t e, const char *what);

#define MD_LAUNCH_CHECK(name) md_hip_check(hipGetLastError(), name)

// Launch on the library's stream. With events attached (mdhip_event_attach_next: bench.py) the dispatch ITSELF carries the
// start / stop timestamps — the kernel's own duration, no marker packets around it (a marker pair costs ~4 us of stream
// time and reads 5-15 % low on a 25-us streaming kernel). Kernel names with template commas go in parentheses.
#define MD_LAUNCH(kernel, grid, block, ...)                                                                            \
  do {                                                                                                                 \
    hipEvent_t md_e0_, md_e1_;                                                                                         \
    if (md_prof_take(&md_e0_, &md_e1_)) hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, md_stream(), md_e0_, md_e1_, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, md_stream(), __VA_ARGS__);                             \
  } while (0)

// MI355X: 256 CUs. Streaming kernels cap the grid and stride (guide §6 G11).
constexpr int MD_NUM_CUS = 256;
constexpr int MD_BLOCK = 256;
static inline int md_max_blocks() {
  const int n = (int)md_opt(MD_OPT_MAX_BLOCKS);  // experiment knob (md_options.h)
  return n > 0 ? n : MD_NUM_CUS * 8;
}
static inline int md_grid_for(int64_t work_items, int per_block = MD_BLOCK, int max_blocks = 0) {
  if (max_blocks <= 0) max_blocks = md_max_blocks();
  int64_t b = (work_items + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > max_blocks) b = max_blocks;
  return (int)b;
}

template <class T, int N> struct alignas(sizeof(T) * N > 16 ? 16 : sizeof(T) * N) MdVec {
  T v[N];
};

// ---- wave / block reductions (wave = 64 lanes) ----------------------------------
template <class T> __device__ __forceinline__ T md_shfl_down(T v, int delta) {
  if constexpr (sizeof(T) == 8) {
    union { T t; int32_t w[2]; } u;
    u.t = v;
    u.w[0] = __shfl_down(u.w[0], delta, 64);
    u.w[1] = __shfl_down(u.w[1], delta, 64);
    return u.t;
  } else if constexpr (sizeof(T) == 4) {
    union { T t; int32_t w; } u;
    u.t = v;
    u.w = __shfl_down(u.w, delta, 64);
    return u.t;
  } else {
    int32_t w = (int32_t)v;
    w = __shfl_down(w, delta, 64);
    return (T)w;
  }
}
