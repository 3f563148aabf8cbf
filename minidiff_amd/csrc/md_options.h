// md_options.h — the ONE table of tuning / experiment switches of libmdhip (and of the CPU test double).
//
// Rules (VERDICT r3 "close the experiment back door"):
//   * no getenv on a launch path: kernels and launchers read md_opt(ID), a plain array load;
//   * the environment is consulted ONCE per process, the first time the table is touched (mdhip_init does it):
//       - CONFIG entries (kind 'c': deployment settings — pinned-memory cap, run-time compilation on/off) are always read;
//       - EXPERIMENT entries (kind 'x': tile forcing, A/B switches, legacy two-launch paths) are read only when
//         MDHIP_EXPERIMENTS=1 is set; without it a stray MDHIP_GEMM_* / MDHIP_*_TICKET / MDHIP_COLS_* / MDHIP_ARG_* /
//         MDHIP_SWEEP_* variable in the environment of a lease changes NOTHING;
//   * tests and A/B scripts force a path through the C-ABI test hook mdhip_debug_set_option(name, value)
//     (include/mdhip.h), which takes effect on the next launch — no process restart, no environment.
// The environment variable of an entry is "MDHIP_" + its upper-cased name.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// X(ID, "name", default, kind)
#define MD_OPTION_LIST(X)                                                                                                        \
  /* deployment configuration (always read) */                                                                                  \
  X(PINNED_CAP, "pinned_cap", (int64_t)4 << 30, 'c')   /* bytes of page-locked host memory outstanding at most */               \
  X(JIT, "jit", 1, 'c')                                /* 0: never compile fused kernels at run time (interpreter only) */      \
  X(JIT_VERBOSE, "jit_verbose", 0, 'c')                /* print hiprtc logs of failed compilations; 2: resource remarks in every log */                        \
  X(INDEX_DEFER, "index_defer", 0, 'c')                /* 1: gathers / scatters never read their bounds verdict back (see index.hip) */ \
  /* experiments (MDHIP_EXPERIMENTS=1, or mdhip_debug_set_option) */                                                            \
  X(JIT_MIN, "jit_min", 1 << 18, 'x')                  /* elements from which a fused program is specialised */                 \
  X(COMM_PRIORITY, "comm_priority", 0, 'x')            /* 1: the collective stream gets the high-priority queue */             \
  X(MAX_BLOCKS, "max_blocks", 0, 'x')                  /* grid cap of the streaming kernels (0: 8 per CU) */                    \
  X(NT, "nt", -1, 'x')                                 /* elementwise non-temporal path: -1 by size | 0 never | 1 always */     \
  X(GEMM_CFG, "gemm_cfg", -1, 'x')                     /* force a tile of gemm.hip's CFG_* enum (-1: cost model) */             \
  X(GEMM_GLDS, "gemm_glds", 1, 'x')                    /* 0: register-staged GEMM kernels only */                               \
  X(GEMM_NBUF, "gemm_nbuf", 0, 'x')                    /* LDS buffers of the 128-row direct-to-LDS tiles: 0 by grid | 2 | 3 */ \
  X(GEMM_PEEL, "gemm_peel", 1, 'x')                    /* ragged products: 0 never peeled | 1 by the model | 2 always */        \
  X(GEMM_TT_SWAP, "gemm_tt_swap", 1, 'x')              /* 0: TT products stay on the register-staged kernel */                  \
  X(GEMM_REPACK, "gemm_repack", 1, 'x')                /* 0: misaligned operands are not copied into aligned buffers */         \
  X(GEMM_SUPER, "gemm_super", 8, 'x')                  /* tile rows per band of the XCD-compact numbering */                    \
  X(GEMM_SPLITK, "gemm_splitk", 1, 'x')                                                                                         \
  X(GEMM_STAMP, "gemm_stamp", 0, 'x')                  /* in-kernel clock stamps (diagnostic) */                                \
  X(GEMM_F64_MFMA, "gemm_f64_mfma", 1, 'x')                                                                                     \
  X(GEMM_SKINNY, "gemm_skinny", 1, 'x')                /* 0: thin products stay on the MFMA / generic kernels */                \
  X(GEMM_WIDEN, "gemm_widen", 1, 'x')                  /* 0: float16 -> float32 / int8 -> int32 products convert their operands first (A/B) */ \
  X(GEMM_NARROW_SKINNY, "gemm_narrow_skinny", 1, 'x')  /* 0: thin and long-k float16 / int8 / uint8 products keep the conversion / generic routes they had (A/B) */ \
  X(GEMM_NARROW_THIN_RUNS, "gemm_narrow_thin_runs", 0, 'x') /* a COUNTER, as gemm_bf16x3_runs: the host adds 1 for every launch it ISSUES of a streaming / long-k kernel on float16 / int8 / uint8 operands (a long-k product is two launches) */ \
  X(GEMM_BF16X3, "gemm_bf16x3", 1, 'x')                /* large float32 products as six bf16 products of pre-split planes: 0 never | 1 above the size floors | 2 every shape the kernels take and whose fp32 plan is plain launches (tests) */ \
  X(GEMM_BF16X3_RUNS, "gemm_bf16x3_runs", 0, 'x')      /* a COUNTER kept in this table so that tests can read it (and, like any entry, write it): the host adds 1 when it ISSUES the bf16x3 product kernel — a graph replay does not count */ \
  X(GEMM_BF16X3_LOOP, "gemm_bf16x3_loop", 3, 'x')      /* k loop of the bf16x3 product kernel: 0 staging in front of the reads, fold behind the MFMAs | 1 staging and fold under the MFMAs | 2 the two waves of a SIMD one segment apart, one in MFMAs while the other reads, stages and folds | 3 (default) loop 2 on the 16x16x32 MFMA, the wave tile as two halves (loops 0 - 2 agree bit for bit; loop 3 has bits of its own: six truncating accumulations of 32 terms per k-tile, not twelve of 16; A/B) */ \
  X(GEMM_BF16X3_BAND, "gemm_bf16x3_band", 0, 'x')      /* tile walk of the bf16x3 product kernel, tile rows per band of an XCD's tiles: 0 by the CU count | 1 row-major | n forced (same bits; A/B) */ \
  X(GEMM_BF16X3_PLANES, "gemm_bf16x3_planes", 1, 'x')  /* image of the bf16x3 planes: 0 [rows][K] | 1 k-tile-major [K / 32][rows][64 B] (same bits; A/B) */ \
  X(GEMM_PRODUCTS, "gemm_products", 6, 'x')            /* plane products of a float32 product on the bf16 matrix cores: 6 full float32 accuracy | 3 a1b1 + a1b2 + a2b1 of two ROUNDED planes | 1 a1b1 of one (anything else: 6). A permission: what the reduced kernels do not take runs as under 6 (ndarray.set_matmul_precision) */ \
  X(JIT_U, "jit_u", 0, 'x')                            /* vector groups per lane and trip of the generated streaming kernels (0: by form) */ \
  X(JIT_BLOCKS, "jit_blocks", 0, 'x')                  /* blocks per CU of the generated EVAL kernels (0: by form) */                     \
  X(JIT_AXES_WIDE, "jit_axes_wide", 0, 'x')            /* 1: generated three / four-axis EVAL kernels take the 64-bit index form at any size (tests) */ \
  X(SWEEP_NB, "sweep_nb", 0, 'x')                      /* fused eval + column sum: row bands (0: by shape) */                   \
  X(SWEEP_RU, "sweep_ru", 0, 'x')                                                                                               \
  X(SWEEP_NT_STORE, "sweep_nt_store", 1, 'x')                                                                                   \
  X(ROWS_WAVE, "rows_wave", 1, 'x')                                                                                             \
  X(COLS_NB, "cols_nb", 0, 'x')                                                                                                 \
  X(ROWS_BLOCKS, "rows_blocks", 0, 'x')                /* blocks of a split row reduction (0: 1024) */                          \
  X(ARG_BLOCKS, "arg_blocks", 0, 'x')                  /* blocks of the strips arg-reduction (0: one per CU) */                 \
  X(ARG_BATCHED, "arg_batched", 1, 'x')                /* 0: argmax / argmin over a middle axis keep the block / thread kernels (A/B) */ \
  X(VAR_BATCHED, "var_batched", 1, 'x')                /* 0: mdhip_var refuses a middle axis, the caller composes (A/B) */      \
  X(VAR_NARROW, "var_narrow", 1, 'x')                  /* 0: mdhip_var refuses float16 / small-integer x, the caller promotes and composes (A/B) */ \
  X(CONVERT_VEC, "convert_vec", 1, 'x')                /* 0: mdhip_convert keeps the one-element k_convert for every call (A/B) */ \
  X(WHERE_VEC, "where_vec", 1, 'x')                    /* 0: `where` with a storage-only result keeps k_nw_where_generic for every call (A/B) */ \
  X(CONVERT_VEC_RUNS, "convert_vec_runs", 0, 'x')      /* a COUNTER, as gemm_narrow_thin_runs: the host adds 1 for every launch it ISSUES of k_nw_convert / k_nw_convert_axes */ \
  X(WHERE_VEC_RUNS, "where_vec_runs", 0, 'x')          /* a COUNTER: the host adds 1 for every launch it ISSUES of k_nw_where / k_nw_where_axes */ \
  X(GATHER_RUNS, "gather_runs", 1, 'x')                                                                                   \
  X(SCATTER_CENSUS, "scatter_census", 1, 'x')                                                                                   \
  X(SCATTER_SORTED, "scatter_sorted", 1, 'x')          /* 0: element-granular duplicates by bid / apply rounds (A/B) */

enum MdOptId {
#define MD_OPT_ENUM(ID, name, dflt, kind) MD_OPT_##ID,
  MD_OPTION_LIST(MD_OPT_ENUM)
#undef MD_OPT_ENUM
  MD_OPT_COUNT
};

struct MdOptDef {
  const char *name;
  int64_t dflt;
  char kind;
};

inline const MdOptDef *md_opt_defs() {
  static const MdOptDef defs[MD_OPT_COUNT] = {
#define MD_OPT_DEF(ID, name, dflt, kind) {name, (int64_t)(dflt), kind},
      MD_OPTION_LIST(MD_OPT_DEF)
#undef MD_OPT_DEF
  };
  return defs;
}

// (one instance per shared object: an inline function's statics are merged across translation units)
inline int64_t *md_opt_table() {
  static int64_t table[MD_OPT_COUNT];
  static const bool loaded = [] {
    const MdOptDef *d = md_opt_defs();
    const char *ex = getenv("MDHIP_EXPERIMENTS");
    const bool experiments = ex && ex[0] == '1' && ex[1] == 0;
    for (int i = 0; i < MD_OPT_COUNT; ++i) {
      table[i] = d[i].dflt;
      if (d[i].kind == 'x' && !experiments) continue;
      char env[64] = "MDHIP_";
      size_t n = strlen(env);
      for (const char *p = d[i].name; *p && n + 1 < sizeof env; ++p) env[n++] = (char)((*p >= 'a' && *p <= 'z') ? *p - 32 : *p);
      env[n] = 0;
      if (const char *v = getenv(env)) table[i] = (int64_t)atoll(v);
    }
    return true;
  }();
  (void)loaded;
  return table;
}
inline int64_t md_opt(int id) { return md_opt_table()[id]; }
inline int md_opt_find(const char *name) {
  const MdOptDef *d = md_opt_defs();
  for (int i = 0; i < MD_OPT_COUNT; ++i)
    if (strcmp(d[i].name, name) == 0) return i;
  return -1;
}
