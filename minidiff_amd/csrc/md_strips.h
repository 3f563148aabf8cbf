// md_strips.h — host side of the column-strips walk (k_reduce_cols_strips, k_arg_cols_strips, k_var_cols, the generated sweep
// kernel, k_skinny_colsum): NS strips of 64 lanes x one 16-B vector across the columns, each cut into NB interleaved row bands;
// the last block of a strip folds the NB partial rows of that strip, which it holds in registers (md_ticket.h). Here: the one
// computation of NB, and the holder of a launch's scratch blocks. Host code only (md_ticket.h is also compiled by hiprtc).
#pragma once
#include <stddef.h>
#include <stdint.h>

extern "C" int mdhip_alloc(size_t, void **);
extern "C" int mdhip_free(void *);

enum MdRound { MD_FLOOR, MD_CEIL };

static inline int64_t md_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The band count: `target` blocks in all over `per_band` strip-blocks per band (NS * outer), rounded as the caller says; then
// <= 64 bands (the last block of a strip holds all its partial rows in registers), a band holds >= rows_per_band rows, >= 1.
// A forced count (an option) goes in as target with per_band 1. What differs from caller to caller — the ticket fit, the
// halving for 32-bit partial offsets — stays with the caller.
static inline int64_t md_strips_bands(int64_t per_band, int64_t target, MdRound round, int64_t n_red, int64_t rows_per_band) {
  int64_t nb = (round == MD_CEIL ? target + per_band - 1 : target) / per_band;
  if (nb > 64) nb = 64;
  if (nb > n_red / rows_per_band) nb = n_red / rows_per_band;
  if (nb < 1) nb = 1;
  return nb;
}

// The scratch blocks of one launch sequence (at most three), freed when the holder leaves scope. mdhip_free is stream-ordered:
// the next user of a block runs after the kernels launched before the free, so leaving scope right behind the launch is safe.
struct MdScratch {
  void *p[3] = {nullptr, nullptr, nullptr};
  int n = 0;
  MdScratch() = default;
  MdScratch(const MdScratch &) = delete;
  MdScratch &operator=(const MdScratch &) = delete;
  ~MdScratch() {
    for (int i = 0; i < n; ++i) mdhip_free(p[i]);
  }
  // bytes == 0: nothing to allocate, *out stays null
  int get(size_t bytes, void **out) {
    *out = nullptr;
    if (bytes == 0) return 0;
    const int rc = mdhip_alloc(bytes, &p[n]);
    if (rc != 0) return rc;
    *out = p[n++];
    return 0;
  }
};
