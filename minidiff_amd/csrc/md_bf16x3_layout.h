// md_bf16x3_layout.h — where the bf16x3 product's bytes lie and in which order its tiles run (gemm_bf16x3.hip; host-testable).
//
// Plane image. A plane holds rows x K bfloat16 (K a multiple of 32). The offset of element (row, k) is
//   (k / 32) * kstep + row * rs + (k % 32) * 2      bytes,
// one form for both layouts (option gemm_bf16x3_planes), told apart by the two strides alone:
//   0  [rows][K]           rs = 2 K, kstep = 64            a 16-row piece of a k-tile is 16 half-used 128-B lines, 2 K bytes apart
//   1  [K / 32][rows][64]  rs = 64,  kstep = 64 rows       the same piece is ONE contiguous 1 KiB, no line shared with another k-tile
// kstep depends on the operand's row count under layout 1: A and B of one product step differently along k.
//
// Tile walk. The product's blocks are numbered wg = 0 .. tiles_m * tiles_n - 1 and every XCD takes a contiguous chunk of that
// numbering (the kernel's bijective chunking); the blocks resident together on an XCD are therefore consecutive wg, and the step from
// wg to a tile decides which operand rows they share in L2. Grouped order with band height gm: the tile rows are cut into groups of gm
// (the last one ragged: min(gm, tiles_m - first_m) rows), a group's tiles are numbered with tile_m running fastest, group after
// group. gm = 1 is the row-major walk (tile_m = wg / tiles_n). md_bf16x3_band picks gm so that the R blocks resident on an XCD read
// the fewest operand rows: 256 gm of A and 128 ceil(R / gm) of B.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_BX3L_HD __host__ __device__
#else
#define MD_BX3L_HD
#endif

MD_BX3L_HD inline int64_t md_bf16x3_row_stride(int planes, int64_t K) { return planes ? 64 : K * 2; }
MD_BX3L_HD inline int64_t md_bf16x3_k_step(int planes, int64_t rows) { return planes ? rows * 64 : 64; }
MD_BX3L_HD inline int64_t md_bf16x3_plane_off(int64_t row, int64_t k, int64_t rs, int64_t kstep) { return (k >> 5) * kstep + row * rs + (k & 31) * 2; }

// wg -> (tile_m, tile_n); 0 <= wg < tiles_m * tiles_n, gm >= 1
MD_BX3L_HD inline void md_bf16x3_tile(int wg, int tiles_m, int tiles_n, int gm, int *tile_m, int *tile_n) {
  const int per_group = gm * tiles_n, grp = wg / per_group, first_m = grp * gm, in = wg - grp * per_group;
  const int h = tiles_m - first_m < gm ? tiles_m - first_m : gm;
  *tile_n = in / h;
  *tile_m = first_m + (in - *tile_n * h);
}

// band height for `resident` blocks per XCD and 256 x 128 tiles, clipped to tiles_m; `forced` > 0 overrides the choice (clipped too)
inline int md_bf16x3_band(int tiles_m, int resident, int forced) {
  int gm = forced;
  if (gm <= 0) {
    int64_t best = -1;
    for (int h = 1; h <= resident; ++h) {
      const int64_t rows = 256 * (int64_t)h + 128 * (int64_t)((resident + h - 1) / h);
      if (best < 0 || rows < best) { best = rows; gm = h; }
    }
  }
  if (gm > tiles_m) gm = tiles_m;
  return gm < 1 ? 1 : gm;
}
