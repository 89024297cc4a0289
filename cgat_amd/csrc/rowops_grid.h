// Host-side launch arithmetic of the row helpers (rowops.hip): which form a column-sum level takes, its grid and its
// (chunk, column) pair count; the grids of the LayerNorm backward at W = 128 and of the damping-mix backward.  Plain C++,
// no HIP: tools/rowops_grid_check.cpp walks it under the address and undefined-behaviour sanitizers on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#define COLSUM_ROWS 128      // rows per chunk, every form
#define COLSUM_NARROW 16     // the narrow form takes cols <= this
#define LN128_WGS 2048       // four-wave workgroups of the W = 128 LayerNorm backward: 32 waves on each of 256 CUs
#define MIX_BWD_WGS 1024     // workgroup cap of mix_bwd (its partials are summed in workgroup order)

enum { COLSUM_FORM_GENERIC = 0, COLSUM_FORM_NARROW = 1, COLSUM_FORM_WIDE = 2 };

static inline int colsum_chunks(int rows) { return (int)(((long)(rows > 0 ? rows : 1) + COLSUM_ROWS - 1) / COLSUM_ROWS); }

struct ColsumGrid {
  int form;
  long pairs;    // narrow: chunks * cols; wide: chunks * (cols / 4); generic: unused (0)
  int gx, gy;    // grid; gy == 1 in the narrow and wide forms
};

// one level over x [rows, cols] at leading dimension ldx, into dst [chunks, cols] (tight)
static inline ColsumGrid colsum_grid(int rows, int cols, long ldx, const void* x, const void* dst) {
  const long chunks = colsum_chunks(rows);
  ColsumGrid g = {COLSUM_FORM_GENERIC, 0, (int)((cols + 63) / 64), (int)chunks};
  const bool aligned = ((((uintptr_t)x) | ((uintptr_t)dst)) & 15) == 0;
  long pairs = 0;
  if (cols <= COLSUM_NARROW) {
    g.form = COLSUM_FORM_NARROW;
    pairs = chunks * cols;
  } else if (cols % 4 == 0 && ldx % 4 == 0 && aligned) {
    g.form = COLSUM_FORM_WIDE;
    pairs = chunks * (cols / 4);
  }
  if (g.form != COLSUM_FORM_GENERIC) {
    const long gx = (pairs + 63) / 64;
    if (gx > 0x7fffffffL) {       // (rows * cols past 2^37: not a shape of this library; the generic grid still holds it)
      g.form = COLSUM_FORM_GENERIC;
      return g;
    }
    g.pairs = pairs;
    g.gx = (int)gx;
    g.gy = 1;
  }
  return g;
}

static inline int ln128_wgs(int rows) {
  const long w = ((long)rows + 3) / 4;
  return (int)(w < LN128_WGS ? (w < 1 ? 1 : w) : LN128_WGS);
}

// min(grid_for(n), 1024): grid_for is (n + 255) / 256 clamped to [1, 4096]
static inline int mix_bwd_wgs(long n) {
  const long b = (n + 255) / 256;
  return (int)(b > MIX_BWD_WGS ? MIX_BWD_WGS : (b < 1 ? 1 : b));
}
