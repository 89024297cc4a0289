// Host-side launch arithmetic of the row helpers (cgat_amd/csrc/rowops_grid.h), walked on the CPU: for every shape of
// tests/test_row_helpers.py the grid of each column-sum level, of the W = 128 LayerNorm backward and of the damping-mix
// backward is replayed thread by thread with the index arithmetic of the kernels in csrc/rowops.hip, on heap buffers of
// exactly the operand sizes.  Every input element must be read once, every output written once, nothing else touched.
// Build and run under the sanitizers (CPU only, no GPU, not loaded into Python):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I cgat_amd/csrc
//       tools/rowops_grid_check.cpp -o build/rowops_grid_check && build/rowops_grid_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rowops_grid.h"

static int fails = 0;
#define EXPECT(cond, ...)                    \
  do {                                       \
    if (!(cond)) {                           \
      ++fails;                               \
      fprintf(stderr, "FAIL: " __VA_ARGS__); \
      fprintf(stderr, "\n");                 \
    }                                        \
  } while (0)

// one level: reads[r * ldx + c] and writes[chunk * cols + c] are counted as the kernels index them
static void colsum_level(int rows, int cols, long ldx, bool aligned, int expect_form) {
  const int chunks = colsum_chunks(rows);
  std::vector<unsigned char> reads((size_t)(rows > 0 ? (rows - 1) * ldx + cols : 0), 0), writes((size_t)chunks * cols, 0);
  const void* base = aligned ? (const void*)256 : (const void*)260;
  const ColsumGrid g = colsum_grid(rows, cols, ldx, base, (const void*)512);
  EXPECT(g.form == expect_form, "form %d, expected %d at rows %d cols %d ldx %ld", g.form, expect_form, rows, cols, ldx);
  EXPECT(g.gx >= 1 && g.gy >= 1, "empty grid at rows %d cols %d", rows, cols);
  for (int by = 0; by < g.gy; ++by)
    for (int bx = 0; bx < g.gx; ++bx)
      for (int t = 0; t < 256; ++t) {
        if (g.form == COLSUM_FORM_GENERIC) {
          const int cl = t & 63, rl = t >> 6, c = bx * 64 + cl;
          const int r0 = by * COLSUM_ROWS, r1 = rows < r0 + COLSUM_ROWS ? rows : r0 + COLSUM_ROWS;
          if (c < cols) {
            for (int r = r0 + rl; r < r1; r += 4) ++reads.at((size_t)r * ldx + c);
            if (rl == 0) ++writes.at((size_t)by * cols + c);
          }
          continue;
        }
        const bool wide = g.form == COLSUM_FORM_WIDE;
        const int per = wide ? cols / 4 : cols, w = wide ? 4 : 1;
        const int rl = wide ? t >> 6 : t & 3, sl = wide ? t & 63 : t >> 2;
        const long pair = (long)bx * 64 + sl;
        if (pair >= g.pairs) continue;
        const int chunk = (int)(pair / per), c = (int)(pair % per) * w;
        const int r0 = chunk * COLSUM_ROWS, r1 = rows < r0 + COLSUM_ROWS ? rows : r0 + COLSUM_ROWS;
        int r = r0 + rl;
        for (; r + 28 < r1; r += 32)
          for (int j = 0; j < 8; ++j)
            for (int k = 0; k < w; ++k) ++reads.at((size_t)(r + 4 * j) * ldx + c + k);
        for (; r < r1; r += 4)
          for (int k = 0; k < w; ++k) ++reads.at((size_t)r * ldx + c + k);
        if (rl == 0)
          for (int k = 0; k < w; ++k) ++writes.at((size_t)pair * w + k);
      }
  for (int r = 0; r < rows; ++r)
    for (long c = 0; c < ldx && (size_t)(r * ldx + c) < reads.size(); ++c)
      EXPECT(reads[(size_t)r * ldx + c] == (c < cols ? 1 : 0), "rows %d cols %d ldx %ld: element (%d, %ld) read %d times", rows,
             cols, ldx, r, c, reads[(size_t)r * ldx + c]);
  for (size_t i = 0; i < writes.size(); ++i)
    EXPECT(writes[i] == 1, "rows %d cols %d ldx %ld: partial %zu written %d times", rows, cols, ldx, i, writes[i]);
}

static int expected_form(int cols, long ldx, bool aligned) {
  if (cols <= COLSUM_NARROW) return COLSUM_FORM_NARROW;
  return (cols % 4 == 0 && ldx % 4 == 0 && aligned) ? COLSUM_FORM_WIDE : COLSUM_FORM_GENERIC;
}

static void colsum_all_levels(int rows, int cols, bool padded) {
  long ld = padded ? cols + 4 : cols;
  bool aligned = !padded;
  int n = rows;
  while (true) {
    colsum_level(n, cols, ld, aligned, expected_form(cols, ld, aligned));
    const int chunks = colsum_chunks(n);
    if (chunks == 1) break;
    n = chunks;      // the partials: tight, in the 256-byte aligned workspace
    ld = cols;
    aligned = true;
  }
}

static void ln128(int rows) {
  std::vector<unsigned char> seen((size_t)rows, 0);
  const int wgs = ln128_wgs(rows);
  EXPECT(wgs >= 1 && wgs <= LN128_WGS, "ln128: %d workgroups at %d rows", wgs, rows);
  const long stride = (long)wgs * 4;
  for (long wave = 0; wave < stride; ++wave) {
    long ra = wave;
    if (ra >= rows) continue;
    while (true) {      // the loop of layernorm_tanh_bwd128_kernel: stores only
      const long rb = ra + stride;
      ++seen.at((size_t)ra);
      const long rn = rb + stride;
      if (rb < rows) ++seen.at((size_t)rb);
      if (rn >= rows) break;
      ra = rn;
    }
  }
  for (int r = 0; r < rows; ++r) EXPECT(seen[r] == 1, "ln128: row %d of %d written %d times", r, rows, seen[r]);
}

static void mix_bwd(long n) {
  std::vector<unsigned char> seen((size_t)n, 0);
  const int wgs = mix_bwd_wgs(n);
  EXPECT(wgs >= 1 && wgs <= MIX_BWD_WGS, "mix_bwd: %d workgroups at n %ld", wgs, n);
  const long stride = (long)wgs * 256;
  for (long t = 0; t < stride; ++t) {
    long i = t;
    for (; i + 3 * stride < n; i += 4 * stride)
      for (int j = 0; j < 4; ++j) ++seen.at((size_t)(i + j * stride));
    for (; i < n; i += stride) ++seen.at((size_t)i);
  }
  for (long i = 0; i < n; ++i) EXPECT(seen[i] == 1, "mix_bwd: element %ld of %ld touched %d times", i, n, seen[i]);
}

int main() {
  const int rows[] = {0, 1, 3, 4, 5, 127, 128, 129, 513, 16385}, cols[] = {1, 3, 5, 16, 20, 63, 64, 65, 128, 132, 1536};
  for (int r : rows)
    for (int c : cols)
      for (int padded = 0; padded < 2; ++padded) colsum_all_levels(r, c, padded != 0);
  colsum_all_levels(1000080, 3, false);      // ga [E, H] of the benchmark batch
  colsum_all_levels(83340, 1536, false);     // Gi [N, 2 H Hd]
  const ColsumGrid big = colsum_grid(2147483647, 16, 16, (const void*)256, (const void*)512);
  EXPECT(big.form == COLSUM_FORM_NARROW && big.pairs == (long)colsum_chunks(2147483647) * 16 && big.gx == (big.pairs + 63) / 64,
         "narrow form at 2^31 - 1 rows: form %d pairs %ld gx %d", big.form, big.pairs, big.gx);
  for (int r : {1, 3, 4, 5, 257, 1023, 8191, 8192, 8193, 16385, 83340}) ln128(r);
  for (long n : {0L, 1L, 128L, 65L * 128, 300L * 128, 2048L * 128, 2049L * 128, 4L * 262144 + 5, 83340L * 128}) mix_bwd(n);
  printf(fails ? "%d failures\n" : "rowops grid check: ok\n", fails);
  return fails ? 1 : 0;
}
