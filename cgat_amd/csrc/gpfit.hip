// Sufficient statistics of the collapsed sparse-GP bound: the data pass of fitting the head that
// csrc/gphead.hip evaluates.  The reference (CGAT/gaussian_process.py:45-66, trained at :233 with VariationalELBO under a
// GaussianLikelihood, targets normalised at :200-204) maximises the bound by minibatch AdamW; for a Gaussian likelihood
// the maximiser in (m, L_S) is closed-form (Titsias' collapsed bound) and the data enter only through
//
//   G = sum_n a~_n a~_n^T   [(M+2) x (M+2)],   a~_n = [a_n, y~_n, 1],   a_n = W1 k(Z, x_n),   W1 = L^-1,
//   k(x, z) = s exp(-max(|x - z|^2, 0) inv_two_l2),   L = chol(K_zz + jitter I)
//
// The WHITENED rows are accumulated: accumulating K_zx K_xz and whitening afterwards multiplies the fp32 rounding error by
// up to s / jitter.  Per chunk of rows, three launches on the caller's stream:
//
//   gp_whiten_rows   phases (a) and (b, W1 only) of gp_predict_kernel (gp_tile.h): one 512-thread workgroup per tile of
//                    32 rows, K^T tile resident in LDS, W1 from its packed image with the triangle stopped at the
//                    diagonal block, v_mfma_f32_32x32x2_f32.  The accumulators (X row on the lane, inducing index in
//                    the registers) are stored, not squared: A~^T [Ma_p][pitch] inducing-major, so every store is a
//                    128-byte run across 32 lanes.  Row M is y~, row M + 1 is 1, rows M + 2 .. Ma_p - 1 are 0; columns
//                    of rows >= N are 0 in every row.  Ma_p = M + 2 rounded up to 32.
//   gp_gram_slabs    C = A~^T A~ over the chunk on the f32-input matrix cores: 128 x 128 output tiles of the lower
//                    triangle (grid.x), the chunk's rows dealt in fixed slabs of 1024 (grid.y); each (tile, slab) writes
//                    its own fp32 partial.  The product of one (tile, slab) is gp_slab_product (gp_slab.h) with A~^T as
//                    both operands.
//   gp_gram_reduce   VALU fp64 (gp_slab_reduce): adds the slabs in slab order into gram [(M+2)^2] (lower triangle); the
//                    first chunk stores, later chunks add, the last one mirrors into the upper triangle.
// No atomics: bitwise deterministic.  No allocation, no host synchronisation; the only host loop enqueues launches.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_slab.h"

// Stores the accumulators of NB chunks of W1 K^T: inducing index m to row m of A~^T, X row r to column col.
template <int NB>
__device__ __forceinline__ void gp_whiten_group(const GpWhitenArgs& p, const float* Kt, int c0, int nC, int nk8,
                                                int k8_end, int lane, long col, bool live) {
  const int hi = lane >> 5;
  f32x16 acc[NB];
  gp_factor_products<NB>(p.W1img, Kt, c0, nC, nk8, k8_end, lane, acc);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (c0 + j < nC) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int m = gp_acc_index(c0 + j, t, hi);
        if (m < p.M) p.At[(long)m * p.pitch + col] = live ? acc[j][t] : 0.f;   // rows M .. are written below
      }
    }
  }
}

__global__ __launch_bounds__(GP_THREADS) void gp_whiten_rows(GpWhitenArgs p) {
  // one LDS block: K^T tile [Mp][32] | staged X [64][33]
  __shared__ __attribute__((aligned(16))) float lds[GP_ROWS * GP_MAX_M + GP_XK * GP_XP];
  float* Kt = lds;
  float* Xs = lds + GP_ROWS * GP_MAX_M;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31;
  const int nC = p.Mp >> 5;
  const long row0 = (long)blockIdx.x * GP_ROWS;

  // ---- (a) cross products, norms, exp ----
  gp_kernel_tile(p, row0, Kt, Xs);
  __syncthreads();

  // ---- (b) a = W1 k on the matrix cores, stored ----
  const int nk8 = p.Mp >> 3;
  const bool live = row0 + r < p.G;
  gp_for_wave_pairs(nC, wave, [&](int c0) {
    gp_whiten_group<2>(p, Kt, c0, nC, nk8, min(nk8, 4 * (c0 + 2)), lane, row0 + r, live);
  });
  // ---- rows M (y~), M + 1 (ones), M + 2 .. Ma_p - 1 (zero) ----
  for (int i = tid; i < (p.Map - p.M) * GP_ROWS; i += GP_THREADS) {
    const int m = p.M + (i >> 5), col = i & 31;
    const long g = row0 + col;
    float v = 0.f;
    if (g < p.G) v = m == p.M ? p.y_norm[g] : (m == p.M + 1 ? 1.f : 0.f);
    p.At[(long)m * p.pitch + g] = v;
  }
}

void gp_launch_whiten_rows(const GpWhitenArgs& args, int n_tiles, hipStream_t stream) {
  hipLaunchKernelGGL(gp_whiten_rows, dim3(n_tiles), dim3(GP_THREADS), 0, stream, args);
}

// Lower-triangle tile number t -> (ti, tj), tj <= ti.
__device__ __forceinline__ void gf_tile_of(int t, int& ti, int& tj) {
  ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  tj = t - ti * (ti + 1) / 2;
}

// At [Map][pitch]; rows_p (a multiple of 32) columns of it are valid.  part [slab][tile][128][128].
__global__ __launch_bounds__(GS_THREADS) void gp_gram_slabs(const float* __restrict__ At, long pitch, int Map, int rows_p,
                                                            float* __restrict__ part, int n_tiles) {
  int ti, tj, wi, wj;
  gf_tile_of(blockIdx.x, ti, tj);
  gp_slab_quadrant(wi, wj);
  const int i0 = ti * GS_TILE, j0 = tj * GS_TILE;
  // a quadrant above the diagonal of a diagonal tile, or past the last row, is not computed
  const bool active = i0 + wi < Map && j0 + wj < Map && j0 + wj <= i0 + wi + 63;
  gp_slab_product(At, Map, At, Map, pitch, i0, j0, blockIdx.y * GS_SLAB, rows_p, active,
                  part + ((long)blockIdx.y * n_tiles + blockIdx.x) * (GS_TILE * GS_TILE));
}

// gram [Ma][Ma], Ma = M + 2.  One thread per element of the 128 x 128 tiles of the lower triangle.
__global__ __launch_bounds__(256) void gp_gram_reduce(const float* __restrict__ part, int n_tiles, int n_slabs, int Ma,
                                                      double* __restrict__ gram, int first, int last) {
  int ti, tj;
  gf_tile_of(blockIdx.x, ti, tj);
  const int e = blockIdx.y * 256 + threadIdx.x;          // element of the tile
  const int i = ti * GS_TILE + (e >> 7), j = tj * GS_TILE + (e & 127);
  if (i >= Ma || j > i) return;
  const double sum = gp_slab_reduce(part, n_tiles, n_slabs, e, gram + (long)i * Ma + j, first);
  if (last && i != j) gram[(long)j * Ma + i] = sum;
}

// ---- host ----
static int gf_tiles(const GpChunks& c) {                   // 128 x 128 tiles of the lower triangle of [Map][Map]
  const int nt = cdiv(c.Map, GS_TILE);
  return nt * (nt + 1) / 2;
}
static size_t gf_part_elems(const GpChunks& c) { return (size_t)c.max_slabs * gf_tiles(c) * GS_TILE * GS_TILE; }

extern "C" size_t cgat_gp_fit_stats_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows) {
  if (!GpChunks::fits(N, M, D, chunk_rows)) return 0;
  const GpChunks c(N, M, D, chunk_rows);
  return ws_round(c.at_elems(), sizeof(float)) + ws_round(gf_part_elems(c), sizeof(float));
}

extern "C" int cgat_gp_fit_stats(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D,
                                 const float* Zimg, int32_t M, const float* centroid, const float* znorm,
                                 const float* W1img, float s, float inv_two_l2, int32_t chunk_rows, double* gram, void* ws,
                                 size_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CGAT_TRY(gp_check_entry("gp_fit_stats", "N", N, 1, M, D,
                          "the whitening kernel keeps a 32 x M tile of the cross-kernel matrix in LDS and supports",
                          &chunk_rows, ldx, X && y_norm && Zimg && centroid && znorm && W1img && gram,
                          (uintptr_t)Zimg | (uintptr_t)W1img, s, inv_two_l2));
  CGAT_TRY(gp_check_workspace("gp_fit_stats", ws, ws_bytes, cgat_gp_fit_stats_workspace_bytes(N, M, D, chunk_rows)));
  GpChunks c(N, M, D, chunk_rows);
  Workspace w(ws, ws_bytes);
  float* At = w.take<float>(c.at_elems());
  float* part = w.take<float>(gf_part_elems(c));
  GpWhitenArgs a{gp_tile_operands(X, ldx, 0, D, Zimg, M, centroid, znorm, s, inv_two_l2), c.Map, (const float4*)W1img,
                 nullptr, At, (long)c.eff_chunk};
  const int n_tiles = gf_tiles(c), Ma = M + 2;
  CGAT_PROF("gp_fit_stats", st);
  while (c.next()) {
    c.place(a, X);
    a.y_norm = y_norm + c.base;
    gp_launch_whiten_rows(a, c.row_tiles, st);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_gram_slabs, dim3(n_tiles, c.n_slabs), dim3(GS_THREADS), 0, st, At, a.pitch, c.Map, c.rows_p, part,
                       n_tiles);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_gram_reduce, dim3(n_tiles, GS_TILE * GS_TILE / 256), dim3(256), 0, st, part, n_tiles, c.n_slabs, Ma,
                       gram, c.first, c.last);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}
