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
//                    its own fp32 partial.  256 threads, each wave a 64 x 64 quadrant (2 x 2 accumulators); both
//                    operands are 128 x 32 panels of A~^T staged in LDS (pitch 36: 16-byte reads without bank conflicts)
//                    with the next panel prefetched into registers.  A lane's 16-byte read holds four k-steps: k-step q
//                    of a group of 8 rows pairs rows q and 4 + q, the same pairing on both operands.
//   gp_gram_reduce   VALU fp64: adds the slabs in slab order into gram [(M+2)^2] (lower triangle); the first chunk
//                    stores, later chunks add, the last one mirrors into the upper triangle.
// No atomics: bitwise deterministic.  No allocation, no host synchronisation; the only host loop enqueues launches.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_tile.h"

#define GF_TILE 128                // output tile of the Gram product
#define GF_KS 32                   // rows of the chunk per staged panel
#define GF_PITCH 36                // floats per panel row in LDS
#define GF_SLAB 1024               // rows of the chunk per partial
#define GF_THREADS 256

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
  const int n_pairs = (nC + 1) >> 1;
  for (int base = 0; base < n_pairs; base += 16) {
    const int q[2] = {base + wave, base + 15 - wave};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (q[i] < n_pairs) {
        const int c0 = 2 * q[i];
        gp_whiten_group<2>(p, Kt, c0, nC, nk8, min(nk8, 4 * (c0 + 2)), lane, row0 + r, live);
      }
    }
  }
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
__global__ __launch_bounds__(GF_THREADS) void gp_gram_slabs(const float* __restrict__ At, long pitch, int Map, int rows_p,
                                                            float* __restrict__ part, int n_tiles) {
  __shared__ __attribute__((aligned(16))) float panel[2][GF_TILE * GF_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  int ti, tj;
  gf_tile_of(blockIdx.x, ti, tj);
  const int i0 = ti * GF_TILE, j0 = tj * GF_TILE;
  const int n0 = blockIdx.y * GF_SLAB;
  const int n_stage = (min(GF_SLAB, rows_p - n0)) / GF_KS;
  // this wave's 64 x 64 quadrant; one above the diagonal of a diagonal tile, or past the last row, is not computed
  const int wi = 64 * (wave >> 1), wj = 64 * (wave & 1);
  const bool active = i0 + wi < Map && j0 + wj < Map && j0 + wj <= i0 + wi + 63;

  // global -> registers: thread covers float4 (row = tid / 8 + 32 u, columns 4 (tid % 8) ..) of each panel
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
  float4 gA[4], gB[4];
  auto fetch = [&](int stage) {
    const long col = (long)n0 + (long)stage * GF_KS + lc4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ra = i0 + lrow + 32 * u, rb = j0 + lrow + 32 * u;
      gA[u] = ra < Map ? *(const float4*)(At + (long)ra * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      gB[u] = rb < Map ? *(const float4*)(At + (long)rb * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[a][b][t] = 0.f;

  fetch(0);
  for (int stage = 0; stage < n_stage; ++stage) {
    __syncthreads();                 // the previous stage's reads are done
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *(float4*)(panel[0] + (lrow + 32 * u) * GF_PITCH + lc4) = gA[u];
      *(float4*)(panel[1] + (lrow + 32 * u) * GF_PITCH + lc4) = gB[u];
    }
    __syncthreads();
    if (stage + 1 < n_stage) fetch(stage + 1);
    if (active) {
#pragma unroll
      for (int k8 = 0; k8 < GF_KS / 8; ++k8) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          fa[a] = *(const float4*)(panel[0] + (wi + 32 * a + r) * GF_PITCH + 8 * k8 + 4 * hi);
          fb[a] = *(const float4*)(panel[1] + (wj + 32 * a + r) * GF_PITCH + 8 * k8 + 4 * hi);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a].x, fb[b].x, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a].y, fb[b].y, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a].z, fb[b].z, acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a].w, fb[b].w, acc[a][b], 0, 0, 0);
          }
      }
    }
  }
  if (active) {
    float* out = part + ((long)blockIdx.y * n_tiles + blockIdx.x) * (GF_TILE * GF_TILE);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int i = wi + gp_acc_index(a, t, hi), j = wj + 32 * b + r;
          out[i * GF_TILE + j] = acc[a][b][t];
        }
  }
}

// gram [Ma][Ma], Ma = M + 2.  One thread per element of the 128 x 128 tiles of the lower triangle.
__global__ __launch_bounds__(256) void gp_gram_reduce(const float* __restrict__ part, int n_tiles, int n_slabs, int Ma,
                                                      double* __restrict__ gram, int first, int last) {
  int ti, tj;
  gf_tile_of(blockIdx.x, ti, tj);
  const int e = blockIdx.y * 256 + threadIdx.x;          // element of the tile
  const int i = ti * GF_TILE + (e >> 7), j = tj * GF_TILE + (e & 127);
  if (i >= Ma || j > i) return;
  const float* src = part + (long)blockIdx.x * (GF_TILE * GF_TILE) + e;
  double sum = 0.0;
  for (int sl = 0; sl < n_slabs; ++sl) sum += (double)src[(long)sl * n_tiles * (GF_TILE * GF_TILE)];
  if (!first) sum += gram[(long)i * Ma + j];
  gram[(long)i * Ma + j] = sum;
  if (last && i != j) gram[(long)j * Ma + i] = sum;
}

// ---- host ----
struct GfShape {
  int Mp, Dp, Map, n_tiles, eff_chunk, max_slabs;
  size_t at_bytes, part_bytes;
};

static GfShape gf_shape(int N, int M, int D, int chunk_rows) {
  GfShape g;
  g.Mp = (M + 31) & ~31;
  g.Dp = (D + GP_XK - 1) & ~(GP_XK - 1);
  g.Map = (M + 2 + 31) & ~31;
  const int nt = cdiv(g.Map, GF_TILE);
  g.n_tiles = nt * (nt + 1) / 2;
  const long n_p = ((long)N + 31) & ~31L;                 // a chunk never holds more than the rows there are
  g.eff_chunk = (int)(n_p < (long)chunk_rows ? n_p : (long)chunk_rows);
  g.max_slabs = cdiv(g.eff_chunk, GF_SLAB);
  g.at_bytes = ws_round((size_t)g.Map * g.eff_chunk, sizeof(float));
  g.part_bytes = ws_round((size_t)g.max_slabs * g.n_tiles * GF_TILE * GF_TILE, sizeof(float));
  return g;
}

extern "C" size_t cgat_gp_fit_stats_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows) {
  if (N < 1 || M < 1 || M > GP_MAX_M || D < 1 || chunk_rows < 32 || (chunk_rows & 31)) return 0;
  const GfShape g = gf_shape(N, M, D, chunk_rows);
  return g.at_bytes + g.part_bytes;
}

extern "C" int cgat_gp_fit_stats(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D,
                                 const float* Zimg, int32_t M, const float* centroid, const float* znorm,
                                 const float* W1img, float s, float inv_two_l2, int32_t chunk_rows, double* gram, void* ws,
                                 size_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CGAT_CHECK_ARG(N >= 1 && M >= 1 && D >= 1, "gp_fit_stats: N = %d, M = %d, D = %d", (int)N, (int)M, (int)D);
  if (M > GP_MAX_M) {
    cgat_set_error("gp_fit_stats: M = %d inducing points; the whitening kernel keeps a 32 x M tile of the cross-kernel "
                   "matrix in LDS and supports M <= %d", (int)M, GP_MAX_M);
    return CGAT_ERR_UNSUPPORTED;
  }
  CGAT_CHECK_ARG(chunk_rows >= 32 && (chunk_rows & 31) == 0, "gp_fit_stats: chunk_rows = %d is not a positive multiple of 32",
                 (int)chunk_rows);
  CGAT_CHECK_ARG(ldx >= D, "gp_fit_stats: ldx = %ld < D = %d", (long)ldx, (int)D);
  CGAT_CHECK_ARG(X && y_norm && Zimg && centroid && znorm && W1img && gram, "gp_fit_stats: null operand");
  CGAT_CHECK_ARG((((uintptr_t)Zimg | (uintptr_t)W1img) & 15) == 0, "gp_fit_stats: the packed images need 16-byte alignment");
  CGAT_CHECK_ARG(s >= 0.f && inv_two_l2 > 0.f, "gp_fit_stats: outputscale / lengthscale out of range");
  const GfShape g = gf_shape(N, M, D, chunk_rows);
  if (!ws || ws_bytes < g.at_bytes + g.part_bytes) {
    cgat_set_error("gp_fit_stats: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, g.at_bytes + g.part_bytes);
    return CGAT_ERR_WORKSPACE;
  }
  CGAT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "gp_fit_stats: the workspace needs 16-byte alignment");
  Workspace w(ws, ws_bytes);
  float* At = w.take<float>((size_t)g.Map * g.eff_chunk);
  float* part = w.take<float>((size_t)g.max_slabs * g.n_tiles * GF_TILE * GF_TILE);
  GpWhitenArgs a;
  a.ldx = (long)ldx; a.D = D; a.M = M; a.Mp = g.Mp; a.Dp = g.Dp; a.Map = g.Map;
  a.Zimg = (const float4*)Zimg; a.centroid = centroid; a.znorm = znorm; a.W1img = (const float4*)W1img;
  a.s = s; a.inv_two_l2 = inv_two_l2; a.At = At; a.pitch = g.eff_chunk;
  const int Ma = M + 2;
  CGAT_PROF("gp_fit_stats", st);
  for (long base = 0; base < N; base += g.eff_chunk) {
    const long left = (long)N - base;
    const int rows = (int)(left < g.eff_chunk ? left : (long)g.eff_chunk);
    const int rows_p = (rows + 31) & ~31;
    const int n_slabs = cdiv(rows_p, GF_SLAB);
    a.X = X + base * (long)ldx; a.y_norm = y_norm + base; a.G = rows;
    gp_launch_whiten_rows(a, rows_p / GP_ROWS, st);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_gram_slabs, dim3(g.n_tiles, n_slabs), dim3(GF_THREADS), 0, st, At, (long)g.eff_chunk, g.Map, rows_p,
                       part, g.n_tiles);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_gram_reduce, dim3(g.n_tiles, GF_TILE * GF_TILE / 256), dim3(256), 0, st, part, g.n_tiles, n_slabs,
                       Ma, gram, base == 0 ? 1 : 0, base + g.eff_chunk >= N ? 1 : 0);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}
