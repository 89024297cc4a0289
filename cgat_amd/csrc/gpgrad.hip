// Data part of the gradient of the collapsed sparse-GP bound with respect to the inducing points, the lengthscale and
// the outputscale: the second streaming pass of fitting the head that csrc/gphead.hip evaluates, after the
// statistics pass of csrc/gpfit.hip.  With the bound's adjoints G2 = 2 dF/dPsi [M x M] and g = dF/dbeta [M] from the host
// (cgat_amd/gp.py, fp64, rounded to fp32), per row n of X
//
//   a_n = W1 k_n,   q_n = G2 a_n + g (y~_n - c),   u_n = W1^T q_n = dF/dk_n,   r_nm = u_nm k_nm
//   colsum_m = sum_n r_nm      d2sum_m = sum_n r_nm |x_n - z_m|^2      P = sum_n r_n (x_n - centroid)^T   [M x D]
//
// Three factors, not one: W1 carries entries up to 1 / sqrt(jitter), and W1^T G2 W1 as one matrix loses u in fp32 as the
// indefinite one-matrix form of the variance does (cgat_amd/gp.py).  One 32 x 1024 fp32 tile is 128 KB of LDS, so the
// tile of K^T and an intermediate never share a workgroup: a, q, u and r pass through ONE chunk buffer in the workspace,
// inducing-major [Ma_p][pitch] as gp_whiten_rows stores A~^T, each overwriting the one before it (a workgroup copies
// its own 32 columns into LDS before it writes them).  Per chunk of rows, on the caller's stream:
//
//   gp_whiten_rows    (csrc/gpfit.hip) rows 0 .. M - 1 of the buffer = a
//   gp_apply_factor   buffer <- F x buffer for a packed image F, one 512-thread workgroup per tile of 32 rows, the tile in
//                     LDS, gp_factor_products on the f32-input matrix cores: once with F = G2 (full, + g (y~ - c)), once
//                     with F = W1^T (upper triangular: chunk pair c0 starts at column block 4 c0 of the image)
//   gp_weight_rows    phase (a) again (gp_distance_tile): d2 and k = s exp(-d2 inv_two_l2) in registers, r = u k back to
//                     the buffer; sum over the tile's 32 rows of r and of r d2 by lane shuffles, one fp32 partial per
//                     (tile, m).  d2 is the recomputed distance, never -log(k / s) 2 l^2.
//   gp_input_rows     (only where dF/dX is asked for) dX = (R^T-tile x Zc - rho o (x - centroid)) / l^2 of the
//                     chunk's rows: the tile of r in LDS as in gp_apply_factor, rho its column sums, gp_factor_products
//                     with the packed image of Zc^T as the factor; reads the buffer only
//   gp_centre_rows    Xc^T [D][pitch] = (x - centroid)^T of the chunk, rows at or past N zero
//   gp_pair_slabs     R^T Xc over the chunk on the f32-input matrix cores, gp_slab_product (gp_slab.h) as gp_gram_slabs
//                     but with two operands: 128 x 128 output tiles (grid.x), fixed slabs of 1024 rows (grid.y), one fp32
//                     partial each
//   gp_grad_reduce_*  VALU fp64: tiles / slabs added in order (the pairs by gp_slab_reduce); the first chunk stores, later
//                     chunks add.
// No atomics: bitwise deterministic.  No allocation, no host synchronisation; the only host loop enqueues launches.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_slab.h"

struct GpApplyArgs {
  float* At;                       // [Map][pitch]; rows < M of the tile's 32 columns are replaced
  long pitch;
  int G, M, Mp;                    // G: rows of the chunk (columns at or past it are written as 0)
  const float4* Fimg;              // packed image of F [Mp, Mp], zero padded
  int upper;                       // F is upper triangular: column blocks before the diagonal block are not read
  const float* g;                  // [M] or null: + g[m] (y_norm[col] - c)
  const float* y_norm;             // offset to the chunk's first row
  float c;
};

__global__ __launch_bounds__(GP_THREADS) void gp_apply_factor(GpApplyArgs p) {
  __shared__ __attribute__((aligned(16))) float Bt[GP_ROWS * GP_MAX_M];      // the tile [Mp][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int nC = p.Mp >> 5, nk8 = p.Mp >> 3;
  const long row0 = (long)blockIdx.x * GP_ROWS;
  for (int i = tid; i < p.Mp * GP_ROWS; i += GP_THREADS) Bt[i] = p.At[(long)(i >> 5) * p.pitch + row0 + (i & 31)];
  __syncthreads();

  const long col = row0 + r;
  const bool live = col < p.G;
  const float yc = p.g && live ? p.y_norm[col] - p.c : 0.f;
  gp_for_wave_pairs(nC, wave, [&](int c0) {
    const int k8_0 = p.upper ? 4 * c0 : 0;
    f32x16 acc[2];
    gp_factor_products<2>(p.Fimg + (long)k8_0 * 64, Bt + k8_0 * 8 * GP_ROWS, c0, nC, nk8, nk8 - k8_0, lane, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (c0 + j < nC) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int m = gp_acc_index(c0 + j, t, hi);
          if (m < p.M) {
            float v = acc[j][t];
            if (p.g) v = fmaf(p.g[m], yc, v);
            p.At[(long)m * p.pitch + col] = live ? v : 0.f;
          }
        }
      }
    }
  });
}

struct GpWeightArgs : GpTile {
  float* At;                       // [Map][pitch]: u in, r = u k out
  long pitch;
  float* pc;                       // [tile][Mp]: sum over the tile's rows of r
  float* pd;                       // [tile][Mp]: of r d2
};

__global__ __launch_bounds__(GP_THREADS) void gp_weight_rows(GpWeightArgs p) {
  __shared__ float Xs[GP_XK * GP_XP];
  const int r = threadIdx.x & 31;
  const long row0 = (long)blockIdx.x * GP_ROWS;
  const long col = row0 + r;
  const bool live = col < p.G;
  float* pc = p.pc + (long)blockIdx.x * p.Mp;
  float* pd = p.pd + (long)blockIdx.x * p.Mp;
  gp_distance_tile(p, row0, Xs, [&](int m, float d2) {
    float rv = 0.f;
    if (m < p.M) {
      float* at = p.At + (long)m * p.pitch + col;
      if (live) rv = *at * (p.s * expf(-d2 * p.inv_two_l2));
      *at = rv;
    }
    float cs = rv, ds = rv * d2;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {         // the 32 rows of the tile: one half of the wave
      cs += __shfl_xor(cs, o);
      ds += __shfl_xor(ds, o);
    }
    if (r == 0 && m < p.M) {
      pc[m] = cs;
      pd[m] = ds;
    }
  });
}

// dF/dx of the chunk's rows from r: dX[row][d] = (sum_m r[m][row] zc[m][d] - rho[row] (x[row][d] - centroid[d]))
// / l^2 with rho = sum_m r[m][row].  One workgroup per tile of 32 rows, the tile of r [Mp][32] in LDS like gp_apply_factor's;
// rows m >= M of the buffer are y~, 1 and padding (gp_whiten_rows) and are loaded as zero.
struct GpInputArgs {
  const float* At;                 // [Map][pitch]: r in rows < M
  long pitch;
  int G, M, Mp, D;                 // G: rows of the chunk (rows at or past it are not written)
  const float4* Ztimg;             // packed image of Zc^T [D rounded up to 32, Mp], zero padded
  const float* X;                  // offset to the chunk's first row, like dX
  long ldx;
  const float* centroid;
  float inv_two_l2;
  float* dX;
  long lddx;
  int vec_x, vec_dx;               // 16-byte loads of X / stores of dX are aligned
};

__global__ __launch_bounds__(GP_THREADS) void gp_input_rows(GpInputArgs p) {
  __shared__ __attribute__((aligned(16))) float Bt[GP_ROWS * GP_MAX_M];      // the tile [Mp][32]
  __shared__ float part[GP_THREADS];                                        // [16][32] partial column sums
  const int tid = threadIdx.x, r = tid & 31;
  const long row0 = (long)blockIdx.x * GP_ROWS;
  // thread tid copies column tid & 31 of rows tid >> 5, + 16, ...: its partial sum of that column, in row order
  float ps = 0.f;
  for (int i = tid; i < p.Mp * GP_ROWS; i += GP_THREADS) {
    const int m = i >> 5;
    const float v = m < p.M ? p.At[(long)m * p.pitch + row0 + (i & 31)] : 0.f;
    Bt[i] = v;
    ps += v;
  }
  part[tid] = ps;
  __syncthreads();
  float rho = 0.f;
#pragma unroll
  for (int j = 0; j < GP_THREADS / GP_ROWS; ++j) rho += part[j * GP_ROWS + r];     // the 16 partials in a fixed order
  gp_input_tile(p, Bt, rho, row0);                                                 // the product and the stores (gp_tile.h)
}

// Xt [D][pitch]: column n of the chunk is x_n - centroid, 0 for n >= G.  grid (rows_p / 32, cdiv(D, 32)).
__global__ __launch_bounds__(256) void gp_centre_rows(const float* __restrict__ X, long ldx, int G, int D,
                                                      const float* __restrict__ centroid, float* __restrict__ Xt,
                                                      long pitch) {
  __shared__ float tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const long row0 = (long)blockIdx.x * 32;
  const int d0 = blockIdx.y * 32;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long g = row0 + ty + 8 * i;
    const int d = d0 + tx;
    tile[ty + 8 * i][tx] = g < G && d < D ? X[g * ldx + d] - centroid[d] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int d = d0 + ty + 8 * i;
    if (d < D) Xt[(long)d * pitch + row0 + tx] = tile[tx][ty + 8 * i];
  }
}

// Rt [>= M][pitch], Xt [D][pitch]; rows_p (a multiple of 32) columns are valid.  part [slab][tile][128][128], tile =
// ti tiles_d + tj over (M, D).
__global__ __launch_bounds__(GS_THREADS) void gp_pair_slabs(const float* __restrict__ Rt, const float* __restrict__ Xt,
                                                            long pitch, int M, int D, int rows_p, float* __restrict__ part,
                                                            int tiles_d) {
  int wi, wj;
  gp_slab_quadrant(wi, wj);
  const int i0 = (blockIdx.x / tiles_d) * GS_TILE, j0 = (blockIdx.x % tiles_d) * GS_TILE;
  const bool active = i0 + wi < M && j0 + wj < D;
  gp_slab_product(Rt, M, Xt, D, pitch, i0, j0, blockIdx.y * GS_SLAB, rows_p, active,
                  part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (GS_TILE * GS_TILE));
}

// P [M][D].  grid (n_tiles, 128 * 128 / 256): one thread per element of the output tiles.
__global__ __launch_bounds__(256) void gp_grad_reduce_pairs(const float* __restrict__ part, int tiles_d, int n_slabs, int M,
                                                            int D, double* __restrict__ P, int first) {
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int i = (blockIdx.x / tiles_d) * GS_TILE + (e >> 7), j = (blockIdx.x % tiles_d) * GS_TILE + (e & 127);
  if (i >= M || j >= D) return;
  gp_slab_reduce(part, gridDim.x, n_slabs, e, P + (long)i * D + j, first);
}

// colsum [M], d2sum [M] from the per-tile partials [n_row_tiles][Mp].  A block owns GQ_RC_COLS columns; the tiles are
// dealt in GQ_RC_SEGS contiguous segments (segment j: tiles [j, j + 1) n_row_tiles / GQ_RC_SEGS), each added in tile
// order by one thread, the segments then in segment order: a fixed order for a given n_row_tiles.
#define GQ_RC_COLS 16
#define GQ_RC_SEGS 16
__global__ __launch_bounds__(GQ_RC_COLS * GQ_RC_SEGS) void gp_grad_reduce_columns(
    const float* __restrict__ pc, const float* __restrict__ pd, int n_row_tiles, int Mp, int M, double* __restrict__ colsum,
    double* __restrict__ d2sum, int first) {
  __shared__ double part[2][GQ_RC_SEGS][GQ_RC_COLS];
  const int lc = threadIdx.x % GQ_RC_COLS, seg = threadIdx.x / GQ_RC_COLS;
  const int m = blockIdx.x * GQ_RC_COLS + lc;
  const int t0 = (int)((long)seg * n_row_tiles / GQ_RC_SEGS), t1 = (int)((long)(seg + 1) * n_row_tiles / GQ_RC_SEGS);
  double cs = 0.0, ds = 0.0;
  if (m < M) {
    for (int t = t0; t < t1; ++t) {
      cs += (double)pc[(long)t * Mp + m];
      ds += (double)pd[(long)t * Mp + m];
    }
  }
  part[0][seg][lc] = cs;
  part[1][seg][lc] = ds;
  __syncthreads();
  if (seg != 0 || m >= M) return;
  cs = first ? 0.0 : colsum[m];
  ds = first ? 0.0 : d2sum[m];
  double c_new = 0.0, d_new = 0.0;
  for (int j = 0; j < GQ_RC_SEGS; ++j) {
    c_new += part[0][j][lc];
    d_new += part[1][j][lc];
  }
  colsum[m] = cs + c_new;
  d2sum[m] = ds + d_new;
}

// ---- host ----
int gp_launch_row_sums(const GpRowSumsWorkspace& w, const GpChunks& ch, const float* X, long ldx, int M, int D,
                       const float* centroid, double* colsum, double* d2sum, double* P, hipStream_t st) {
  const int n_tiles = GpRowSumsWorkspace::tiles(M, D), tiles_d = cdiv(D, GS_TILE);
  const long pitch = ch.eff_chunk;
  hipLaunchKernelGGL(gp_centre_rows, dim3(ch.row_tiles, cdiv(D, 32)), dim3(256), 0, st, X, ldx, ch.rows, D, centroid, w.Xt,
                     pitch);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_pair_slabs, dim3(n_tiles, ch.n_slabs), dim3(GS_THREADS), 0, st, w.At, w.Xt, pitch, M, D, ch.rows_p,
                     w.part, tiles_d);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_grad_reduce_pairs, dim3(n_tiles, GS_TILE * GS_TILE / 256), dim3(256), 0, st, w.part, tiles_d,
                     ch.n_slabs, M, D, P, ch.first);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(gp_grad_reduce_columns, dim3(cdiv(M, GQ_RC_COLS)), dim3(GQ_RC_COLS * GQ_RC_SEGS), 0, st, w.pc, w.pd,
                     ch.row_tiles, ch.Mp, M, colsum, d2sum, ch.first);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

extern "C" size_t cgat_gp_fit_grad_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows) {
  if (!GpChunks::fits(N, M, D, chunk_rows)) return 0;
  return GpRowSumsWorkspace::bytes(GpChunks(N, M, D, chunk_rows), M, D);
}

// Both entries: `inputs` asks for dX as well (Ztimg, dX, lddx are then checked; ignored otherwise).
static int gp_fit_grad_run(const char* name, bool inputs, const float* X, int64_t ldx, const float* y_norm, int32_t N,
                           int32_t D, const float* Zimg, int32_t M, const float* centroid, const float* znorm,
                           const float* W1img, const float* W1timg, const float* G2img, const float* g, float c, float s,
                           float inv_two_l2, int32_t chunk_rows, double* colsum, double* d2sum, double* P,
                           const float* Ztimg, float* dX, int64_t lddx, void* ws, size_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CGAT_TRY(gp_check_entry(
      name, "N", N, 1, M, D, "the kernels keep a 32 x M tile of the cross-kernel matrix in LDS and support",
      &chunk_rows, ldx, X && y_norm && Zimg && centroid && znorm && W1img && W1timg && G2img && g && colsum && d2sum && P,
      (uintptr_t)Zimg | (uintptr_t)W1img | (uintptr_t)W1timg | (uintptr_t)G2img, s, inv_two_l2));
  if (inputs) {
    CGAT_CHECK_ARG(Ztimg && dX, "%s: null operand", name);
    CGAT_CHECK_ARG(lddx >= D, "%s: lddx = %ld < D = %d", name, (long)lddx, D);
    CGAT_CHECK_ARG(((uintptr_t)Ztimg & 15) == 0, "%s: the packed images need 16-byte alignment", name);
  }
  CGAT_TRY(gp_check_workspace(name, ws, ws_bytes, cgat_gp_fit_grad_workspace_bytes(N, M, D, chunk_rows)));
  GpChunks ch(N, M, D, chunk_rows);
  const GpRowSumsWorkspace w(ch, M, D, ws, ws_bytes);
  float *At = w.At, *pc = w.pc, *pd = w.pd;
  const long pitch = ch.eff_chunk;
  const GpTile tile = gp_tile_operands(X, ldx, 0, D, Zimg, M, centroid, znorm, s, inv_two_l2);
  GpWhitenArgs a{tile, ch.Map, (const float4*)W1img, nullptr, At, pitch};
  GpWeightArgs k{tile, At, pitch, pc, pd};
  GpApplyArgs f;
  f.At = At; f.pitch = pitch; f.M = M; f.Mp = ch.Mp; f.c = c;
  GpInputArgs in{At, pitch, 0, (int)M, ch.Mp, (int)D, (const float4*)Ztimg, X, (long)ldx, centroid, inv_two_l2, dX, (long)lddx,
                 (((uintptr_t)X & 15) == 0 && (ldx & 3) == 0) ? 1 : 0, (((uintptr_t)dX & 15) == 0 && (lddx & 3) == 0) ? 1 : 0};
  CGAT_PROF(name, st);
  while (ch.next()) {
    ch.place(a, X);
    ch.place(k, X);
    a.y_norm = f.y_norm = y_norm + ch.base;
    f.G = ch.rows;
    gp_launch_whiten_rows(a, ch.row_tiles, st);
    CGAT_LAUNCH_CHECK();
    f.Fimg = (const float4*)G2img; f.upper = 0; f.g = g;
    hipLaunchKernelGGL(gp_apply_factor, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    f.Fimg = (const float4*)W1timg; f.upper = 1; f.g = nullptr;
    hipLaunchKernelGGL(gp_apply_factor, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_weight_rows, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, k);
    CGAT_LAUNCH_CHECK();
    if (inputs) {
      in.G = ch.rows;
      in.X = a.X;
      in.dX = dX + ch.base * lddx;
      hipLaunchKernelGGL(gp_input_rows, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, in);
      CGAT_LAUNCH_CHECK();
    }
    CGAT_TRY(gp_launch_row_sums(w, ch, a.X, (long)ldx, M, D, centroid, colsum, d2sum, P, st));
  }
  return CGAT_OK;
}

extern "C" int cgat_gp_fit_grad(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D, const float* Zimg,
                                int32_t M, const float* centroid, const float* znorm, const float* W1img,
                                const float* W1timg, const float* G2img, const float* g, float c, float s,
                                float inv_two_l2, int32_t chunk_rows, double* colsum, double* d2sum, double* P, void* ws,
                                size_t ws_bytes, void* stream) {
  return gp_fit_grad_run("gp_fit_grad", false, X, ldx, y_norm, N, D, Zimg, M, centroid, znorm, W1img, W1timg, G2img, g, c, s,
                         inv_two_l2, chunk_rows, colsum, d2sum, P, nullptr, nullptr, 0, ws, ws_bytes, stream);
}

extern "C" int cgat_gp_fit_grad_inputs(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D,
                                       const float* Zimg, int32_t M, const float* centroid, const float* znorm,
                                       const float* W1img, const float* W1timg, const float* G2img, const float* g, float c,
                                       float s, float inv_two_l2, int32_t chunk_rows, double* colsum, double* d2sum,
                                       double* P, const float* Ztimg, float* dX, int64_t lddx, void* ws, size_t ws_bytes,
                                       void* stream) {
  return gp_fit_grad_run("gp_fit_grad_inputs", true, X, ldx, y_norm, N, D, Zimg, M, centroid, znorm, W1img, W1timg, G2img, g,
                         c, s, inv_two_l2, chunk_rows, colsum, d2sum, P, Ztimg, dX, lddx, ws, ws_bytes, stream);
}
