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
//   gp_centre_rows    Xc^T [D][pitch] = (x - centroid)^T of the chunk, rows at or past N zero
//   gp_pair_slabs     R^T Xc over the chunk on the f32-input matrix cores, the structure of gp_gram_slabs with two
//                     operands: 128 x 128 output tiles (grid.x), fixed slabs of 1024 rows (grid.y), one fp32 partial each
//   gp_grad_reduce_*  VALU fp64: tiles / slabs added in order; the first chunk stores, later chunks add.
// No atomics: bitwise deterministic.  No allocation, no host synchronisation; the only host loop enqueues launches.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_tile.h"

#define GQ_TILE 128                // output tile of R^T Xc
#define GQ_KS 32                   // rows of the chunk per staged panel
#define GQ_PITCH 36                // floats per panel row in LDS
#define GQ_SLAB 1024               // rows of the chunk per partial
#define GQ_THREADS 256

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
  const int n_pairs = (nC + 1) >> 1;
  for (int base = 0; base < n_pairs; base += 16) {
    const int q[2] = {base + wave, base + 15 - wave};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (q[i] < n_pairs) {
        const int c0 = 2 * q[i];
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
      }
    }
  }
}

struct GpWeightArgs {
  const float* X;                  // already offset to the chunk's first row
  long ldx;
  int G, D, M;
  int Mp, Dp;
  const float4* Zimg;
  const float* centroid;
  const float* znorm;
  float s, inv_two_l2;
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
__global__ __launch_bounds__(GQ_THREADS) void gp_pair_slabs(const float* __restrict__ Rt, const float* __restrict__ Xt,
                                                            long pitch, int M, int D, int rows_p, float* __restrict__ part,
                                                            int tiles_d) {
  __shared__ __attribute__((aligned(16))) float panel[2][GQ_TILE * GQ_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int i0 = (blockIdx.x / tiles_d) * GQ_TILE, j0 = (blockIdx.x % tiles_d) * GQ_TILE;
  const int n0 = blockIdx.y * GQ_SLAB;
  const int n_stage = (min(GQ_SLAB, rows_p - n0)) / GQ_KS;
  const int wi = 64 * (wave >> 1), wj = 64 * (wave & 1);       // this wave's 64 x 64 quadrant
  const bool active = i0 + wi < M && j0 + wj < D;

  // global -> registers: thread covers float4 (row = tid / 8 + 32 u, columns 4 (tid % 8) ..) of each panel
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
  float4 gA[4], gB[4];
  auto fetch = [&](int stage) {
    const long col = (long)n0 + (long)stage * GQ_KS + lc4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ra = i0 + lrow + 32 * u, rb = j0 + lrow + 32 * u;
      gA[u] = ra < M ? *(const float4*)(Rt + (long)ra * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      gB[u] = rb < D ? *(const float4*)(Xt + (long)rb * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
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
      *(float4*)(panel[0] + (lrow + 32 * u) * GQ_PITCH + lc4) = gA[u];
      *(float4*)(panel[1] + (lrow + 32 * u) * GQ_PITCH + lc4) = gB[u];
    }
    __syncthreads();
    if (stage + 1 < n_stage) fetch(stage + 1);
    if (active) {
#pragma unroll
      for (int k8 = 0; k8 < GQ_KS / 8; ++k8) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          fa[a] = *(const float4*)(panel[0] + (wi + 32 * a + r) * GQ_PITCH + 8 * k8 + 4 * hi);
          fb[a] = *(const float4*)(panel[1] + (wj + 32 * a + r) * GQ_PITCH + 8 * k8 + 4 * hi);
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
    float* out = part + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (GQ_TILE * GQ_TILE);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int i = wi + gp_acc_index(a, t, hi), j = wj + 32 * b + r;
          out[i * GQ_TILE + j] = acc[a][b][t];
        }
  }
}

// P [M][D].  grid (n_tiles, 128 * 128 / 256): one thread per element of the output tiles.
__global__ __launch_bounds__(256) void gp_grad_reduce_pairs(const float* __restrict__ part, int tiles_d, int n_slabs, int M,
                                                            int D, double* __restrict__ P, int first) {
  const int e = blockIdx.y * 256 + threadIdx.x;
  const int i = (blockIdx.x / tiles_d) * GQ_TILE + (e >> 7), j = (blockIdx.x % tiles_d) * GQ_TILE + (e & 127);
  if (i >= M || j >= D) return;
  const float* src = part + (long)blockIdx.x * (GQ_TILE * GQ_TILE) + e;
  double sum = 0.0;
  for (int sl = 0; sl < n_slabs; ++sl) sum += (double)src[(long)sl * gridDim.x * (GQ_TILE * GQ_TILE)];
  if (!first) sum += P[(long)i * D + j];
  P[(long)i * D + j] = sum;
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
struct GqShape {
  int Mp, Dp, Map, tiles_m, tiles_d, eff_chunk, max_slabs;
  size_t at_bytes, xt_bytes, col_bytes, part_bytes;
  size_t total() const { return at_bytes + xt_bytes + 2 * col_bytes + part_bytes; }
};

static GqShape gq_shape(int N, int M, int D, int chunk_rows) {
  GqShape g;
  g.Mp = (M + 31) & ~31;
  g.Dp = (D + GP_XK - 1) & ~(GP_XK - 1);
  g.Map = (M + 2 + 31) & ~31;
  g.tiles_m = cdiv(M, GQ_TILE);
  g.tiles_d = cdiv(D, GQ_TILE);
  const long n_p = ((long)N + 31) & ~31L;                 // a chunk never holds more than the rows there are
  g.eff_chunk = (int)(n_p < (long)chunk_rows ? n_p : (long)chunk_rows);
  g.max_slabs = cdiv(g.eff_chunk, GQ_SLAB);
  g.at_bytes = ws_round((size_t)g.Map * g.eff_chunk, sizeof(float));
  g.xt_bytes = ws_round((size_t)D * g.eff_chunk, sizeof(float));
  g.col_bytes = ws_round((size_t)(g.eff_chunk / GP_ROWS) * g.Mp, sizeof(float));
  g.part_bytes = ws_round((size_t)g.max_slabs * g.tiles_m * g.tiles_d * GQ_TILE * GQ_TILE, sizeof(float));
  return g;
}

extern "C" size_t cgat_gp_fit_grad_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows) {
  if (N < 1 || M < 1 || M > GP_MAX_M || D < 1 || chunk_rows < 32 || (chunk_rows & 31)) return 0;
  return gq_shape(N, M, D, chunk_rows).total();
}

extern "C" int cgat_gp_fit_grad(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D, const float* Zimg,
                                int32_t M, const float* centroid, const float* znorm, const float* W1img,
                                const float* W1timg, const float* G2img, const float* g, float c, float s,
                                float inv_two_l2, int32_t chunk_rows, double* colsum, double* d2sum, double* P, void* ws,
                                size_t ws_bytes, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  CGAT_CHECK_ARG(N >= 1 && M >= 1 && D >= 1, "gp_fit_grad: N = %d, M = %d, D = %d", (int)N, (int)M, (int)D);
  if (M > GP_MAX_M) {
    cgat_set_error("gp_fit_grad: M = %d inducing points; the kernels keep a 32 x M tile of the cross-kernel matrix in LDS "
                   "and support M <= %d", (int)M, GP_MAX_M);
    return CGAT_ERR_UNSUPPORTED;
  }
  CGAT_CHECK_ARG(chunk_rows >= 32 && (chunk_rows & 31) == 0, "gp_fit_grad: chunk_rows = %d is not a positive multiple of 32",
                 (int)chunk_rows);
  CGAT_CHECK_ARG(ldx >= D, "gp_fit_grad: ldx = %ld < D = %d", (long)ldx, (int)D);
  CGAT_CHECK_ARG(X && y_norm && Zimg && centroid && znorm && W1img && W1timg && G2img && g && colsum && d2sum && P,
                 "gp_fit_grad: null operand");
  CGAT_CHECK_ARG((((uintptr_t)Zimg | (uintptr_t)W1img | (uintptr_t)W1timg | (uintptr_t)G2img) & 15) == 0,
                 "gp_fit_grad: the packed images need 16-byte alignment");
  CGAT_CHECK_ARG(s >= 0.f && inv_two_l2 > 0.f, "gp_fit_grad: outputscale / lengthscale out of range");
  const GqShape q = gq_shape(N, M, D, chunk_rows);
  if (!ws || ws_bytes < q.total()) {
    cgat_set_error("gp_fit_grad: workspace of %zu bytes, %zu needed", ws ? ws_bytes : (size_t)0, q.total());
    return CGAT_ERR_WORKSPACE;
  }
  CGAT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "gp_fit_grad: the workspace needs 16-byte alignment");
  Workspace w(ws, ws_bytes);
  float* At = w.take<float>((size_t)q.Map * q.eff_chunk);
  float* Xt = w.take<float>((size_t)D * q.eff_chunk);
  float* pc = w.take<float>((size_t)(q.eff_chunk / GP_ROWS) * q.Mp);
  float* pd = w.take<float>((size_t)(q.eff_chunk / GP_ROWS) * q.Mp);
  float* part = w.take<float>((size_t)q.max_slabs * q.tiles_m * q.tiles_d * GQ_TILE * GQ_TILE);
  const long pitch = q.eff_chunk;
  GpWhitenArgs a;
  a.ldx = (long)ldx; a.D = D; a.M = M; a.Mp = q.Mp; a.Dp = q.Dp; a.Map = q.Map;
  a.Zimg = (const float4*)Zimg; a.centroid = centroid; a.znorm = znorm; a.W1img = (const float4*)W1img;
  a.s = s; a.inv_two_l2 = inv_two_l2; a.At = At; a.pitch = pitch;
  GpApplyArgs f;
  f.At = At; f.pitch = pitch; f.M = M; f.Mp = q.Mp; f.c = c;
  GpWeightArgs k;
  k.ldx = (long)ldx; k.D = D; k.M = M; k.Mp = q.Mp; k.Dp = q.Dp;
  k.Zimg = (const float4*)Zimg; k.centroid = centroid; k.znorm = znorm; k.s = s; k.inv_two_l2 = inv_two_l2;
  k.At = At; k.pitch = pitch; k.pc = pc; k.pd = pd;
  const int n_tiles = q.tiles_m * q.tiles_d;
  CGAT_PROF("gp_fit_grad", st);
  for (long base = 0; base < N; base += q.eff_chunk) {
    const long left = (long)N - base;
    const int rows = (int)(left < q.eff_chunk ? left : (long)q.eff_chunk);
    const int rows_p = (rows + 31) & ~31;
    const int row_tiles = rows_p / GP_ROWS;
    const int n_slabs = cdiv(rows_p, GQ_SLAB);
    const int first = base == 0 ? 1 : 0;
    a.X = X + base * (long)ldx; a.y_norm = y_norm + base; a.G = rows;
    gp_launch_whiten_rows(a, row_tiles, st);
    CGAT_LAUNCH_CHECK();
    f.G = rows; f.y_norm = y_norm + base;
    f.Fimg = (const float4*)G2img; f.upper = 0; f.g = g;
    hipLaunchKernelGGL(gp_apply_factor, dim3(row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    f.Fimg = (const float4*)W1timg; f.upper = 1; f.g = nullptr;
    hipLaunchKernelGGL(gp_apply_factor, dim3(row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    k.X = a.X; k.G = rows;
    hipLaunchKernelGGL(gp_weight_rows, dim3(row_tiles), dim3(GP_THREADS), 0, st, k);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_centre_rows, dim3(row_tiles, cdiv(D, 32)), dim3(256), 0, st, a.X, (long)ldx, rows, (int)D, centroid,
                       Xt, pitch);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_pair_slabs, dim3(n_tiles, n_slabs), dim3(GQ_THREADS), 0, st, At, Xt, pitch, (int)M, (int)D, rows_p,
                       part, q.tiles_d);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_grad_reduce_pairs, dim3(n_tiles, GQ_TILE * GQ_TILE / 256), dim3(256), 0, st, part, q.tiles_d, n_slabs,
                       (int)M, (int)D, P, first);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_grad_reduce_columns, dim3(cdiv(M, GQ_RC_COLS)), dim3(GQ_RC_COLS * GQ_RC_SEGS), 0, st, pc, pd,
                       row_tiles, q.Mp, (int)M, colsum, d2sum, first);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}
