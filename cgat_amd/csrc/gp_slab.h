// Products over a chunk of rows, shared by csrc/gpfit.hip (A~^T A~) and csrc/gpgrad.hip (R^T Xc):
//   gp_slab_product  one 128 x 128 tile of A B^T over one slab of 1024 rows, on the f32-input matrix cores
//   gp_slab_reduce   one element of such a tile: its slabs added in slab order in fp64, stored or added to the result
//   GpChunks         (host) the walk over the chunks of rows and what the workspace of a chunk holds
//   GpRowSumsWorkspace, gp_launch_row_sums  (host) the workspace of a chunk of 10d and the launches that end it: R^T Xc and
//                    the column sums, which csrc/gpkmeans.hip runs with a one-hot R
// Both operands are inducing-major, [rows][pitch] with the chunk's rows along the pitch, as gp_whiten_rows stores A~^T.
#pragma once
#include "gp_tile.h"

#define GS_TILE 128                // output tile of the product
#define GS_KS 32                   // rows of the chunk per staged panel
#define GS_PITCH 36                // floats per panel row in LDS: 16-byte reads without bank conflicts
#define GS_SLAB 1024               // rows of the chunk per partial
#define GS_THREADS 256

// out [128][128] = A[i0 .. i0 + 127] . B[j0 .. j0 + 127]^T over the columns n0 .. min(n0 + 1024, rows_p) - 1 of both
// (rows_p a multiple of 32); rows of A at or past rows_a and of B at or past rows_b count as zero.  One workgroup of 256
// threads, each wave a 64 x 64 quadrant (gp_slab_quadrant) as 2 x 2 accumulators; a wave that is not `active` helps to
// stage and neither multiplies nor stores.  Both operands are staged as 128 x 32 panels in LDS with the next panel
// prefetched into registers.  A lane's 16-byte read holds four k-steps: k-step q of a group of 8 rows pairs rows q and
// 4 + q, the same pairing on both operands.
__device__ __forceinline__ void gp_slab_quadrant(int& wi, int& wj) {
  const int wave = threadIdx.x >> 6;
  wi = 64 * (wave >> 1);
  wj = 64 * (wave & 1);
}

__device__ __forceinline__ void gp_slab_product(const float* __restrict__ A, int rows_a, const float* __restrict__ B,
                                                int rows_b, long pitch, int i0, int j0, int n0, int rows_p, bool active,
                                                float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float panel[2][GS_TILE * GS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int r = lane & 31, hi = lane >> 5;
  const int n_stage = (min(GS_SLAB, rows_p - n0)) / GS_KS;
  int wi, wj;
  gp_slab_quadrant(wi, wj);

  // global -> registers: thread covers float4 (row = tid / 8 + 32 u, columns 4 (tid % 8) ..) of each panel
  const int lrow = tid >> 3, lc4 = (tid & 7) * 4;
  float4 gA[4], gB[4];
  auto fetch = [&](int stage) {
    const long col = (long)n0 + (long)stage * GS_KS + lc4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ra = i0 + lrow + 32 * u, rb = j0 + lrow + 32 * u;
      gA[u] = ra < rows_a ? *(const float4*)(A + (long)ra * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
      gB[u] = rb < rows_b ? *(const float4*)(B + (long)rb * pitch + col) : make_float4(0.f, 0.f, 0.f, 0.f);
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
      *(float4*)(panel[0] + (lrow + 32 * u) * GS_PITCH + lc4) = gA[u];
      *(float4*)(panel[1] + (lrow + 32 * u) * GS_PITCH + lc4) = gB[u];
    }
    __syncthreads();
    if (stage + 1 < n_stage) fetch(stage + 1);
    if (active) {
#pragma unroll
      for (int k8 = 0; k8 < GS_KS / 8; ++k8) {
        float4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          fa[a] = *(const float4*)(panel[0] + (wi + 32 * a + r) * GS_PITCH + 8 * k8 + 4 * hi);
          fb[a] = *(const float4*)(panel[1] + (wj + 32 * a + r) * GS_PITCH + 8 * k8 + 4 * hi);
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
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int i = wi + gp_acc_index(a, t, hi), j = wj + 32 * b + r;
          out[i * GS_TILE + j] = acc[a][b][t];
        }
  }
}

// Element e of output tile blockIdx.x of part [slab][tile][128][128]: the n_slabs partials added in slab order; the first
// chunk stores the sum to *dst, later chunks add it.  Returns what *dst now holds.
__device__ __forceinline__ double gp_slab_reduce(const float* __restrict__ part, int n_tiles, int n_slabs, int e,
                                                 double* __restrict__ dst, int first) {
  const float* src = part + (long)blockIdx.x * (GS_TILE * GS_TILE) + e;
  double sum = 0.0;
  for (int sl = 0; sl < n_slabs; ++sl) sum += (double)src[(long)sl * n_tiles * (GS_TILE * GS_TILE)];
  if (!first) sum += *dst;
  *dst = sum;
  return sum;
}

// ---- host ----
// The rows [0, N) in chunks of eff_chunk rows (chunk_rows, or all the rows rounded up to 32 where that is less).  What a
// call fixes is set by the constructor; next() steps to the following chunk and is false after the last one.
struct GpChunks {
  int N, Mp, Dp, Map, eff_chunk, max_slabs;                // Map: M + 2 (A~ = [a, y~, 1]) rounded up to 32
  long base = 0;                                           // first row of the chunk
  int rows = 0, rows_p, row_tiles, n_slabs, first, last;   // rows_p: rows rounded up to 32; row_tiles: rows_p / 32

  // what cgat_gp_fit_*_workspace_bytes refuse with 0 and gp_check_entry with a message
  static bool fits(int N, int M, int D, int chunk_rows) {
    return N >= 1 && M >= 1 && M <= GP_MAX_M && D >= 1 && chunk_rows >= 32 && (chunk_rows & 31) == 0;
  }
  GpChunks(int N_, int M, int D, int chunk_rows) : N(N_), Mp(gp_pad_m(M)), Dp(gp_pad_d(D)), Map(gp_pad_m(M + 2)) {
    const long n_p = ((long)N + 31) & ~31L;                // a chunk never holds more than the rows there are
    eff_chunk = (int)(n_p < (long)chunk_rows ? n_p : (long)chunk_rows);
    max_slabs = cdiv(eff_chunk, GS_SLAB);
  }
  size_t at_elems() const { return (size_t)Map * eff_chunk; }   // the chunk buffer [Map][eff_chunk]
  bool next() {
    base += rows ? eff_chunk : 0;                          // rows == 0: before the first chunk
    if (base >= N) return false;
    const long left = (long)N - base;
    rows = (int)(left < eff_chunk ? left : (long)eff_chunk);
    rows_p = (rows + 31) & ~31;
    row_tiles = rows_p / GP_ROWS;
    n_slabs = cdiv(rows_p, GS_SLAB);
    first = base == 0 ? 1 : 0;
    last = base + eff_chunk >= N ? 1 : 0;
    return true;
  }
  // the operands of phase (a) at the current chunk
  void place(GpTile& t, const float* X) const {
    t.X = X + base * t.ldx;
    t.G = rows;
  }
};

// The workspace of a chunk of the gradient pass, which the k-means step (csrc/gpkmeans.hip, 10f) lays out
// the same way: the chunk buffer [Map][eff_chunk], Xc^T [D][eff_chunk], the per-tile partials pc, pd [eff_chunk / 32][Mp]
// and the slab partials of R^T Xc [max_slabs][tiles of (M, D)][128][128].
struct GpRowSumsWorkspace {
  float *At, *Xt, *pc, *pd, *part;
  static int tiles(int M, int D) { return cdiv(M, GS_TILE) * cdiv(D, GS_TILE); }
  static size_t xt_elems(const GpChunks& c, int D) { return (size_t)D * c.eff_chunk; }
  static size_t col_elems(const GpChunks& c) { return (size_t)(c.eff_chunk / GP_ROWS) * c.Mp; }
  static size_t part_elems(const GpChunks& c, int M, int D) {
    return (size_t)c.max_slabs * tiles(M, D) * GS_TILE * GS_TILE;
  }
  static size_t bytes(const GpChunks& c, int M, int D) {
    return ws_round(c.at_elems(), sizeof(float)) + ws_round(xt_elems(c, D), sizeof(float)) +
           2 * ws_round(col_elems(c), sizeof(float)) + ws_round(part_elems(c, M, D), sizeof(float));
  }
  GpRowSumsWorkspace(const GpChunks& c, int M, int D, void* ws, size_t ws_bytes) {
    Workspace w(ws, ws_bytes);
    At = w.take<float>(c.at_elems());
    Xt = w.take<float>(xt_elems(c, D));
    pc = w.take<float>(col_elems(c));
    pd = w.take<float>(col_elems(c));
    part = w.take<float>(part_elems(c, M, D));
  }
};

// The sums over the rows of the current chunk `ch` that end a chunk of both passes (defined in csrc/gpgrad.hip), on
// `stream`: with R^T = rows < M of w.At and the partials w.pc, w.pd [ch.row_tiles][Mp] the caller's kernels have written,
//   gp_centre_rows, gp_pair_slabs, gp_grad_reduce_pairs   P [M][D] (+)= R^T (X - centroid) over the chunk's rows
//   gp_grad_reduce_columns                                colsum, d2sum [M] (+)= the tiles of pc, pd added in tile order
// fp64, stored by the first chunk and added to by the later ones.  `X`: the chunk's first row.  Returns a CGAT_* code.
int gp_launch_row_sums(const GpRowSumsWorkspace& w, const GpChunks& ch, const float* X, long ldx, int M, int D,
                       const float* centroid, double* colsum, double* d2sum, double* P, hipStream_t stream);

static inline int gp_check_workspace(const char* name, const void* ws, size_t ws_bytes, size_t needed) {
  if (!ws || ws_bytes < needed) {
    cgat_set_error("%s: workspace of %zu bytes, %zu needed", name, ws ? ws_bytes : (size_t)0, needed);
    return CGAT_ERR_WORKSPACE;
  }
  CGAT_CHECK_ARG(((uintptr_t)ws & 15) == 0, "%s: the workspace needs 16-byte alignment", name);
  return CGAT_OK;
}
