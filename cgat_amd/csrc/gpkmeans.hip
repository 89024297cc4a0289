// One Lloyd step of k-means over the embeddings, for the inducing points of the sparse-GP head: the reference
// starts Z from a random batch of training rows (CGAT/gaussian_process.py:208-226); this is the step that moves such a
// start to the centres of the data.  Per row n of X, with the centres Z as the fit's phase (a) reads them (packed image of
// Z - centroid, |z_m - centroid|^2):
//
//   a_n = argmin_{m < M} max(|x_n - z_m|^2, 0)   (a tie goes to the smaller m)        d_n = that minimum
//   counts_m = #{n : a_n = m}      wss_m = sum_{a_n = m} d_n      P_m = sum_{a_n = m} (x_n - centroid)
//
// so the new centre is centroid + P_m / counts_m (cgat_amd/gp.py, fp64 on the host) and sum(wss) is the inertia of the
// assignment.  Per chunk of rows, on the caller's stream:
//
//   gp_assign_rows      phase (a) (gp_distance_tile, gp_tile.h) with an argmin as the functor: no tile of K^T, 10.5 KB of
//                       LDS.  Writes a_n, the one-hot columns R^T[m][n] = 1[a_n = m] into the chunk buffer and one fp32
//                       partial per (tile, m) of the count (exact: at most 32) and of d, added in row order.
//   gp_launch_row_sums  (csrc/gpgrad.hip) the sums that end a chunk of the gradient pass, with the one-hot R: P = R^T Xc
//                       over slabs of 1024 rows on the f32-input matrix cores (every product is 1 x or 0 x, so a slab's
//                       partial is the fp32 sum of its members), counts and wss from the partials, all added in fp64 in a
//                       fixed order; the first chunk stores, later chunks add.
// No atomics: bitwise deterministic.  No allocation, no host synchronisation; the only host loop enqueues launches.
#include <climits>
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_slab.h"

struct GpAssignArgs : GpTile {
  int32_t* assign;                 // offset to the chunk's first row, like X
  float* Rt;                       // [>= Mp][pitch]: the one-hot columns of the tile's 32 rows, rows < Mp
  long pitch;
  float* pc;                       // [tile][Mp]: rows of the tile assigned to m
  float* pd;                       // [tile][Mp]: sum of their minimum distances
};

// (d, m) <- the smaller of (d, m) and (od, om): by distance, then by index.
__device__ __forceinline__ void gk_take_min(float& d, int& m, float od, int om) {
  if (od < d || (od == d && om < m)) {
    d = od;
    m = om;
  }
}

__global__ __launch_bounds__(GP_THREADS) void gp_assign_rows(GpAssignArgs p) {
  __shared__ float Xs[GP_XK * GP_XP];
  __shared__ float wave_d[GP_WAVES][GP_ROWS];
  __shared__ int wave_m[GP_WAVES][GP_ROWS];
  __shared__ float row_d[GP_ROWS];
  __shared__ int row_m[GP_ROWS];                   // -1: a row at or past G
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const long row0 = (long)blockIdx.x * GP_ROWS;

  // A padded centre (m >= M) has a zero image and znorm 0: its "distance" is |x - centroid|^2 and must never compete.
  float bd = INFINITY;
  int bm = INT_MAX;
  gp_distance_tile(p, row0, Xs, [&](int m, float d2) {
    if (m < p.M) gk_take_min(bd, bm, d2, m);
  });
  gk_take_min(bd, bm, __shfl_xor(bd, 32), __shfl_xor(bm, 32));      // the two lane halves hold different m of row r
  if (hi == 0) {
    wave_d[wave][r] = bd;
    wave_m[wave][r] = bm;
  }
  __syncthreads();
  if (tid < GP_ROWS) {
    bd = wave_d[0][tid];
    bm = wave_m[0][tid];
#pragma unroll
    for (int w = 1; w < GP_WAVES; ++w) gk_take_min(bd, bm, wave_d[w][tid], wave_m[w][tid]);
    const bool live = row0 + tid < p.G;
    row_d[tid] = live ? bd : 0.f;
    row_m[tid] = live ? bm : -1;
    if (live) p.assign[row0 + tid] = bm;
  }
  __syncthreads();

  // R^T of the tile: thread -> (m, four columns), a wave stores eight whole 128-byte rows per instruction
  for (int i = tid; i < p.Mp * (GP_ROWS / 4); i += GP_THREADS) {
    const int m = i >> 3, c4 = (i & 7) * 4;
    const float4 v = make_float4(row_m[c4] == m ? 1.f : 0.f, row_m[c4 + 1] == m ? 1.f : 0.f, row_m[c4 + 2] == m ? 1.f : 0.f,
                                 row_m[c4 + 3] == m ? 1.f : 0.f);
    *(float4*)(p.Rt + (long)m * p.pitch + row0 + c4) = v;
  }
  float* pc = p.pc + (long)blockIdx.x * p.Mp;
  float* pd = p.pd + (long)blockIdx.x * p.Mp;
  for (int m = tid; m < p.Mp; m += GP_THREADS) {
    float cnt = 0.f, sum = 0.f;
#pragma unroll
    for (int i = 0; i < GP_ROWS; ++i) {
      if (row_m[i] == m) {
        cnt += 1.f;
        sum += row_d[i];
      }
    }
    pc[m] = cnt;
    pd[m] = sum;
  }
}

// ---- host ----
extern "C" size_t cgat_gp_kmeans_step_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows) {
  return cgat_gp_fit_grad_workspace_bytes(N, M, D, chunk_rows);
}

extern "C" int cgat_gp_kmeans_step(const float* X, int64_t ldx, int32_t N, int32_t D, const float* Zimg, int32_t M,
                                   const float* centroid, const float* znorm, int32_t chunk_rows, int32_t* assign,
                                   double* counts, double* wss, double* P, void* ws, size_t ws_bytes, void* stream) {
  const char* name = "gp_kmeans_step";
  hipStream_t st = (hipStream_t)stream;
  CGAT_TRY(gp_check_entry(name, "N", N, 1, M, D, "the tile of distances and the chunk buffer are those of the fit, which supports",
                          &chunk_rows, ldx, X && Zimg && centroid && znorm && assign && counts && wss && P, (uintptr_t)Zimg,
                          1.f, 1.f));
  CGAT_TRY(gp_check_workspace(name, ws, ws_bytes, cgat_gp_kmeans_step_workspace_bytes(N, M, D, chunk_rows)));
  GpChunks ch(N, M, D, chunk_rows);
  const GpRowSumsWorkspace w(ch, M, D, ws, ws_bytes);
  GpAssignArgs a{gp_tile_operands(X, ldx, 0, D, Zimg, M, centroid, znorm, 1.f, 1.f), assign, w.At, (long)ch.eff_chunk, w.pc,
                 w.pd};
  CGAT_PROF(name, st);
  while (ch.next()) {
    ch.place(a, X);
    a.assign = assign + ch.base;
    hipLaunchKernelGGL(gp_assign_rows, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, a);
    CGAT_LAUNCH_CHECK();
    CGAT_TRY(gp_launch_row_sums(w, ch, a.X, (long)ldx, M, D, centroid, counts, wss, P, st));
  }
  return CGAT_OK;
}
