// Derivative of the sparse-GP head's prediction in its input: the backward of csrc/gphead.hip, the
// reference's CGAT/gaussian_process.py:247-268 made differentiable in the embeddings.  With alpha = W1 k_x, S = L_S L_S^T and
// a = W1^T m the latent distribution of 10b is
//
//   mean_f = c + alpha . m            var_f = s + alpha^T (S - I) alpha
//
// so with the upstream gradients gm = dL/dmean_f and gv = dL/dvar_f of a row, G2 = 2 (S - I) (symmetric, from the host
// in fp64) and k = s exp(-max(|x - z_m|^2, 0) inv_two_l2)
//
//   q = gv G2 alpha + gm m,    u = W1^T q = dL/dk,    r_m = u_m k_m,    rho = sum_m r_m
//   dL/dx = (sum_m r_m (z_m - centroid) - rho (x - centroid)) 2 inv_two_l2
//
// which is the chain of the bound's gradient (csrc/gpgrad.hip) with a per-row coefficient on the G2
// product and without any sum over the rows.  Three factors, never W1^T G2 W1 as one matrix (csrc/gpgrad.hip says why).
// alpha, q and u pass through ONE chunk buffer in the workspace, inducing-major [Ma_p][pitch] as gp_whiten_rows stores it,
// each overwriting the one before it.  Per chunk of rows, on the caller's stream:
//
//   gp_whiten_rows    (csrc/gpfit.hip) rows 0 .. M - 1 of the buffer = alpha.  Not launched where gv is null: q = gm m then.
//   gp_back_apply     buffer <- gv[row] (G2 x buffer) + gm[row] m, then buffer <- W1^T x buffer (upper triangular): the
//                     tile [Mp][32] in LDS, gp_factor_products on the f32-input matrix cores, as gp_apply_factor of
//                     csrc/gpgrad.hip, which stays as it is (no multiply is added on the bound's path)
//   gp_back_input     phase (a) again (gp_distance_tile): r = u k with d2 recomputed, written into the tile in LDS and not
//                     to the buffer; after one barrier rho as column sums in a fixed order and the product with the image
//                     of Zc^T (gp_input_tile, gp_tile.h: the product and the rounding sequence of gp_input_rows).  One
//                     launch in place of gp_weight_rows + gp_input_rows: the tile of r is neither stored nor read back.
// No atomics: bitwise deterministic, and a row's dX does not depend on chunk_rows.  No allocation, no host
// synchronisation; the only host loop enqueues launches.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_slab.h"

struct GpBackApplyArgs {
  float* At;                       // [Map][pitch]; rows < M of the tile's 32 columns are replaced
  long pitch;
  int G, M, Mp;                    // G: rows of the chunk (columns at or past it are written as 0)
  const float4* Fimg;              // packed image of F [Mp, Mp], zero padded
  int upper;                       // F is upper triangular (W1^T): no coefficients, out = F x buffer
  const float* m;                  // [M] (the G2 step)
  const float* gm;                 // [rows of the chunk] or null: + m[i] gm[col]
  const float* gv;                 // [rows of the chunk] or null: the product times gv[col]; null: no product, no read of At
};

__global__ __launch_bounds__(GP_THREADS) void gp_back_apply(GpBackApplyArgs p) {
  __shared__ __attribute__((aligned(16))) float Bt[GP_ROWS * GP_MAX_M];      // the tile [Mp][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int nC = p.Mp >> 5, nk8 = p.Mp >> 3;
  const long row0 = (long)blockIdx.x * GP_ROWS;
  const long col = row0 + r;
  const bool live = col < p.G;
  const bool product = p.upper || p.gv;
  if (product) {
    // rows m >= M of the buffer are not this pass's: loaded as zero
    for (int i = tid; i < p.Mp * GP_ROWS; i += GP_THREADS)
      Bt[i] = (i >> 5) < p.M ? p.At[(long)(i >> 5) * p.pitch + row0 + (i & 31)] : 0.f;
  }
  __syncthreads();
  const float cv = !p.upper && p.gv && live ? p.gv[col] : 0.f;
  const float cm = !p.upper && p.gm && live ? p.gm[col] : 0.f;
  gp_for_wave_pairs(nC, wave, [&](int c0) {
    const int k8_0 = p.upper ? 4 * c0 : 0;
    f32x16 acc[2];
    if (product) gp_factor_products<2>(p.Fimg + (long)k8_0 * 64, Bt + k8_0 * 8 * GP_ROWS, c0, nC, nk8, nk8 - k8_0, lane, acc);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (c0 + j < nC) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const int mi = gp_acc_index(c0 + j, t, hi);
          if (mi < p.M) {
            float v;
            if (p.upper) {
              v = acc[j][t];
            } else {
              v = p.gv ? cv * acc[j][t] : 0.f;
              if (p.gm) v = fmaf(p.m[mi], cm, v);
            }
            p.At[(long)mi * p.pitch + col] = live ? v : 0.f;
          }
        }
      }
    }
  });
}

struct GpBackInputArgs : GpTile {  // X, G: the chunk's (GpChunks::place)
  const float* At;                 // [Map][pitch]: u in rows < M
  long pitch;
  const float4* Ztimg;             // packed image of Zc^T [D rounded up to 32, Mp], zero padded
  float* dX;                       // offset to the chunk's first row, like X
  long lddx;
  int vec_x, vec_dx;               // 16-byte loads of X / stores of dX are aligned
};

__global__ __launch_bounds__(GP_THREADS) void gp_back_input(GpBackInputArgs p) {
  // one LDS block: the tile of r [Mp][32] | staged X [64][33] | [16][32] partial column sums
  __shared__ __attribute__((aligned(16))) float lds[GP_ROWS * GP_MAX_M + GP_XK * GP_XP + GP_THREADS];
  float* Rt = lds;
  float* Xs = lds + GP_ROWS * GP_MAX_M;
  float* part = Xs + GP_XK * GP_XP;
  const int tid = threadIdx.x, r = tid & 31;
  const long row0 = (long)blockIdx.x * GP_ROWS;
  const long col = row0 + r;
  const bool live = col < p.G;
  gp_distance_tile(p, row0, Xs, [&](int m, float d2) {
    float rv = 0.f;
    if (m < p.M && live) rv = p.At[(long)m * p.pitch + col] * (p.s * expf(-d2 * p.inv_two_l2));
    Rt[m * GP_ROWS + r] = rv;
  });
  __syncthreads();
  // thread tid adds column tid & 31 of rows tid >> 5, + 16, ...: gp_input_rows' partial sums, in its order
  float ps = 0.f;
  for (int i = tid; i < p.Mp * GP_ROWS; i += GP_THREADS) ps += Rt[i];
  part[tid] = ps;
  __syncthreads();
  float rho = 0.f;
#pragma unroll
  for (int j = 0; j < GP_THREADS / GP_ROWS; ++j) rho += part[j * GP_ROWS + r];     // the 16 partials in a fixed order
  gp_input_tile(p, Rt, rho, row0);
}

// ---- host ----
extern "C" size_t cgat_gp_predict_backward_workspace_bytes(int32_t G, int32_t M, int32_t D, int32_t chunk_rows) {
  if (!GpChunks::fits(G, M, D, chunk_rows)) return 0;
  return ws_round(GpChunks(G, M, D, chunk_rows).at_elems(), sizeof(float));       // the chunk buffer alone
}

extern "C" int cgat_gp_predict_backward(const float* X, int64_t ldx, int32_t G, int32_t D, const float* Zimg, int32_t M,
                                        const float* centroid, const float* znorm, const float* W1img,
                                        const float* W1timg, const float* G2img, const float* m, const float* gm,
                                        const float* gv, float s, float inv_two_l2, int32_t chunk_rows,
                                        const float* Ztimg, float* dX, int64_t lddx, void* ws, size_t ws_bytes,
                                        void* stream) {
  const char* name = "gp_predict_backward";
  hipStream_t st = (hipStream_t)stream;
  CGAT_TRY(gp_check_entry(
      name, "G", G, 1, M, D, "the kernels keep a 32 x M tile of the cross-kernel matrix in LDS and support", &chunk_rows,
      ldx, X && Zimg && centroid && znorm && W1img && W1timg && G2img && m && (gm || gv) && Ztimg && dX,
      (uintptr_t)Zimg | (uintptr_t)W1img | (uintptr_t)W1timg | (uintptr_t)G2img | (uintptr_t)Ztimg, s, inv_two_l2));
  CGAT_CHECK_ARG(lddx >= D, "%s: lddx = %ld < D = %d", name, (long)lddx, D);
  CGAT_TRY(gp_check_workspace(name, ws, ws_bytes, cgat_gp_predict_backward_workspace_bytes(G, M, D, chunk_rows)));
  GpChunks ch(G, M, D, chunk_rows);
  float* At = (float*)ws;
  const long pitch = ch.eff_chunk;
  const GpTile tile = gp_tile_operands(X, ldx, 0, D, Zimg, M, centroid, znorm, s, inv_two_l2);
  GpWhitenArgs a{tile, ch.Map, (const float4*)W1img, nullptr, At, pitch};
  GpBackApplyArgs f{At, pitch, 0, (int)M, ch.Mp, nullptr, 0, m, nullptr, nullptr};
  GpBackInputArgs in{tile, At, pitch, (const float4*)Ztimg, dX, (long)lddx,
                     (((uintptr_t)X & 15) == 0 && (ldx & 3) == 0) ? 1 : 0,
                     (((uintptr_t)dX & 15) == 0 && (lddx & 3) == 0) ? 1 : 0};
  CGAT_PROF(name, st);
  while (ch.next()) {
    ch.place(a, X);
    ch.place(in, X);
    in.dX = dX + ch.base * lddx;
    f.G = ch.rows;
    f.gm = gm ? gm + ch.base : nullptr;
    f.gv = gv ? gv + ch.base : nullptr;
    if (gv) {
      a.y_norm = gv + ch.base;       // row M of the buffer, which gp_whiten_rows fills from it, is not read by this pass
      gp_launch_whiten_rows(a, ch.row_tiles, st);
      CGAT_LAUNCH_CHECK();
    }
    f.Fimg = (const float4*)G2img; f.upper = 0;
    hipLaunchKernelGGL(gp_back_apply, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    f.Fimg = (const float4*)W1timg; f.upper = 1;
    hipLaunchKernelGGL(gp_back_apply, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, f);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(gp_back_input, dim3(ch.row_tiles), dim3(GP_THREADS), 0, st, in);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}
