// Sparse variational GP head on graph embeddings: the prediction side of the reference's screening flow,
// CGAT/gaussian_process.py:45-66 (ScaleKernel(RBFKernel), Constant/ZeroMean, whitened VariationalStrategy with a
// CholeskyVariationalDistribution) as evaluated at :247-268 (latent mean, confidence region mean +- 2 stddev, denorm).
//
//   k_x[m]   = s * exp(-max(|x - z_m|^2, 0) * inv_two_l2)                     M inducing points z_m, width D
//   mean_f   = c + k_x . a                          a  = L^-T m,  L = chol(K_zz + jitter I)
//   var_f    = max(s - |W1 k_x|^2 + |W2 k_x|^2, 0)  W1 = L^-1 (lower triangular),  W2 = L_S^T L^-1
//   pred     = mean_f * std + mean,   lower / upper = (mean_f -+ 2 sqrt(var_f)) * std + mean
//
// a, W1, W2, |z|^2 and the centroid of Z come from the caller (cgat_amd/gp.py computes them once per model in fp64);
// the centroid is subtracted from Z there and from x here, before squaring and multiplying.
//
// One launch, one 512-thread workgroup (8 waves, two per SIMD) per tile of 32 rows of X:
//   (a) S = Zc . Xc^T on the f32-input matrix cores (v_mfma_f32_32x32x2_f32, exact fp32 operands, fp32 accumulate): the
//       A operand is a 32-row chunk of Zc, read straight from the packed image (one 16-byte load per lane feeds four
//       MFMAs), the B operand is the X tile, centred and staged k-major in LDS 64 columns at a time.  Wave w owns the
//       chunks w, w + 8, ... of Z (at most four: M <= 1024).  The accumulator has the X row on the lane and the
//       inducing point in the registers, so norms + exp are applied in place and the tile's K^T[m][row] is written to
//       LDS without bank conflicts: 32 x 1024 x 4 B = 128 KiB of the CU's 160.  It never goes to HBM.
//   (b) U = F . K^T with F = [W1; W2] streamed from L2 / HBM through the same packed image, the K^T tile as the B
//       operand from LDS.  Again row-on-lane: each lane squares and sums its 16 registers per chunk.  W1 is lower
//       triangular, so its chunk pairs stop at the diagonal block and are dealt to the waves by gp_for_wave_pairs.
//       k_x . a is a VALU pass over the tile.
//   (c) the per-wave partial sums are added in a fixed order and 32 lanes write the outputs.
// No atomics: bitwise deterministic.  No workspace, no host synchronisation: capturable.
//
// The packed operand image, the tile constants, the operand record GpTile, the device code of (a) and of the products
// of (b) and the entries' argument check are in gp_tile.h, shared with csrc/gpfit.hip and csrc/gpgrad.hip.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "gp_tile.h"

struct GpArgs : GpTile {
  const float* avec;               // [Mp] a, zero padded
  const float4* Fimg;              // packed image of [W1; W2], each section [Mp, Mp], zero padded
  float c, tgt_mean, tgt_std;
  float *mean_f, *var_f, *pred, *lower, *upper;
};

// NB chunks c0 .. c0 + NB - 1 (those below c_end) of the packed factor image against the K^T tile, k8 in [0, k8_end);
// k8_end is a multiple of 4.  Returns this lane's sum of squares of the products.
template <int NB>
__device__ __forceinline__ float gp_factor_group(const float4* __restrict__ Fimg, const float* Kt, int c0, int c_end,
                                                 int nk8, int k8_end, int lane) {
  f32x16 acc[NB];
  gp_factor_products<NB>(Fimg, Kt, c0, c_end, nk8, k8_end, lane, acc);
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    if (c0 + j < c_end) {   // a chunk past the section was computed on a repeated image: not counted
#pragma unroll
      for (int t = 0; t < 16; ++t) ss = fmaf(acc[j][t], acc[j][t], ss);
    }
  }
  return ss;
}

__global__ __launch_bounds__(GP_THREADS) void gp_predict_kernel(GpArgs p) {
  // one LDS block: K^T tile [Mp][32] | staged X [64][33] | per-wave partial sums
  __shared__ __attribute__((aligned(16))) float lds[GP_ROWS * GP_MAX_M + GP_XK * GP_XP + 3 * 16 * GP_ROWS];
  float* Kt = lds;
  float* Xs = lds + GP_ROWS * GP_MAX_M;
  float* red = Xs + GP_XK * GP_XP;           // [3][16][32]: dot with a (16 parts), |W1 k|^2 and |W2 k|^2 (8 waves)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int nC = p.Mp >> 5;
  const long row0 = (long)blockIdx.x * GP_ROWS;

  // ---- (a) cross products, norms, exp ----
  gp_kernel_tile(p, row0, Kt, Xs);
  __syncthreads();

  // ---- (b) the dot with a (VALU), the two squared norms (matrix cores) ----
  {
    const int row = tid & 31, part = tid >> 5;
    float dot = 0.f;
    for (int m = part; m < p.M; m += 16) dot = fmaf(Kt[m * GP_ROWS + row], p.avec[m], dot);
    red[part * GP_ROWS + row] = dot;
  }
  float ss1 = 0.f, ss2 = 0.f;
  const int nk8 = p.Mp >> 3;
  {
    // W1, chunk pairs up to their diagonal block
    gp_for_wave_pairs(nC, wave, [&](int c0) {
      ss1 += gp_factor_group<2>(p.Fimg, Kt, c0, nC, nk8, min(nk8, 4 * (c0 + 2)), lane);
    });
    // W2, chunk quads over the full width
    const int n_quads = (nC + 3) >> 2;
    const float4* F2 = p.Fimg + (long)nC * nk8 * 64;
    for (int q = wave; q < n_quads; q += GP_WAVES) ss2 += gp_factor_group<4>(F2, Kt, 4 * q, nC, nk8, nk8, lane);
  }
  ss1 += __shfl_xor(ss1, 32);
  ss2 += __shfl_xor(ss2, 32);
  if (hi == 0) {
    red[(16 + wave) * GP_ROWS + r] = ss1;
    red[(32 + wave) * GP_ROWS + r] = ss2;
  }
  __syncthreads();

  // ---- (c) outputs ----
  if (tid < GP_ROWS && row0 + tid < p.G) {
    float dot = 0.f, q1 = 0.f, q2 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) dot += red[i * GP_ROWS + tid];
#pragma unroll
    for (int w = 0; w < GP_WAVES; ++w) {
      q1 += red[(16 + w) * GP_ROWS + tid];
      q2 += red[(32 + w) * GP_ROWS + tid];
    }
    const long g = row0 + tid;
    const float mf = p.c + dot;
    const float vf = fmaxf(p.s - q1 + q2, 0.f);
    p.mean_f[g] = mf;
    p.var_f[g] = vf;
    const float two_sd = 2.f * sqrtf(vf);
    if (p.pred) p.pred[g] = mf * p.tgt_std + p.tgt_mean;
    if (p.lower) p.lower[g] = (mf - two_sd) * p.tgt_std + p.tgt_mean;
    if (p.upper) p.upper[g] = (mf + two_sd) * p.tgt_std + p.tgt_mean;
  }
}

extern "C" size_t cgat_gp_predict_workspace_bytes(int32_t G, int32_t M, int32_t D) {
  (void)G; (void)M; (void)D;
  return 0;   // the tile of the cross-kernel matrix lives in LDS
}

extern "C" int cgat_gp_predict(const float* X, int64_t ldx, int32_t G, int32_t D, const float* Zimg, int32_t M,
                               const float* centroid, const float* znorm, const float* factors, float c, float s,
                               float inv_two_l2, float tgt_mean, float tgt_std, float* mean_f, float* var_f, float* pred,
                               float* lower, float* upper, void* ws, size_t ws_bytes, void* stream) {
  (void)ws; (void)ws_bytes;
  hipStream_t st = (hipStream_t)stream;
  CGAT_TRY(gp_check_entry("gp_predict", "G", G, 0, M, D,
                          "the fused kernel keeps a 32 x M tile of the cross-kernel matrix in LDS and supports", nullptr, ldx,
                          X && Zimg && centroid && znorm && factors && mean_f && var_f,
                          (uintptr_t)Zimg | (uintptr_t)factors, s, inv_two_l2));
  if (G == 0) return CGAT_OK;
  const GpTile t = gp_tile_operands(X, ldx, G, D, Zimg, M, centroid, znorm, s, inv_two_l2);
  const GpArgs a{t, factors, (const float4*)(factors + t.Mp), c, tgt_mean, tgt_std, mean_f, var_f, pred, lower, upper};
  CGAT_PROF("gp_predict", st);
  hipLaunchKernelGGL(gp_predict_kernel, dim3(cdiv(G, GP_ROWS)), dim3(GP_THREADS), 0, st, a);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
