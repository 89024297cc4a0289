// Device code shared by the sparse-GP kernels: csrc/gphead.hip (prediction), csrc/gpfit.hip (the fit
// statistics) and csrc/gpgrad.hip (the gradient of the bound).  All work on a tile of 32 rows of
// X with one 512-thread workgroup (8 waves, two per SIMD):
//   gp_distance_tile    max(|x_row - z_m|^2, 0) of the tile, handed to a functor
//   gp_kernel_tile      K^T[m][row] = s exp(-max(|x_row - z_m|^2, 0) inv_two_l2) of the tile, into LDS
//   gp_factor_products  NB 32-row chunks of a packed factor image times that K^T tile, on the f32-input matrix cores
// and gp_launch_whiten_rows (host, defined in csrc/gpfit.hip) enqueues the whitening kernel of 10c for 10d.
//
// Packed operand image of a row-major matrix P [R, Kd] (R a multiple of 32, Kd a multiple of 8):
//   img[((c * Kd/8 + k8) * 64 + lane) * 4 + q] = P[32 c + (lane & 31)][8 k8 + 2 q + (lane >> 5)]
// i.e. float4 number (c, k8, lane) holds lane's A operand of the four MFMA k-steps 8 k8 .. 8 k8 + 7 of chunk c.
#pragma once
#include <hip/hip_runtime.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GP_ROWS 32
#define GP_MAX_M 1024
#define GP_THREADS 512
#define GP_WAVES 8
#define GP_XK 64                   // columns of X staged per step (the packed image of Zc is padded to this)
#define GP_XP 33                   // pitch of the staged X tile: [k][row], conflict-free to write and to read

// Operands of gp_whiten_rows (csrc/gpfit.hip): A~^T = [W1 K^T; y~; 1; 0] of one chunk of rows.
struct GpWhitenArgs {
  const float* X;                  // already offset to the chunk's first row
  long ldx;
  int G, D, M;                     // G: rows of X left from the chunk's first row (tiles past it are zero filled)
  int Mp, Dp, Map;
  const float4* Zimg;
  const float* centroid;
  const float* znorm;
  const float4* W1img;             // packed image of W1 [Mp, Mp], lower triangular, zero padded
  const float* y_norm;             // offset like X
  float s, inv_two_l2;
  float* At;                       // [Map][pitch]
  long pitch;
};
// One workgroup per tile of 32 rows on `stream`; the caller follows it with CGAT_LAUNCH_CHECK().
void gp_launch_whiten_rows(const GpWhitenArgs& args, int n_tiles, hipStream_t stream);

// Inducing index of accumulator register t of chunk c on a lane of the upper (hi = 1) or lower half of the wave; the X
// row of the tile is lane & 31.
__device__ __forceinline__ int gp_acc_index(int c, int t, int hi) { return 32 * c + (t & 3) + 8 * (t >> 2) + 4 * hi; }

// NB chunks c0 .. c0 + NB - 1 (those below c_end) of the packed factor image against the K^T tile, k8 in [0, k8_end);
// k8_end is a multiple of 4.  acc[j] receives chunk c0 + j; a chunk past c_end is computed on a repeated image and must
// not be used.
template <int NB>
__device__ __forceinline__ void gp_factor_products(const float4* __restrict__ Fimg, const float* Kt, int c0, int c_end,
                                                   int nk8, int k8_end, int lane, f32x16 (&acc)[NB]) {
  const int r = lane & 31, hi = lane >> 5;
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[j][t] = 0.f;
  const float4* src[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) src[j] = Fimg + ((long)min(c0 + j, c_end - 1) * nk8) * 64 + lane;
  float4 cur[2][NB], nxt[2][NB];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int j = 0; j < NB; ++j) nxt[u][j] = cur[u][j] = src[j][(long)u * 64];
  for (int k8 = 0; k8 < k8_end; k8 += 2) {
    if (k8 + 2 < k8_end) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int j = 0; j < NB; ++j) nxt[u][j] = src[j][(long)(k8 + 2 + u) * 64];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float* kb = Kt + ((k8 + u) * 8 + hi) * GP_ROWS + r;
      const float b0 = kb[0], b1 = kb[2 * GP_ROWS], b2 = kb[4 * GP_ROWS], b3 = kb[6 * GP_ROWS];
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j].x, b0, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j].y, b1, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j].z, b2, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[u][j].w, b3, acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < NB; ++j) cur[u][j] = nxt[u][j];
  }
}

// Phase (a) of the kernels: cross products of the tile's rows (row0 ..) with every inducing point and the norms;
// store(m, d2) receives max(|x_r - z_m|^2, 0) of inducing index m < Mp and X row r = lane & 31 of the tile, once each, in
// wave-uniform control flow.  `p` carries X, ldx, G (rows of X), D, Mp, Dp, Zimg, centroid, znorm.  Xs [64][33] is LDS.
// Rows of the tile at or past G are staged as zeros (their distances are those of x = centroid: finite, and the caller's
// to discard).
template <class Args, class Store>
__device__ __forceinline__ void gp_distance_tile(const Args& p, long row0, float* Xs, Store store) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int nC = p.Mp >> 5;
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[j][t] = 0.f;
  float xn = 0.f;
  const int nk8 = p.Dp >> 3;
  for (int kc = 0; kc < p.Dp; kc += GP_XK) {
    __syncthreads();
    {
      const int k = tid & 63, kk = kc + k;
      const float cen = kk < p.D ? p.centroid[kk] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = (tid >> 6) + 8 * i;
        const long g = row0 + row;
        float v = 0.f;
        if (g < p.G && kk < p.D) v = p.X[g * p.ldx + kk] - cen;
        Xs[k * GP_XP + row] = v;
      }
    }
    __syncthreads();
    float b[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      b[i] = Xs[((i >> 2) * 8 + 2 * (i & 3) + hi) * GP_XP + r];
      xn = fmaf(b[i], b[i], xn);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = wave + GP_WAVES * j;
      if (c < nC) {
        const float4* src = p.Zimg + ((long)c * nk8 + (kc >> 3)) * 64 + lane;
        float4 a[8];
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) a[k8] = src[k8 * 64];
#pragma unroll
        for (int k8 = 0; k8 < 8; ++k8) {
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k8].x, b[4 * k8 + 0], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k8].y, b[4 * k8 + 1], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k8].z, b[4 * k8 + 2], acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[k8].w, b[4 * k8 + 3], acc[j], 0, 0, 0);
        }
      }
    }
  }
  xn += __shfl_xor(xn, 32);        // the two lane halves hold the even and the odd columns of row r
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = wave + GP_WAVES * j;
    if (c < nC) {
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int m = 32 * c + (t & 3) + 8 * (t >> 2) + 4 * hi;
        float d2 = xn + p.znorm[m] - 2.f * acc[j][t];
        d2 = fmaxf(d2, 0.f);
        store(m, d2);
      }
    }
  }
}

// K^T[m][row] = s exp(-d2 inv_two_l2) of the tile into Kt [Mp][32] (LDS), 0 for m >= M; `p` carries M, s, inv_two_l2 as
// well.  The caller synchronises before it reads Kt.
template <class Args>
__device__ __forceinline__ void gp_kernel_tile(const Args& p, long row0, float* Kt, float* Xs) {
  const int r = threadIdx.x & 31;
  gp_distance_tile(p, row0, Xs, [&](int m, float d2) {
    const float kv = p.s * expf(-d2 * p.inv_two_l2);
    Kt[m * GP_ROWS + r] = m < p.M ? kv : 0.f;
  });
}
