// Device and host code shared by the sparse-GP entries: csrc/gphead.hip (prediction), csrc/gpfit.hip (the fit
// statistics), csrc/gpgrad.hip (the gradient of the bound), csrc/gpkmeans.hip (the k-means step
// for the inducing points) and csrc/gpback.hip (the backward of the prediction).  All work on a
// tile of 32 rows of X with one 512-thread workgroup (8 waves, two per SIMD):
//   GpTile              the operands of phase (a), filled by gp_tile_operands; the kernels that run it derive theirs from it
//   gp_distance_tile    max(|x_row - z_m|^2, 0) of the tile, handed to a functor
//   gp_kernel_tile      K^T[m][row] = s exp(-max(|x_row - z_m|^2, 0) inv_two_l2) of the tile, into LDS
//   gp_factor_products  NB 32-row chunks of a packed factor image times that K^T tile, on the f32-input matrix cores
//   gp_for_wave_pairs   the chunk pairs of a triangular factor that a wave owns
//   gp_input_tile       dX of the tile's rows from a tile of r in LDS: the product with Zc^T and the stores (10e, 10g)
//   gp_check_entry      (host) the argument checks the C entries share
// and gp_launch_whiten_rows (host, defined in csrc/gpfit.hip) enqueues the whitening kernel of 10c for 10d.  The slab
// products over a chunk of rows and the chunk walk of 10c and 10d are in gp_slab.h.
//
// Packed operand image of a row-major matrix P [R, Kd] (R a multiple of 32, Kd a multiple of 8):
//   img[((c * Kd/8 + k8) * 64 + lane) * 4 + q] = P[32 c + (lane & 31)][8 k8 + 2 q + (lane >> 5)]
// i.e. float4 number (c, k8, lane) holds lane's A operand of the four MFMA k-steps 8 k8 .. 8 k8 + 7 of chunk c.
#pragma once
#include <hip/hip_runtime.h>
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define GP_ROWS 32
#define GP_MAX_M 1024
#define GP_THREADS 512
#define GP_WAVES 8
#define GP_XK 64                   // columns of X staged per step (the packed image of Zc is padded to this)
#define GP_XP 33                   // pitch of the staged X tile: [k][row], conflict-free to write and to read

// What gp_distance_tile and gp_kernel_tile read.
struct GpTile {
  const float* X;                  // offset to the first row the launch covers
  long ldx;
  int G, D, M;                     // G: rows of X from that row on (tiles past them are zero filled)
  int Mp, Dp;                      // M rounded up to 32, D rounded up to 64
  const float4* Zimg;              // packed image of Zc [Mp, Dp], zero padded
  const float* centroid;           // [D]
  const float* znorm;              // [Mp] |z_m - centroid|^2, zero padded
  float s, inv_two_l2;
};

static inline int gp_pad_m(int M) { return (M + 31) & ~31; }
static inline int gp_pad_d(int D) { return (D + GP_XK - 1) & ~(GP_XK - 1); }

static inline GpTile gp_tile_operands(const float* X, int64_t ldx, int G, int D, const float* Zimg, int M,
                                      const float* centroid, const float* znorm, float s, float inv_two_l2) {
  return GpTile{X, (long)ldx, G, D, M, gp_pad_m(M), gp_pad_d(D), (const float4*)Zimg, centroid, znorm, s, inv_two_l2};
}

// The checks the entries share, in the order they report: the shape (`rows_name` = `rows` >= min_rows), the refusal
// of M > GP_MAX_M (`lds_clause`: who keeps the tile in LDS), chunk_rows where the entry has chunks (null otherwise), then,
// unless the call is empty, the row stride, `operands` (every pointer the entry needs is there), `images` (the packed
// images' addresses or-ed together) and the kernel's parameters.
static inline int gp_check_entry(const char* name, const char* rows_name, int rows, int min_rows, int M, int D,
                                 const char* lds_clause, const int32_t* chunk_rows, int64_t ldx, bool operands,
                                 uintptr_t images, float s, float inv_two_l2) {
  CGAT_CHECK_ARG(rows >= min_rows && M >= 1 && D >= 1, "%s: %s = %d, M = %d, D = %d", name, rows_name, rows, M, D);
  if (M > GP_MAX_M) {
    cgat_set_error("%s: M = %d inducing points; %s M <= %d", name, M, lds_clause, GP_MAX_M);
    return CGAT_ERR_UNSUPPORTED;
  }
  CGAT_CHECK_ARG(!chunk_rows || (*chunk_rows >= 32 && (*chunk_rows & 31) == 0),
                 "%s: chunk_rows = %d is not a positive multiple of 32", name, (int)*chunk_rows);
  if (rows == 0) return CGAT_OK;
  CGAT_CHECK_ARG(ldx >= D, "%s: ldx = %ld < D = %d", name, (long)ldx, D);
  CGAT_CHECK_ARG(operands, "%s: null operand", name);
  CGAT_CHECK_ARG((images & 15) == 0, "%s: the packed images need 16-byte alignment", name);
  CGAT_CHECK_ARG(s >= 0.f && inv_two_l2 > 0.f, "%s: outputscale / lengthscale out of range", name);
  return CGAT_OK;
}

// Operands of gp_whiten_rows (csrc/gpfit.hip): A~^T = [W1 K^T; y~; 1; 0] of one chunk of rows.
struct GpWhitenArgs : GpTile {
  int Map;
  const float4* W1img;             // packed image of W1 [Mp, Mp], lower triangular, zero padded
  const float* y_norm;             // offset like X
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

// The chunk pairs of a triangular factor [Mp, Mp] (nC = Mp / 32 chunks): pair q covers chunks 2 q and 2 q + 1, whose
// column blocks stop (lower triangle) or start (upper) at their diagonal, so the work of a pair grows with q.  Pairs q and
// 15 - q of every sixteen go to the same wave, which balances the triangle over the 8 waves.  body(c0) receives the first
// chunk c0 = 2 q of each pair `wave` owns, in that order.
template <class Body>
__device__ __forceinline__ void gp_for_wave_pairs(int nC, int wave, Body body) {
  const int n_pairs = (nC + 1) >> 1;
  for (int base = 0; base < n_pairs; base += 16) {
    const int q[2] = {base + wave, base + 15 - wave};
#pragma unroll
    for (int i = 0; i < 2; ++i)
      if (q[i] < n_pairs) body(2 * q[i]);
  }
}

// Phase (a) of the kernels: cross products of the tile's rows (row0 ..) with every inducing point and the norms;
// store(m, d2) receives max(|x_r - z_m|^2, 0) of inducing index m < Mp and X row r = lane & 31 of the tile, once each, in
// wave-uniform control flow.  `p` is a GpTile or derives from one.  Xs [64][33] is LDS.
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
        const int m = gp_acc_index(c, t, hi);
        float d2 = xn + p.znorm[m] - 2.f * acc[j][t];
        d2 = fmaxf(d2, 0.f);
        store(m, d2);
      }
    }
  }
}

// dX[row][d] = (sum_m r[m][row] zc[m][d] - rho (x[row][d] - centroid[d])) 2 inv_two_l2 of the tile's rows row0 .. that are
// below p.G, from the tile of r, Rt [Mp][32] in LDS (rows m >= M zero), and this lane's rho = sum_m r[m][lane & 31].  `p`
// has X, ldx, dX, lddx (all offset to the launch's first row), G, D, Mp, centroid, inv_two_l2, Ztimg (the packed image of
// Zc^T [D rounded up to 32, Mp], zero padded) and vec_x / vec_dx (16-byte loads of X / stores of dX are aligned).
// Columns at or past D and rows at or past G are never written.
template <class Args>
__device__ __forceinline__ void gp_input_tile(const Args& p, const float* Rt, float rho, long row0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int nC = (p.D + 31) >> 5, nk8 = p.Mp >> 3;
  const long row = row0 + r;
  const bool live = row < p.G;
  const float scale = 2.f * p.inv_two_l2;
  const float* xrow = p.X + row * p.ldx;
  float* orow = p.dX + row * p.lddx;
  // one rounding sequence whichever path loads and stores: the bits do not depend on the strides
  auto value = [&](float acc, float x, int d) { return scale * fmaf(-rho, x - p.centroid[d], acc); };
  auto emit = [&](int c, const f32x16& acc) {
    if (!live) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d0 = gp_acc_index(c, 4 * q, hi);                            // registers 4 q .. 4 q + 3: d0 .. d0 + 3
      if (d0 + 3 < p.D) {
        float x[4];
        if (p.vec_x) {
          const float4 xv = *(const float4*)(xrow + d0);
          x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) x[i] = xrow[d0 + i];
        }
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = value(acc[4 * q + i], x[i], d0 + i);
        if (p.vec_dx) {
          *(float4*)(orow + d0) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) orow[d0 + i] = o[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int d = d0 + i;
          if (d < p.D) orow[d] = value(acc[4 * q + i], xrow[d], d);
        }
      }
    }
  };
  // The nC chunks of 32 embedding dimensions in 8 contiguous shares, the nC % 8 larger ones to the first waves: waves w and
  // w + 4 run on one SIMD, so the matrix work per SIMD is even where nC % 8 <= 4 (D = 384: shares of 2 and 1 chunks, 3 per
  // SIMD; D = 640: of 3 and 2, 5 per SIMD).  A share runs as pairs, its last three chunks as one triple (one pass over the
  // tile in place of two).  Measured at N = 10^6, M = 1000: against shares dealt 1, 2, 1, 2, .. and pairs
  // plus a single, 11.7 -> 9.9 ms at D = 384 and 17.0 -> 14.4 ms at D = 640.
  const int base = nC / GP_WAVES, rem = nC % GP_WAVES;
  const int c_lo = wave * base + min(wave, rem), c_hi = c_lo + base + (wave < rem ? 1 : 0);
  for (int c = c_lo; c < c_hi;) {
    if (c + 3 == c_hi) {
      f32x16 acc[3];
      gp_factor_products<3>(p.Ztimg, Rt, c, nC, nk8, nk8, lane, acc);
      emit(c, acc[0]);
      emit(c + 1, acc[1]);
      emit(c + 2, acc[2]);
      c += 3;
    } else if (c + 1 < c_hi) {
      f32x16 acc[2];
      gp_factor_products<2>(p.Ztimg, Rt, c, nC, nk8, nk8, lane, acc);
      emit(c, acc[0]);
      emit(c + 1, acc[1]);
      c += 2;
    } else {
      f32x16 acc[1];
      gp_factor_products<1>(p.Ztimg, Rt, c, nC, nk8, nk8, lane, acc);
      emit(c, acc[0]);
      c += 1;
    }
  }
}

// K^T[m][row] = s exp(-d2 inv_two_l2) of the tile into Kt [Mp][32] (LDS), 0 for m >= M.  The caller synchronises before it
// reads Kt.
template <class Args>
__device__ __forceinline__ void gp_kernel_tile(const Args& p, long row0, float* Kt, float* Xs) {
  const int r = threadIdx.x & 31;
  gp_distance_tile(p, row0, Xs, [&](int m, float d2) {
    const float kv = p.s * expf(-d2 * p.inv_two_l2);
    Kt[m * GP_ROWS + r] = m < p.M ? kv : 0.f;
  });
}
