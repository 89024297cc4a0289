// The hypernetwork contraction's weight gradient:  out[a,b,c] = sum_n p[n,a] q[n,b] r[n,c]  (bilinear.hip has the forward
// contractions it belongs to).  Four routes, chosen once in bilinear_wgrad_launch: the batched fp16 kernels (f16x3: here;
// f16x3c: wgradc.hip), six-pass planes, the f32-input MFMA kernel, and the fp32 engine (gemm.hip) at widths other than 128.
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"
#include "wgrad_batch.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// weight gradient: out[a,b,c] = sum_n p[n,a] q[n,b] r[n,c]
// grid (NA, splits): one 128(b) x 128(c) output tile per workgroup over a slice of rows
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void bilinear_wgrad128_kernel(const float* __restrict__ p, long ldp,
                                                                const float* __restrict__ q, long ldq,
                                                                const float* __restrict__ rr, long ldr,
                                                                float* __restrict__ slab, int nrows,
                                                                int rows_per_split, int NA) {
  __shared__ __attribute__((aligned(16))) float qs[2][32 * 128];
  __shared__ __attribute__((aligned(16))) float rs[2][32 * 128];
  __shared__ float ps[2][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int a = blockIdx.x, z = blockIdx.y;
  const int nbeg = z * rows_per_split;
  const int nend = min(nrows, nbeg + rows_per_split);
  const int wb = (wave >> 1) * 64, wc = (wave & 1) * 64;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 16; ++t) acc[i][j][t] = 0.f;

  // staging registers (named, not an array captured by a lambda: that form went to scratch)
  float4 vq0, vq1, vq2, vq3, vr0, vr1, vr2, vr3;
  float vp = 0.f;
  const int f_n = tid >> 5, f_cq = tid & 31;  // piece i covers chunk row f_n + 8*i
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#define WG_LOAD1(i_, vq_, vr_)                                                  \
  {                                                                             \
    int n = n0_ + f_n + 8 * (i_);                                               \
    if (n < nend) {                                                             \
      vq_ = *reinterpret_cast<const float4*>(q + (long)n * ldq + 4 * f_cq);     \
      vr_ = *reinterpret_cast<const float4*>(rr + (long)n * ldr + 4 * f_cq);    \
    } else {                                                                    \
      vq_ = zero4;                                                              \
      vr_ = zero4;                                                              \
    }                                                                           \
  }
#define WG_GLOAD(n0)                                                            \
  {                                                                             \
    const int n0_ = (n0);                                                       \
    WG_LOAD1(0, vq0, vr0) WG_LOAD1(1, vq1, vr1) WG_LOAD1(2, vq2, vr2) WG_LOAD1(3, vq3, vr3) \
    if (tid < 32) vp = (n0_ + tid < nend) ? p[(long)(n0_ + tid) * ldp + a] : 0.f; \
  }
#define WG_LSTORE(buf)                                                          \
  {                                                                             \
    float* dq = &qs[buf][f_n * 128 + 4 * f_cq];                                 \
    float* dr = &rs[buf][f_n * 128 + 4 * f_cq];                                 \
    *reinterpret_cast<float4*>(dq) = vq0;                                       \
    *reinterpret_cast<float4*>(dq + 8 * 128) = vq1;                             \
    *reinterpret_cast<float4*>(dq + 16 * 128) = vq2;                            \
    *reinterpret_cast<float4*>(dq + 24 * 128) = vq3;                            \
    *reinterpret_cast<float4*>(dr) = vr0;                                       \
    *reinterpret_cast<float4*>(dr + 8 * 128) = vr1;                             \
    *reinterpret_cast<float4*>(dr + 16 * 128) = vr2;                            \
    *reinterpret_cast<float4*>(dr + 24 * 128) = vr3;                            \
    if (tid < 32) ps[buf][tid] = vp;                                            \
  }

  // two-level summation over the (long) row dimension: partial sums of 512 rows
  f32x16 tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int t = 0; t < 16; ++t) tot[i][j][t] = 0.f;
  const int nchunks = (nend - nbeg + 31) / 32;
  if (nchunks > 0) {
    WG_GLOAD(nbeg);
    WG_LSTORE(0);
  }
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunks) WG_GLOAD(nbeg + (c + 1) * 32);
    if ((c & 15) == 0 && c > 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int t = 0; t < 16; ++t) acc[i][j][t] = 0.f;
        }
    }
    {  // operands of step i+1 are fetched from LDS before the MFMAs of step i issue
      const float* qb = &qs[cur][hi * 128 + wb + r];
      const float* rb = &rs[cur][hi * 128 + wc + r];
      const float* pb = &ps[cur][hi];
      float pv = pb[0], q0 = qb[0], q1 = qb[32], b0 = rb[0], b1 = rb[32];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float pvn = pv, q0n = q0, q1n = q1, b0n = b0, b1n = b1;
        if (i < 15) {
          pvn = pb[2 * (i + 1)];
          q0n = qb[(2 * (i + 1)) * 128];
          q1n = qb[(2 * (i + 1)) * 128 + 32];
          b0n = rb[(2 * (i + 1)) * 128];
          b1n = rb[(2 * (i + 1)) * 128 + 32];
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the next step's LDS reads ahead of this step's MFMAs
        const float a0 = pv * q0, a1 = pv * q1;
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        pv = pvn; q0 = q0n; q1 = q1n; b0 = b0n; b1 = b1n;
      }
    }
    if (c + 1 < nchunks) WG_LSTORE(cur ^ 1);
    __syncthreads();
  }
#undef WG_LOAD1
#undef WG_GLOAD
#undef WG_LSTORE
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] += tot[i][j];
  float* o = slab + ((long)z * NA + a) * 128 * 128;
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      int b = wb + bi * 32 + (t & 3) + 8 * (t >> 2) + 4 * hi;
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) o[(long)b * 128 + wc + bj * 32 + r] = acc[bi][bj][t];
    }
}

// ---------------------------------------------------------------------------------------
// Split-bf16 weight gradient:  out[a,b,c] = sum_n p[n,a] q[n,b] r[n,c]  with the contraction
// index n on the MFMA k axis.  Pre-passes (once per call, ~0.1 ms at N = 83k):
//   pT, qT [128][Np]   transposes (Np = N rounded up to 32, zero padded): an A fragment needs 8
//                      consecutive n for one b
//   Rq [Np/16][piece][cb][h][r][j]   r split into three bf16 planes in B-fragment order
// Workgroup = 8 waves = two `a` values (waves 0-3 / 4-7) x 128 b x 128 c; wave = 32 b x 128 c.
// The A fragment (p*q, 8 values per lane) is split on the fly; six MFMA passes, smallest first.
// ---------------------------------------------------------------------------------------
// mx (optional): max |in| is folded into it (zeroed before; f16x3 mode)
__global__ void transpose_pad_kernel(const float* __restrict__ in, long ld, int rows, int cols, int rows_pad,
                                     float* __restrict__ out, float* __restrict__ mx) {  // out[c][n] = in[n][c], n < rows_pad (zeros beyond rows)
  __shared__ float t[32][33];
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 8 rows per pass
  float m = 0.f;
  for (int i = ty; i < 32; i += 8) {
    int n = n0 + i, c = c0 + tx;
    const float v = (n < rows && c < cols) ? in[(long)n * ld + c] : 0.f;
    t[i][tx] = v;
    m = fmaxf(m, fabsf(v));
  }
  if (mx) block_absmax_commit(m, mx);
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    int c = c0 + i, n = n0 + tx;
    if (c < cols && n < rows_pad) out[(long)c * rows_pad + n] = t[tx][i];
  }
}

// F16: two fp16 planes of 2^k r, 2^k from mx[2] = max |r| (f16x3 mode; mx = {max|p|, max|q|, max|r|})
template <bool F16>
__global__ void split_rows_bf16_kernel(const float* __restrict__ r, long ldr, int rows, int rows_pad,
                                       __bf16* __restrict__ dst, const float* __restrict__ mx) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows_pad * 128) return;
  const int n = (int)(i >> 7), c = (int)(i & 127);
  float v = n < rows ? r[(long)n * ldr + c] : 0.f;
  const int s = n >> 4, h = (n >> 3) & 1, j = n & 7, cb = c >> 5, rr = c & 31;
  constexpr int NP = F16 ? 2 : 3;
  const long base = (long)s * NP * 4;
  if constexpr (F16) {
    float sr, ir;
    pow2_scale(mx[2], sr, ir);
    v *= sr;
    const _Float16 x1 = (_Float16)v, x2 = (_Float16)(v - (float)x1);
    _Float16* d16 = reinterpret_cast<_Float16*>(dst);
    d16[((((base + 0 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x1;
    d16[((((base + 1 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x2;
  } else {
    __bf16 x1, x2, x3;
    split3_bf16(v, x1, x2, x3);
    dst[((((base + 0 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x1;
    dst[((((base + 1 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x2;
    dst[((((base + 2 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x3;
  }
}

// Tried and dropped (round 1): the same kernel on v_mfma_f32_16x16x32_bf16 with the product split of the next k-step
// interleaved between the MFMAs and the flush through slab tiles -- 1.74 ms vs 1.66 ms for this form.  The kernel is
// bound by the SIMD's vector ISSUE port, not by the matrix pipe: per 32-row step a wave issues ~170 VALU instructions
// for the 16 product splits (4 cycles each) and its MFMAs hold the port for 8 cycles apiece; 96 16x16x32 MFMAs
// (768 cycles of issue) leave less room beside them than 48 32x32x16 ones (384), so here the 32x32x16 shape wins
// although it clocks lower.  Fewer VALU instructions per split is the remaining lever.
template <int PASSES>
__global__ __launch_bounds__(512, 2) void bilinear_wgrad128_bf16_kernel(const float* __restrict__ pT,
                                                                        const float* __restrict__ qT,
                                                                        const uint4* __restrict__ Rq,
                                                                        float* __restrict__ slab, int rows_pad,
                                                                        int rows_per_split, int NA,
                                                                        const float* __restrict__ mx) {
  constexpr bool F16 = PASSES == 2;        // two fp16 planes, three passes; mx = {max|p|, max|q|, max|r|}
  constexpr int NP = F16 ? 2 : 3;
  constexpr int KS = 2;                    // k-steps (16 rows each) per chunk
  constexpr int RCH = KS * NP * 256;       // 16-byte pieces of Rq per chunk
  constexpr int QP = 36;                   // pitch (floats) of the q^T tile: conflict-free 16-byte reads
  __shared__ uint4 Rs[2][RCH];
  __shared__ __attribute__((aligned(16))) float Qs[2][128 * QP];
  __shared__ __attribute__((aligned(16))) float Ps[2][2 * 32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int grp = wave >> 2, wb = wave & 3;
  // XCD-aware placement: workgroups are dealt to the 8 XCDs round-robin by linear id, and every workgroup of a row
  // split streams the same q^T / r tiles.  With (x, y) = (a pair, split) in natural order each XCD's L2 would serve
  // all splits' streams at once (27 MB each, 4 MB of L2); remapped, the workgroups sharing an XCD share ONE stream
  // and run in near lockstep, so the tiles are fetched into that L2 once instead of once per workgroup.
  int bx = blockIdx.x, by = blockIdx.y;
  {
    const int nx = gridDim.x, ny = gridDim.y, total = nx * ny;
    if (total % 8 == 0 && 8 % ny == 0) {
      const int lin = by * nx + bx, xcd = lin & 7, w = lin >> 3;   // w-th workgroup of its XCD
      const int xps = 8 / ny;                                      // XCDs per split
      by = xcd / xps;
      bx = (xcd % xps) * (total / 8) + w;                          // a-pair index inside the split
      if (bx >= nx) { bx = blockIdx.x; by = blockIdx.y; }          // irregular grid: natural order
    }
  }
  const int a0 = bx * 2, z = by;
  const int nbeg = z * rows_per_split;
  const int nend = min(rows_pad, nbeg + rows_per_split);
  const int nchunks = (nend - nbeg) / 32;   // rows_per_split and rows_pad are multiples of 32

  f32x16 acc[4], tot[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int t = 0; t < 16; ++t) { acc[cb][t] = 0.f; tot[cb][t] = 0.f; }

  // F16: the products p*q are brought into fp16 range by 2^k from max|p| max|q| (folded into the staged p); the sums
  // come out scaled by that and by r's scale
  float spq = 1.f, inv_all = 1.f;
  if constexpr (F16) {
    float ipq, sr, ir;
    pow2_scale(mx[0] * mx[1], spq, ipq);
    pow2_scale(mx[2], sr, ir);
    inv_all = ipq * ir;
  }
  uint4 pr0, pr1, pr2;
  float4 pq0, pq1;
  float pp = 0.f;
  const int qb0 = tid >> 3, qn4 = tid & 7;                 // q^T pieces: rows qb0 and qb0 + 64
#define WG_GLOAD(n0_)                                                                   \
  {                                                                                     \
    const uint4* rb = Rq + (long)((n0_) >> 4) * (NP * 256) + tid;                       \
    pr0 = rb[0]; pr1 = rb[512];                                                         \
    if (NP == 3) pr2 = rb[1024];                                                        \
    pq0 = *reinterpret_cast<const float4*>(qT + (long)qb0 * rows_pad + (n0_) + 4 * qn4);        \
    pq1 = *reinterpret_cast<const float4*>(qT + (long)(qb0 + 64) * rows_pad + (n0_) + 4 * qn4); \
    if (tid < 64) {                                                                     \
      const int aa = a0 + (tid >> 5);                                                   \
      pp = aa < NA ? pT[(long)aa * rows_pad + (n0_) + (tid & 31)] : 0.f;                \
      if (F16) pp *= spq;                                                               \
      if (((((n0_) - nbeg) >> 5) >> 4) & 1) pp = -pp; /* odd flush groups accumulate -p*q*r */ \
    }                                                                                   \
  }
#define WG_LSTORE(buf_)                                                                 \
  {                                                                                     \
    uint4* lb = &Rs[buf_][tid];                                                         \
    lb[0] = pr0; lb[512] = pr1;                                                         \
    if (NP == 3) lb[1024] = pr2;                                                        \
    *reinterpret_cast<float4*>(&Qs[buf_][qb0 * QP + 4 * qn4]) = pq0;                    \
    *reinterpret_cast<float4*>(&Qs[buf_][(qb0 + 64) * QP + 4 * qn4]) = pq1;             \
    if (tid < 64) Ps[buf_][tid] = pp;                                                   \
  }
  if (nchunks > 0) {
    WG_GLOAD(nbeg);
    WG_LSTORE(0);
  }
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int cur = c & 1;
    if (c + 1 < nchunks) WG_GLOAD(nbeg + (c + 1) * 32);
    if ((c & 15) == 0 && c > 0) {   // two-level summation over the long row dimension (512-row partials);
      // groups alternate in sign (see bilinear_rows128_bf16_kernel: cancels the bf16 MFMA's floor bias)
      const float sg = (((c >> 4) - 1) & 1) ? -1.f : 1.f;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        tot[cb] += acc[cb] * sg;
#pragma unroll
        for (int t = 0; t < 16; ++t) acc[cb][t] = 0.f;
      }
    }
    const bf16x8* bs = reinterpret_cast<const bf16x8*>(&Rs[cur][hi * 32 + r]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const float4* q4 = reinterpret_cast<const float4*>(&Qs[cur][(wb * 32 + r) * QP + ks * 16 + 8 * hi]);
      const float4* p4 = reinterpret_cast<const float4*>(&Ps[cur][grp * 32 + ks * 16 + 8 * hi]);
      const float4 qa = q4[0], qb = q4[1], pa = p4[0], pb = p4[1];
      const float av[8] = {pa.x * qa.x, pa.y * qa.y, pa.z * qa.z, pa.w * qa.w,
                           pb.x * qb.x, pb.y * qb.y, pb.z * qb.z, pb.w * qb.w};
      bf16x8 a1, a2v, a3;
      if constexpr (F16) {
        split2_x8_f16(av, a1, a2v);
      } else {
        split3_x8(av, a1, a2v, a3);
      }
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        const bf16x8 b1 = bs[((ks * NP + 0) * 4 + cb) * 64];
        const bf16x8 b2 = bs[((ks * NP + 1) * 4 + cb) * 64];
        if constexpr (F16) {
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a2v), __builtin_bit_cast(f16x8, b1), acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, b2), acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, b1), acc[cb], 0, 0, 0);
        } else {
          if (PASSES >= 6) {
            const bf16x8 b3 = bs[((ks * 3 + 2) * 4 + cb) * 64];
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3, b1, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b3, acc[cb], 0, 0, 0);
            acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2v, b2, acc[cb], 0, 0, 0);
          }
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2v, b1, acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b2, acc[cb], 0, 0, 0);
          acc[cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc[cb], 0, 0, 0);
        }
      }
    }
    if (c + 1 < nchunks) WG_LSTORE(cur ^ 1);
    __syncthreads();
  }
#undef WG_GLOAD
#undef WG_LSTORE
  const int a = a0 + grp;
  if (a >= NA) return;
  float* o = slab + ((long)z * NA + a) * 128 * 128;
  const float sg_last = (nchunks > 0 && (((nchunks - 1) >> 4) & 1)) ? -1.f : 1.f;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    acc[cb] = acc[cb] * sg_last + tot[cb];
    if constexpr (F16) acc[cb] = acc[cb] * inv_all;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int b = wb * 32 + (t & 3) + 8 * (t >> 2) + 4 * hi;
      o[(long)b * 128 + cb * 32 + r] = acc[cb][t];
    }
  }
}

// ---------------------------------------------------------------------------------------
// f16x3 weight gradient, BATCHED over predicted layers and software-pipelined (round 2).
//
// Same arithmetic and data layout as bilinear_wgrad128_bf16_kernel<2> above (pT, qT transposes, Rq = two fp16 planes of
// 2^k r in B-fragment order, products p*q split on the fly, 512-row partial sums with alternating sign), two changes:
//  * one launch covers every (layer, row split, a pair) unit: the four predicted layers of a hypernetwork give
//    4 x 64 = 256 units = one workgroup per CU with NO row split, so the slabs, their summation pass and three of
//    the four launches disappear (the per-layer launches of round 1 had to split the rows four ways to fill the chip,
//    or ran on half of it beside another stream).  A workgroup loops over units when the grid is smaller.
//  * the loop is a software pipeline in source order, pinned with sched_barrier: the round-1 kernel ran, per 16-row
//    step and wave, [4 LDS reads -> 24 VALU of product split -> 12 MFMAs] back to back, and because the two waves of
//    a SIMD leave the chunk barrier together they both sat in the read + split phase at the same time with the matrix
//    pipe idle (measured 0.50 of the MFMA issue rate).  Here the A fragments of step s+1 are produced in the issue
//    slots an MFMA leaves free (it holds the vector port for 8 of its 32 cycles) while the MFMAs of step s run, the
//    B fragments are double-buffered one column block ahead, and a three-slot LDS ring lets the fragments of the next
//    chunk be fetched BEFORE the chunk barrier, so no wave starts a chunk with an empty matrix pipe.
// ---------------------------------------------------------------------------------------
// (WgradBatchDesc / WgradPrepDesc: wgrad_batch.h)

// mx[4 * (l0 + layer) + which] = max |tensor|, which 0 / 1 / 2 = p / q / r  (mx zeroed before; also wgradc.hip)
__global__ void absmax_rows_batch_kernel(WgradPrepDesc d, int l0, long ldp, long ldq, long ldr, int rows, int NA,
                                         float* __restrict__ mx) {
  const int layer = blockIdx.y / 3, which = blockIdx.y % 3;
  const float* t = which == 0 ? d.p[layer] : (which == 1 ? d.q[layer] : d.r[layer]);
  const long ld = which == 0 ? ldp : (which == 1 ? ldq : ldr);
  const int cols = which == 0 ? NA : 128;
  float m = 0.f;
  if (cols == 128 && (ld & 3) == 0 && (((uintptr_t)t) & 15) == 0) {
    m = absmax_rows128(t, ld, rows, blockIdx.x, gridDim.x);
  } else {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)rows * cols; i += (long)gridDim.x * blockDim.x)
      m = fmaxf(m, fabsf(t[(i / cols) * ld + (i % cols)]));
  }
  block_absmax_commit(m, mx + 4 * (l0 + layer) + which);
}
int absmax_rows_batch_launch(const WgradPrepDesc& d, int l0, int n, long ldp, long ldq, long ldr, int rows, int NA,
                             float* mx, int wgs, hipStream_t stream) {
  hipLaunchKernelGGL(absmax_rows_batch_kernel, dim3(wgs, 3 * n), dim3(256), 0, stream, d, l0, ldp, ldq, ldr, rows, NA, mx);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// z = 2 * layer + which: which 0 -> pT [128][rows_pad] = (p * 2^k * sign(n))^T, 2^k from max|p| max|q| (the products
// p*q must fit fp16) and sign(n) = -1 in the odd 512-row groups of n's row split (the kernel's partial sums alternate
// in sign); which 1 -> qT = q^T.  Rows beyond `rows` and columns beyond NA are zero.
__global__ void transpose_pad_batch_kernel(WgradPrepDesc d, long ldp, long ldq, int rows, int NA, int rows_pad,
                                           int rows_per_split, float* __restrict__ pT, float* __restrict__ qT, long sT,
                                           const float* __restrict__ mx) {
  __shared__ float t[32][33];
  const int layer = blockIdx.z >> 1, which = blockIdx.z & 1;
  const float* in = which ? d.q[layer] : d.p[layer];
  const long ld = which ? ldq : ldp;
  const int cols = which ? 128 : NA;
  float* out = (which ? qT : pT) + (long)layer * sT;
  const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float scale = 1.f;
  if (!which) {
    float ipq;
    pow2_scale(mx[4 * layer] * mx[4 * layer + 1], scale, ipq);
    if ((((n0 % rows_per_split) >> 5) >> 4) & 1) scale = -scale;   // a 32-row tile never straddles a 512-row group
  }
  for (int i = ty; i < 32; i += 8) {
    const int n = n0 + i, c = c0 + tx;
    t[i][tx] = (n < rows && c < cols) ? in[(long)n * ld + c] * scale : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, n = n0 + tx;
    if (c < 128 && n < rows_pad) out[(long)c * rows_pad + n] = t[tx][i];
  }
}
__global__ void split_rows_f16_batch_kernel(WgradPrepDesc d, long ldr, int rows, int rows_pad, _Float16* __restrict__ dst,
                                            long sR_halfs, const float* __restrict__ mx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows_pad * 128) return;
  const int layer = blockIdx.y;
  const int n = (int)(i >> 7), c = (int)(i & 127);
  float v = n < rows ? d.r[layer][(long)n * ldr + c] : 0.f;
  const int s = n >> 4, h = (n >> 3) & 1, j = n & 7, cb = c >> 5, rr = c & 31;
  const long base = (long)s * 2 * 4;
  float sr, ir;
  pow2_scale(mx[4 * layer + 2], sr, ir);
  v *= sr;
  const _Float16 x1 = (_Float16)v, x2 = (_Float16)(v - (float)x1);
  _Float16* d16 = dst + (long)layer * sR_halfs;
  d16[((((base + 0 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x1;
  d16[((((base + 1 * 4 + cb) * 2 + h) * 32 + rr) * 8) + j] = x2;
}

// Ring slot (one 32-row chunk): Rs = two k-steps x two planes x four column blocks x 64 lanes x 16 B of r fragments;
// Qs = the q^T tile [128 b][32 n] with the eight 16-byte pieces of a row XOR-swizzled by (b >> 1) & 7 (LDS-DMA writes
// 1 KB per wave instruction linearly, so there is no room for a padded pitch: the swizzle is applied on the GLOBAL
// address each lane fetches, and makes the 16-byte fragment reads of 32 consecutive rows conflict-free); Ps = the
// two staged p rows.
#define WGP_RS_B 16384
#define WGP_QS_B 16384
#define WGP_PS_B 256
#define WGP_BUF_B (WGP_RS_B + WGP_QS_B + WGP_PS_B)
#define WGP_SLOTS 4
#define WGP_SB() __builtin_amdgcn_sched_barrier(0)

// one pair of products -> one 32-bit word of each fragment plane (6 VALU)
#define WGP_SPLIT(k_, pa_, pb_, qa_, qb_)                                    \
  {                                                                          \
    unsigned w1_, w2_;                                                       \
    split2_pair_f16((pa_) * (qa_), (pb_) * (qb_), w1_, w2_);                 \
    asm volatile("" : "+v"(w1_), "+v"(w2_)); /* packed words NOW: the conversions must not sink into the next step */ \
    nh[k_] = w1_; nl[k_] = w2_;                                              \
  }

__global__ __launch_bounds__(512, 2) void bilinear_wgrad128_f16p_kernel(const float* __restrict__ pT_,
                                                                        const float* __restrict__ qT_,
                                                                        const uint4* __restrict__ Rq_,
                                                                        const float* __restrict__ mx_,
                                                                        WgradBatchDesc u) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[WGP_SLOTS * WGP_BUF_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int grp = wave >> 2, wb = wave & 3;
  const int total = u.n_layers * u.splits * u.npairs, streams = u.n_layers * u.splits;
  const bool xcd_map = total % 8 == 0 && streams <= 8 && 8 % streams == 0 && u.npairs % (8 / streams) == 0 &&
                       gridDim.x % 8 == 0;
  const int rows_pad = u.rows_pad;
  // ---- per-lane LDS read offsets inside a slot ----
  const unsigned rd_rs = lane * 16;
  const int rowb = wb * 32 + r;
  const int fsw = (rowb >> 1) & 7;
  unsigned rd_q[2][2];   // [k-step][first / second 16-byte piece of the lane's 8 values]
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int e = 0; e < 2; ++e) rd_q[ks][e] = WGP_RS_B + rowb * 128 + (((ks * 4 + 2 * hi + e) ^ fsw) << 4);
  const unsigned rd_ps = WGP_RS_B + WGP_QS_B + (grp * 32 + 8 * hi) * 4;
  // ---- LDS-DMA: scalar LDS bases of this wave's pieces, per-lane global byte offsets ----
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned dma_w = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const unsigned voff_r = (unsigned)tid * 16;
  const unsigned voff_q = (unsigned)(((tid >> 3) * (long)rows_pad + 4 * ((tid & 7) ^ ((tid >> 4) & 7))) * 4);
  const unsigned voff_q2 = voff_q + (unsigned)((long)64 * rows_pad * 4);

  for (int v = blockIdx.x; v < total; v += gridDim.x) {
    // XCD-aware placement: workgroups are dealt to the 8 XCDs round-robin by linear id, and every workgroup of a
    // (layer, split) stream reads the same q^T / r tiles.  Mapped so that the workgroups sharing an XCD share ONE stream
    // and run in near lockstep, the tiles enter that L2 once instead of once per workgroup (speed only).
    int stream, pair;
    if (xcd_map) {
      const int xcd = v & 7, w = v >> 3, xps = 8 / streams;
      stream = xcd / xps;
      pair = (xcd % xps) * (total / 8) + w;
    } else {
      stream = v / u.npairs;
      pair = v % u.npairs;
    }
    stream = __builtin_amdgcn_readfirstlane(stream);   // uniform: keep the unit's addressing on the scalar unit
    pair = __builtin_amdgcn_readfirstlane(pair);
    const int layer = stream / u.splits, z = stream % u.splits;
    const int a0 = pair * 2;
    const int nbeg = z * u.rows_per_split;
    const int nend = min(rows_pad, nbeg + u.rows_per_split);
    const int nchunks = (nend - nbeg) / 32;   // rows_per_split and rows_pad are multiples of 32
    const char* pT = reinterpret_cast<const char*>(pT_ + (long)layer * u.sT + (long)a0 * rows_pad);
    const char* qT = reinterpret_cast<const char*>(qT_ + (long)layer * u.sT);
    const char* Rq = reinterpret_cast<const char*>(Rq_ + (long)layer * u.sR);
    const float* mx = mx_ + 4 * layer;
    const unsigned voff_p = (unsigned)(((lane >> 5) * (long)rows_pad + (lane & 31)) * 4);

    f32x16 acc[4], tot[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int t = 0; t < 16; ++t) { acc[cb][t] = 0.f; tot[cb][t] = 0.f; }
    float inv_all;
    {
      float spq, ipq, sr, ir;
      pow2_scale(mx[0] * mx[1], spq, ipq);
      pow2_scale(mx[2], sr, ir);
      inv_all = ipq * ir;
    }
    if (nchunks > 0) {
      // chunk ci -> ring slot ci % 4; five LDS-DMA instructions per wave (the index is clamped: the last iterations
      // re-load the last chunk into a slot nobody reads, which keeps the vmcnt arithmetic uniform)
#define WGP_DMA(ci_)                                                                        \
  {                                                                                         \
    const int cc_ = (ci_) < nchunks ? (ci_) : nchunks - 1;                                  \
    const long n0_ = nbeg + (long)cc_ * 32;                                                 \
    const unsigned d_ = dma_w + (unsigned)((ci_) & 3) * WGP_BUF_B;                          \
    const char* rb_ = Rq + (n0_ >> 4) * 8192;                                               \
    glds_b128(rb_, voff_r, d_);                                                             \
    glds_b128(rb_ + 8192, voff_r, d_ + 8192);                                               \
    glds_b128(qT + n0_ * 4, voff_q, d_ + WGP_RS_B);                                         \
    glds_b128(qT + n0_ * 4, voff_q2, d_ + WGP_RS_B + 8192);                                 \
    glds_b32(pT + n0_ * 4, voff_p, sbase + (unsigned)((ci_) & 3) * WGP_BUF_B + WGP_RS_B + WGP_QS_B); \
  }
      WGP_DMA(0);
      WGP_DMA(1);
      WGP_DMA(2);
      wait_vmcnt<5>();                  // chunks 0 and 1 have landed (this wave's pieces) ...
      __builtin_amdgcn_s_barrier();     // ... and everybody else's
      asm volatile("" ::: "memory");
      // fragments of the first step
      unsigned nh[4], nl[4];
      bf16x8 B[2][2];
      {
        const float4 qa = *reinterpret_cast<const float4*>(smem + rd_q[0][0]);
        const float4 qb = *reinterpret_cast<const float4*>(smem + rd_q[0][1]);
        const float4 pa = *reinterpret_cast<const float4*>(smem + rd_ps);
        const float4 pb = *reinterpret_cast<const float4*>(smem + rd_ps + 16);
        WGP_SPLIT(0, pa.x, pa.y, qa.x, qa.y) WGP_SPLIT(1, pa.z, pa.w, qa.z, qa.w)
        WGP_SPLIT(2, pb.x, pb.y, qb.x, qb.y) WGP_SPLIT(3, pb.z, pb.w, qb.z, qb.w)
        B[0][0] = *reinterpret_cast<const bf16x8*>(smem + rd_rs);
        B[0][1] = *reinterpret_cast<const bf16x8*>(smem + rd_rs + 4096);
      }
      // One 16-row step: 12 MFMAs on the fragments (a1, a2) made during the previous step; meanwhile the p, q values
      // of the NEXT step (slot offset so_, k-step kn_) are read and split into (nh, nl), and the B fragments are
      // fetched one column block ahead (the last prefetch reads the next step's first block at bn_).
#define WGP_STEP(bc_, bn_, so_, kn_)                                                                               \
  {                                                                                                                \
    const bf16x8 a1 = __builtin_bit_cast(bf16x8, make_uint4(nh[0], nh[1], nh[2], nh[3]));                          \
    const bf16x8 a2 = __builtin_bit_cast(bf16x8, make_uint4(nl[0], nl[1], nl[2], nl[3]));                          \
    WGP_SB();                                                                                                      \
    /* ---- column block 0: issue the reads of the next step's p, q ---- */                                        \
    B[1][0] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 1024);                                               \
    B[1][1] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 4096 + 1024);                                        \
    const float4 qa = *reinterpret_cast<const float4*>(smem + (so_) + rd_q[kn_][0]);                               \
    const float4 pa = *reinterpret_cast<const float4*>(smem + (so_) + rd_ps + (kn_) * 64);                         \
    WGP_SB();                                                                                                      \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a2), __builtin_bit_cast(f16x8, B[0][0]), acc[0], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    const float4 qb = *reinterpret_cast<const float4*>(smem + (so_) + rd_q[kn_][1]);                               \
    const float4 pb = *reinterpret_cast<const float4*>(smem + (so_) + rd_ps + (kn_) * 64 + 16);                    \
    WGP_SB();                                                                                                      \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[0][1]), acc[0], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[0][0]), acc[0], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    /* ---- column block 1: split pairs 0, 1 ---- */                                                               \
    B[0][0] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 2048);                                               \
    B[0][1] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 4096 + 2048);                                        \
    WGP_SB();                                                                                                      \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a2), __builtin_bit_cast(f16x8, B[1][0]), acc[1], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    WGP_SPLIT(0, pa.x, pa.y, qa.x, qa.y)                                                                           \
    WGP_SB();                                                                                                      \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[1][1]), acc[1], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    WGP_SPLIT(1, pa.z, pa.w, qa.z, qa.w)                                                                           \
    WGP_SB();                                                                                                      \
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[1][0]), acc[1], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    /* ---- column block 2: split pairs 2, 3 ---- */                                                               \
    B[1][0] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 3072);                                               \
    B[1][1] = *reinterpret_cast<const bf16x8*>(smem + (bc_) + 4096 + 3072);                                        \
    WGP_SB();                                                                                                      \
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a2), __builtin_bit_cast(f16x8, B[0][0]), acc[2], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    WGP_SPLIT(2, pb.x, pb.y, qb.x, qb.y)                                                                           \
    WGP_SB();                                                                                                      \
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[0][1]), acc[2], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    WGP_SPLIT(3, pb.z, pb.w, qb.z, qb.w)                                                                           \
    WGP_SB();                                                                                                      \
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[0][0]), acc[2], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    /* ---- column block 3: first B block of the next step ---- */                                                 \
    B[0][0] = *reinterpret_cast<const bf16x8*>(smem + (bn_));                                                      \
    B[0][1] = *reinterpret_cast<const bf16x8*>(smem + (bn_) + 4096);                                               \
    WGP_SB();                                                                                                      \
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a2), __builtin_bit_cast(f16x8, B[1][0]), acc[3], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[1][1]), acc[3], 0, 0, 0); \
    WGP_SB();                                                                                                      \
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a1), __builtin_bit_cast(f16x8, B[1][0]), acc[3], 0, 0, 0); \
    WGP_SB();                                                                                                      \
  }
#pragma clang loop unroll(disable)
      for (int c = 0; c < nchunks; ++c) {
        // chunk c + 3 into the slot chunk c - 1 was computed from (its readers passed the barrier that ended c - 1)
        WGP_DMA(c + 3);
        if ((c & 15) == 0 && c > 0) {   // two-level summation over the long row dimension (512-row partials);
          // groups alternate in sign (cancels the MFMA accumulator's rounding bias, see bilinear_rows128_ring16_kernel)
          const float sg = (((c >> 4) - 1) & 1) ? -1.f : 1.f;
#pragma unroll
          for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int t = 0; t < 16; ++t) {
              tot[cb][t] = fmaf(acc[cb][t], sg, tot[cb][t]);
              acc[cb][t] = 0.f;
            }
        }
        const unsigned o0 = (unsigned)(c & 3) * WGP_BUF_B, o1 = (unsigned)((c + 1) & 3) * WGP_BUF_B;
        // step 0 of chunk c: next = step 1 of the same slot
        WGP_STEP(o0 + rd_rs, o0 + rd_rs + 8192, o0, 1)
        // step 1: next = step 0 of chunk c + 1 (landed and published by the barrier that ended chunk c - 1)
        WGP_STEP(o0 + rd_rs + 8192, o1 + rd_rs, o1, 0)
        // chunk c + 2 (issued one iteration ago) must have landed before the barrier publishes it; younger than it:
        // only this iteration's five loads
        wait_vmcnt<5>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the clamped re-loads still in flight target this unit's ring
#undef WGP_DMA
#undef WGP_STEP
    }
    const int a = a0 + grp;
    if (a < u.NA) {
      float* o = u.splits == 1 ? u.out[layer] + (long)a * 128 * 128
                               : u.slab + (((long)layer * u.splits + z) * u.NA + a) * 128 * 128;
      const float sg_last = (nchunks > 0 && (((nchunks - 1) >> 4) & 1)) ? -1.f : 1.f;
      // the lane id is laundered so that the 64 per-lane store addresses are computed HERE, once per unit, instead of
      // being hoisted out of the unit loop and kept alive (= spilled) across the main loop
      int tl = tid;
      asm volatile("" : "+v"(tl));
      const int e_r = tl & 31, e_hi = (tl >> 5) & 1, e_wb = (tl >> 6) & 3;
      float* ol = o + (long)(e_wb * 32 + 4 * e_hi) * 128 + e_r;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) {
        acc[cb] = (acc[cb] * sg_last + tot[cb]) * inv_all;
#pragma unroll
        for (int t = 0; t < 16; ++t) ol[((t & 3) + 8 * (t >> 2)) * 128 + cb * 32] = acc[cb][t];
      }
    }
    __syncthreads();   // the ring is re-filled by the next unit's prologue
  }
}

static int wgrad_splits(int nrows, int NA) {
  int s = cdiv(512, NA);                 // aim at >= 2 workgroups per CU
  int maxs = nrows / 256;                // at least 8 chunks of 32 rows per split
  if (s > maxs) s = maxs;
  if (s < 1) s = 1;
  return s;
}

static bool wgrad_fast(const float* q, long ldq, const float* r, long ldr, int NB, int NC) {
  return NB == 128 && NC == 128 && (ldq % 4) == 0 && (ldr % 4) == 0 && (((uintptr_t)q) & 15) == 0 &&
         (((uintptr_t)r) & 15) == 0;
}

static int wgrad_bf16_splits(int NA) { return cdiv(256, cdiv(NA, 2)); }   // one 512-thread workgroup per CU
static size_t wgrad_bf16_ws(int nrows, int NA, size_t* o_pT, size_t* o_qT, size_t* o_Rq, size_t* o_slab) {
  const size_t np = (size_t)cdiv(nrows, 32) * 32;
  size_t off = 0;
  *o_pT = off; off += ws_round(np * 128, 4);
  *o_qT = off; off += ws_round(np * 128, 4);
  *o_Rq = off; off += ws_round(np * 128 * 3, 2);
  *o_slab = off; off += ws_round((size_t)wgrad_bf16_splits(NA) * NA * 128 * 128, 4);
  off += 16;                              // f16x3: {max|p|, max|q|, max|r|} behind the slabs
  return off;
}

// ---- batched f16x3 launch (bilinear_wgrad128_f16p_kernel) ----
// row splits per layer: enough units to fill the chip once (more only adds slab traffic), at least 8 chunks per split
static int wgrad_batch_pick(int n_layers, int nrows, int NA, int* rps_out) {
  const int npairs = cdiv(NA, 2), np = cdiv(nrows, 32) * 32;
  int splits = 256 / (n_layers * npairs);
  if (splits > np / 256) splits = np / 256;
  if (splits < 1) splits = 1;
  const int rps = cdiv(np / 32, splits) * 32;
  if (rps_out) *rps_out = rps;
  return cdiv(np, rps);
}
static size_t wgrad_batch_ws(int n_layers, int nrows, int NA, int splits, size_t* o_pT, size_t* o_qT, size_t* o_Rq,
                             size_t* o_slab, size_t* o_mx) {
  const size_t np = (size_t)cdiv(nrows, 32) * 32;
  size_t off = 0;
  *o_pT = off; off += ws_round((size_t)n_layers * np * 128, 4);
  *o_qT = off; off += ws_round((size_t)n_layers * np * 128, 4);
  *o_Rq = off; off += ws_round((size_t)n_layers * np * 128 * 2, 2);
  *o_slab = off; if (splits > 1) off += ws_round((size_t)n_layers * splits * NA * 128 * 128, 4);
  *o_mx = off; off += 256;
  return off;
}
bool bilinear_wgrad_batch_fast(int n_layers, int NA, int NB, int NC, long ldq, long ldr) {
  return mode_f16_T() && n_layers >= 1 && n_layers <= WGB_MAX && NA >= 1 && NA <= 128 && NB == 128 && NC == 128 &&
         (ldr % 4) == 0;
}
// Does the batched kernel of an n_layers batch take these operands?  The one definition bilinear_wgrad_batch_prep (for
// its layer's pair: n_given = 1), bilinear_wgrad_batch_launch (for all n_layers pairs) and a caller that decides its route
// before its first launch share: the mode and the dims, q and r of every given layer 16-byte aligned, and at most 8e6
// rows (the q^T tile is fetched with 32-bit lane offsets: 128 rows of rows_pad floats must stay below 4 GB).
bool bilinear_wgrad_batch_takes(int n_layers, int n_given, const float* const* q, long ldq, const float* const* r, long ldr,
                                int nrows, int NA, int NB, int NC) {
  bool aligned = true;
  for (int l = 0; l < n_given && l < WGB_MAX; ++l)
    aligned = aligned && ((((uintptr_t)q[l]) | ((uintptr_t)r[l])) & 15) == 0;
  return aligned && nrows > 0 && nrows <= 8000000 && bilinear_wgrad_batch_fast(n_layers, NA, NB, NC, ldq, ldr);
}
size_t bilinear_wgrad_batch_ws_bytes(int n_layers, int nrows, int NA, int NB, int NC) {
  const size_t single = bilinear_wgrad_ws_bytes(nrows, NA, NB, NC);
  if (NB != 128 || NC != 128 || NA > 128 || NA < 1 || n_layers > WGB_MAX || n_layers < 1 || nrows <= 0) return single;
  size_t a, b, c, d, e;
  size_t batch = wgrad_batch_ws(n_layers, nrows, NA, wgrad_batch_pick(n_layers, nrows, NA, nullptr), &a, &b, &c, &d, &e);
  const size_t batch_c = wgradc_ws_bytes(n_layers, nrows, NA);     // f16x3c form (wgradc.hip)
  if (batch_c > batch) batch = batch_c;
  return batch > single ? batch : single;
}
// The batched workspace, carved: per layer pT, qT [128][np] (np = the rows rounded up to 32), Rq = two fp16 planes of
// [np][128], the slabs of `splits` row splits of rps rows, and mx = 4 floats per layer ({max|p|, max|q|, max|r|, -})
struct WgradBatchWs {
  float *pT, *qT, *slab, *mx;
  _Float16* Rq;
  int np, rps, splits;
  size_t need;
};
static int wgrad_batch_carve(WgradBatchWs& w, const char* who, void* ws, size_t ws_bytes, int n_layers, int nrows, int NA) {
  size_t o_pT, o_qT, o_Rq, o_slab, o_mx;
  w.np = cdiv(nrows, 32) * 32;
  w.splits = wgrad_batch_pick(n_layers, nrows, NA, &w.rps);
  w.need = wgrad_batch_ws(n_layers, nrows, NA, w.splits, &o_pT, &o_qT, &o_Rq, &o_slab, &o_mx);
  if (!ws || ws_bytes < w.need) {
    cgat_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, w.need);
    return CGAT_ERR_WORKSPACE;
  }
  w.pT = (float*)((char*)ws + o_pT);
  w.qT = (float*)((char*)ws + o_qT);
  w.Rq = (_Float16*)((char*)ws + o_Rq);
  w.slab = (float*)((char*)ws + o_slab);
  w.mx = (float*)((char*)ws + o_mx);
  return CGAT_OK;
}
// The operand preparation of layers [l0, l0 + n) of the batch (pd: their operands, entry 0 = layer l0): maxima, scaled
// transposes, fp16 planes.  mx_fill floats from layer l0's maxima on are zeroed first.
static int wgrad_f16_prepare(const WgradBatchWs& w, int l0, int n, const WgradPrepDesc& pd, long ldp, long ldq, long ldr,
                             int nrows, int NA, int mx_fill, hipStream_t stream) {
  const long sT = (long)w.np * 128, sR8 = (long)w.np * 128 * 2;   // per-layer strides: floats of pT / qT, halves of Rq
  float* mx = w.mx + 4 * l0;
  CGAT_TRY(fill_launch(mx, 0.f, mx_fill, stream));
  CGAT_TRY(absmax_rows_batch_launch(pd, 0, n, ldp, ldq, ldr, nrows, NA, mx, 256, stream));
  hipLaunchKernelGGL(transpose_pad_batch_kernel, dim3(w.np / 32, 4, 2 * n), dim3(256), 0, stream, pd, ldp, ldq, nrows, NA,
                     w.np, w.rps, w.pT + (size_t)l0 * sT, w.qT + (size_t)l0 * sT, sT, (const float*)mx);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(split_rows_f16_batch_kernel, dim3(cdiv((long)w.np * 128, 256), n), dim3(256), 0, stream, pd, ldr, nrows,
                     w.np, w.Rq + (size_t)l0 * sR8, sR8, (const float*)mx);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
// The operand preparation (maxima, scaled transposes, fp16 planes) of ONE layer -- slot `slot` of an `n_layers` batch --
// so that a caller whose layers become ready one after the other can issue each layer's share early, on any stream,
// and finish with bilinear_wgrad_batch_launch(..., prepared = true) on the same workspace.  CGAT_ERR_UNSUPPORTED when
// the batched f16x3 kernel would not take these operands (the caller then launches unprepared).
int bilinear_wgrad_batch_prep(int slot, int n_layers, const float* p, long ldp, const float* q, long ldq, const float* r,
                              long ldr, int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes,
                              hipStream_t stream) {
  if (slot < 0 || slot >= n_layers || !bilinear_wgrad_batch_takes(n_layers, 1, &q, ldq, &r, ldr, nrows, NA, NB, NC))
    return CGAT_ERR_UNSUPPORTED;
  if (mode_f16c())
    return wgradc_prep(slot, 1, n_layers, &p, ldp, &q, ldq, &r, ldr, nrows, NA, ws, ws_bytes, stream);
  WgradBatchWs w;
  CGAT_TRY(wgrad_batch_carve(w, "bilinear_wgrad_batch_prep", ws, ws_bytes, n_layers, nrows, NA));
  WgradPrepDesc pd;
  memset(&pd, 0, sizeof(pd));
  pd.p[0] = p; pd.q[0] = q; pd.r[0] = r;
  return wgrad_f16_prepare(w, slot, 1, pd, ldp, ldq, ldr, nrows, NA, 4, stream);
}

// out[l][a,b,c] = sum_n p[l][n,a] q[l][n,b] r[l][n,c] for l < n_layers in ONE launch (f16x3 mode; other modes: one
// launch per layer).  max_wgs: workgroups of the grid (0 = 256, one per CU; 128 = half of the chip for running beside
// an HBM-bound kernel on another stream -- every workgroup then walks two units)
int bilinear_wgrad_batch_launch(int n_layers, const float* const* p, long ldp, const float* const* q, long ldq,
                                const float* const* r, long ldr, float* const* out, int nrows, int NA, int NB, int NC,
                                void* ws, size_t ws_bytes, hipStream_t stream, int max_wgs, bool prepared) {
  if (n_layers <= 0) return CGAT_OK;
  if (!bilinear_wgrad_batch_takes(n_layers, n_layers, q, ldq, r, ldr, nrows, NA, NB, NC)) {
    CGAT_CHECK_ARG(!prepared, "bilinear_wgrad_batch: prepared operands but not the batched form");
    for (int l = 0; l < n_layers; ++l)
      CGAT_TRY(bilinear_wgrad_launch(p[l], ldp, q[l], ldq, r[l], ldr, out[l], nrows, NA, NB, NC, ws, ws_bytes, stream,
                                     max_wgs > 0 && max_wgs < 256 ? max_wgs / cdiv(NA, 2) : 0));
    return CGAT_OK;
  }
  if (mode_f16c())
    return wgradc_launch(n_layers, p, ldp, q, ldq, r, ldr, out, nrows, NA, ws, ws_bytes, stream, max_wgs, prepared);
  if (max_wgs <= 0 || max_wgs > 256) max_wgs = 256;
  WgradBatchWs w;
  CGAT_TRY(wgrad_batch_carve(w, "bilinear_wgrad_batch", ws, ws_bytes, n_layers, nrows, NA));
  WgradPrepDesc pd;
  WgradBatchDesc u;
  memset(&pd, 0, sizeof(pd));
  memset(&u, 0, sizeof(u));
  for (int l = 0; l < n_layers; ++l) { pd.p[l] = p[l]; pd.q[l] = q[l]; pd.r[l] = r[l]; u.out[l] = out[l]; }
  u.slab = w.slab;
  u.sT = (long)w.np * 128;
  u.sR = (long)w.np * 128 * 2 * 2 / 16;
  u.n_layers = n_layers; u.splits = w.splits; u.npairs = cdiv(NA, 2); u.NA = NA; u.rows_pad = w.np;
  u.rows_per_split = w.rps;
  if (!prepared) CGAT_TRY(wgrad_f16_prepare(w, 0, n_layers, pd, ldp, ldq, ldr, nrows, NA, 64, stream));
  const int units = n_layers * u.splits * u.npairs;
  {
    CGAT_PROF("bilinear_wgrad", stream);
    hipLaunchKernelGGL(bilinear_wgrad128_f16p_kernel, dim3(units < max_wgs ? units : max_wgs), dim3(512), 0, stream,
                       (const float*)w.pT, (const float*)w.qT, (const uint4*)w.Rq, (const float*)w.mx, u);
  }
  CGAT_LAUNCH_CHECK();
  if (u.splits > 1) {
    const long n = (long)NA * 128 * 128;
    CGAT_TRY(sum_slabs_batch_launch(u.slab, u.splits, n, n, n_layers, u.splits * n, u.out, 128, stream));
  }
  return CGAT_OK;
}

size_t bilinear_wgrad_ws_bytes(int nrows, int NA, int NB, int NC) {
  if (!(NB == 128 && NC == 128) && nrows > 0 && NA > 0 && NB > 0 && NC > 0) {   // fp32 engine, split over the rows
    const int sp = gemm_pick_splits(NA, NB * NC, nrows);
    return sp > 1 ? ws_round((size_t)sp * NA * NB * NC, 4) : 0;
  }
  if (NB == 128 && NC == 128) {
    size_t a, b, c, d;
    size_t bf = wgrad_bf16_ws(nrows, NA, &a, &b, &c, &d);
    size_t f32 = ws_round((size_t)wgrad_splits(nrows, NA) * NA * NB * NC, 4);
    if (f32 > bf) bf = f32;
    if (NA >= 1 && NA <= 128 && nrows > 0) {   // the f16x3 / f16x3c forms: batched kernels with one layer
      size_t e;
      const size_t one = wgrad_batch_ws(1, nrows, NA, wgrad_batch_pick(1, nrows, NA, nullptr), &a, &b, &c, &d, &e);
      if (one > bf) bf = one;
      const size_t one_c = wgradc_ws_bytes(1, nrows, NA);
      if (one_c > bf) bf = one_c;
    }
    return bf;
  }
  return 0;
}

// Six-pass planes (every split mode at NB = NC = 128 that the batched fp16 forms do not take): transposes, plane image of
// r, bilinear_wgrad128_bf16_kernel over row splits, slab sum
static int wgrad_planes(const float* p, long ldp, const float* q, long ldq, const float* r, long ldr, float* out, int nrows,
                        int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream, int force_splits) {
  size_t o_pT, o_qT, o_Rq, o_slab;
  const size_t need = wgrad_bf16_ws(nrows, NA, &o_pT, &o_qT, &o_Rq, &o_slab);
  if (!ws || ws_bytes < need) {
    cgat_set_error("bilinear_wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
    return CGAT_ERR_WORKSPACE;
  }
  const int np = cdiv(nrows, 32) * 32;
  float* pT = (float*)((char*)ws + o_pT);
  float* qT = (float*)((char*)ws + o_qT);
  __bf16* Rq = (__bf16*)((char*)ws + o_Rq);
  float* slab = (float*)((char*)ws + o_slab);
  float* mx = (float*)((char*)ws + need - 16);
  const bool f16 = mode_f16();
  if (f16) CGAT_TRY(fill_launch(mx, 0.f, 4, stream));
  hipLaunchKernelGGL(transpose_pad_kernel, dim3(np / 32, cdiv(NA, 32)), dim3(256), 0, stream, p, ldp, nrows, NA, np, pT,
                     f16 ? mx : (float*)nullptr);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(transpose_pad_kernel, dim3(np / 32, 4), dim3(256), 0, stream, q, ldq, nrows, 128, np, qT,
                     f16 ? mx + 1 : (float*)nullptr);
  CGAT_LAUNCH_CHECK();
  if (f16) {
    CGAT_TRY(absmax_rows128_wgs_launch(r, ldr, nrows, mx + 2, 512, stream));
    hipLaunchKernelGGL(split_rows_bf16_kernel<true>, dim3(cdiv((long)np * 128, 256)), dim3(256), 0, stream, r, ldr, nrows, np, Rq, (const float*)mx);
  } else {
    hipLaunchKernelGGL(split_rows_bf16_kernel<false>, dim3(cdiv((long)np * 128, 256)), dim3(256), 0, stream, r, ldr, nrows, np, Rq, (const float*)mx);
  }
  CGAT_LAUNCH_CHECK();
  int splits = wgrad_bf16_splits(NA);
  if (force_splits > 0 && force_splits < splits) splits = force_splits;
  int rps = cdiv(np / 32, splits) * 32;
  splits = cdiv(np, rps);
  {
    CGAT_PROF("bilinear_wgrad", stream);
    if (f16)
      hipLaunchKernelGGL(bilinear_wgrad128_bf16_kernel<2>, dim3(cdiv(NA, 2), splits), dim3(512), 0, stream, pT, qT,
                         (const uint4*)Rq, slab, np, rps, NA, (const float*)mx);
    else if (!mode_bf16x3())
      hipLaunchKernelGGL(bilinear_wgrad128_bf16_kernel<6>, dim3(cdiv(NA, 2), splits), dim3(512), 0, stream, pT, qT,
                         (const uint4*)Rq, slab, np, rps, NA, (const float*)mx);
    else
      hipLaunchKernelGGL(bilinear_wgrad128_bf16_kernel<3>, dim3(cdiv(NA, 2), splits), dim3(512), 0, stream, pT, qT,
                         (const uint4*)Rq, slab, np, rps, NA, (const float*)mx);
  }
  CGAT_LAUNCH_CHECK();
  long n = (long)NA * NB * NC;
  CGAT_TRY(sum_slabs_launch(slab, splits, n, out, n, stream));
  return CGAT_OK;
}

// fp32 MFMA (mode f32 at NB = NC = 128): bilinear_wgrad128_kernel over row splits, slab sum
static int wgrad_f32_mfma(const float* p, long ldp, const float* q, long ldq, const float* r, long ldr, float* out,
                          int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream) {
  int splits = wgrad_splits(nrows, NA);
  size_t need = ws_round((size_t)splits * NA * NB * NC, 4);
  if (!ws || ws_bytes < need) {
    cgat_set_error("bilinear_wgrad: workspace too small (%zu < %zu)", ws_bytes, need);
    return CGAT_ERR_WORKSPACE;
  }
  int rps = cdiv(nrows, splits);
  rps = ((rps + 31) / 32) * 32;
  splits = cdiv(nrows, rps);
  if (splits < 1) splits = 1;
  {
    CGAT_PROF("bilinear_wgrad", stream);
    hipLaunchKernelGGL(bilinear_wgrad128_kernel, dim3(NA, splits), dim3(256), 0, stream, p, ldp, q, ldq, r, ldr,
                       (float*)ws, nrows, rps, NA);
  }
  CGAT_LAUNCH_CHECK();
  long n = (long)NA * NB * NC;
  return sum_slabs_launch((const float*)ws, splits, n, out, n, stream);
}

// widths other than 128: out [NA, NB * NC] = p^T (q (x) r) on the fp32 engine, rows split over workgroups when the
// output has few tiles (33 ms -> 0.7 at 83 340 rows of width 64)
static int wgrad_engine(const float* p, long ldp, const float* q, long ldq, const float* r, long ldr, float* out,
                        int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream) {
  GemmParams g = gemm_params(NA, NB * NC, nrows, p, ldp, r, ldr, out, (long)NB * NC);
  g.a_kmajor = 1; g.b_kmajor = 1;
  g.b_outer = q; g.ld_b_outer = ldq; g.outer_n = NC;
  g.splits = gemm_pick_splits(NA, NB * NC, nrows);
  if (g.splits > 1 && (!ws || ws_bytes < ws_round((size_t)g.splits * NA * NB * NC, 4))) g.splits = 1;
  return gemm_launch(g, ws, ws_bytes, stream);
}

// force_splits > 0: number of row splits = workgroups per `a` pair (default: enough for one workgroup per CU; 2 gives
// 128 workgroups, i.e. half the chip, for running beside an HBM-bound kernel on another stream)
int bilinear_wgrad_launch(const float* p, long ldp, const float* q, long ldq, const float* r, long ldr, float* out,
                          int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream,
                          int force_splits) {
  if (!wgrad_fast(q, ldq, r, ldr, NB, NC))
    return wgrad_engine(p, ldp, q, ldq, r, ldr, out, nrows, NA, NB, NC, ws, ws_bytes, stream);
  // f16x3 / f16x3c: the batched kernels with one layer (row splits fill the chip)
  if (mode_f16_T() && nrows > 0 && nrows <= 8000000 && NA <= 128)
    return bilinear_wgrad_batch_launch(1, &p, ldp, &q, ldq, &r, ldr, &out, nrows, NA, NB, NC, ws, ws_bytes, stream,
                                       force_splits > 0 ? force_splits * cdiv(NA, 2) : 0);
  if (mode_split() && nrows > 0)
    return wgrad_planes(p, ldp, q, ldq, r, ldr, out, nrows, NA, NB, NC, ws, ws_bytes, stream, force_splits);
  return wgrad_f32_mfma(p, ldp, q, ldq, r, ldr, out, nrows, NA, NB, NC, ws, ws_bytes, stream);
}
