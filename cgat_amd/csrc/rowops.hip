// Row-wise / elementwise kernels around the matrix-core products: LayerNorm(no affine)+tanh
// of the predicted layers (reference Hypernetworksmp.py:103-107), activation derivatives,
// column sums for bias gradients, the H_Net damping mix (Hypernetworksmp.py:310-312).
// All HBM-bound, one wave per row or grid-stride; accurate tanhf/rsqrtf (no fast-math).
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"
#include "rowops_grid.h"

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// y = tanh((u - mean) * rsqrt(var + eps)), biased variance; one wave per row
__global__ void layernorm_tanh_fwd_kernel(const float* __restrict__ u, float* __restrict__ y, int rows, int W,
                                          float eps) {
  int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = u + (long)row * W;
  float s = 0.f;
  for (int c = lane; c < W; c += 64) s += x[c];
  float mean = wave_sum(s) / W;
  float v = 0.f;
  for (int c = lane; c < W; c += 64) {
    float d = x[c] - mean;
    v += d * d;
  }
  float rstd = rsqrtf(wave_sum(v) / W + eps);
  for (int c = lane; c < W; c += 64) y[(long)row * W + c] = tanhf((x[c] - mean) * rstd);
}

// gu = rstd * (gx - mean(gx) - xhat * mean(gx * xhat)),  gx = gy * (1 - y^2)
__global__ void layernorm_tanh_bwd_kernel(const float* __restrict__ u, const float* __restrict__ y,
                                          const float* __restrict__ gy, float* __restrict__ gu, int rows, int W,
                                          float eps) {
  int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* x = u + (long)row * W;
  const float* yy = y + (long)row * W;
  const float* g = gy + (long)row * W;
  float s = 0.f;
  for (int c = lane; c < W; c += 64) s += x[c];
  float mean = wave_sum(s) / W;
  float v = 0.f;
  for (int c = lane; c < W; c += 64) {
    float d = x[c] - mean;
    v += d * d;
  }
  float rstd = rsqrtf(wave_sum(v) / W + eps);
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane; c < W; c += 64) {
    float gx = g[c] * (1.f - yy[c] * yy[c]);
    s1 += gx;
    s2 += gx * (x[c] - mean) * rstd;
  }
  s1 = wave_sum(s1) / W;
  s2 = wave_sum(s2) / W;
  for (int c = lane; c < W; c += 64) {
    float gx = g[c] * (1.f - yy[c] * yy[c]);
    float xh = (x[c] - mean) * rstd;
    gu[(long)row * W + c] = rstd * (gx - s1 - xh * s2);
  }
}

int layernorm_tanh_fwd_launch(const float* u, float* y, int rows, int W, float eps, hipStream_t s) {
  if (rows <= 0) return CGAT_OK;
  hipLaunchKernelGGL(layernorm_tanh_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, u, y, rows, W, eps);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// The same at W = 128, bit for bit.  One wave still reduces one row: lane k holds columns k and k + 64 of u, y and gy in
// registers (each loaded once), adds the two in that order wherever the kernel above loops over c = lane, lane + 64, and
// the xor butterfly 32 .. 1 of wave_sum follows.  A wave walks rows with a grid stride and requests the next row's six
// dwords before it reduces the present one, so two rows are in flight per wave; the grid is sized to the chip (LN128_WGS
// workgroups of four waves, rowops_grid.h: 32 waves per CU), not to rows / 4.
// The roundings are part of the contract and are pinned here (contraction off, fmaf where one rounding is meant); they are
// the ones hipcc gives the kernel above at two columns per lane:
//   s = (0 + x0) + x1;  d_k = x_k - mean;  v = fma(d1, d1, fma(d0, d0, 0));  rstd = rsqrtf(sum(v) / W + eps)
//   one_k = fma(-y_k, y_k, 1);  gx_k = g_k * one_k;  s1 = (0 + gx0) + gx1;  s2 = (0 + t0) + t1,  t_k = ((x_k - mean) * gx_k) * rstd
//   gu_k = rstd * fma(-s2, rstd * (x_k - mean), fma(g_k, one_k, -s1))        (s1, s2 the row means)
__device__ __forceinline__ float ln128_gu(float x, float yy, float g, float mean, float rstd, float s1, float s2) {
#pragma clang fp contract(off)
  const float one = __builtin_fmaf(-yy, yy, 1.f);
  const float xh = rstd * (x - mean);
  return rstd * __builtin_fmaf(-s2, xh, __builtin_fmaf(g, one, -s1));
}
struct Ln128Row {
  float x0, x1, y0, y1, g0, g1;
};
__device__ __forceinline__ Ln128Row ln128_load(const float* __restrict__ u, const float* __restrict__ y,
                                               const float* __restrict__ gy, long o) {
  return {u[o], u[o + 64], y[o], y[o + 64], gy[o], gy[o + 64]};
}
__device__ __forceinline__ float2 ln128_row(const Ln128Row& r, float eps) {
#pragma clang fp contract(off)
  constexpr int W = 128;
  float s = 0.f;
  s += r.x0;
  s += r.x1;
  const float mean = wave_sum(s) / W;
  const float d0 = r.x0 - mean, d1 = r.x1 - mean;
  const float v = __builtin_fmaf(d1, d1, __builtin_fmaf(d0, d0, 0.f));
  const float rstd = rsqrtf(wave_sum(v) / W + eps);
  const float gx0 = r.g0 * __builtin_fmaf(-r.y0, r.y0, 1.f), gx1 = r.g1 * __builtin_fmaf(-r.y1, r.y1, 1.f);
  float s1 = 0.f, s2 = 0.f;
  s1 += gx0;
  s2 += ((r.x0 - mean) * gx0) * rstd;
  s1 += gx1;
  s2 += ((r.x1 - mean) * gx1) * rstd;
  s1 = wave_sum(s1) / W;
  s2 = wave_sum(s2) / W;
  return make_float2(ln128_gu(r.x0, r.y0, r.g0, mean, rstd, s1, s2), ln128_gu(r.x1, r.y1, r.g1, mean, rstd, s1, s2));
}
__global__ __launch_bounds__(256) void layernorm_tanh_bwd128_kernel(const float* __restrict__ u, const float* __restrict__ y,
                                                                    const float* __restrict__ gy, float* __restrict__ gu,
                                                                    int rows, float eps) {
  constexpr int W = 128;
  const int lane = threadIdx.x & 63;
  const long stride = (long)gridDim.x * (blockDim.x >> 6);
  long ra = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (ra >= rows) return;
  // two register sets, a and b, in turn: the loads of one are requested before the other is reduced.  Loads and
  // arithmetic are unconditional and only the stores are guarded (a wave past its last row requests that row again and
  // drops the result), so that no load can be moved behind a branch, next to its first use
  Ln128Row a = ln128_load(u, y, gy, ra * W + lane);
  while (true) {
    const long rb = ra + stride;
    const Ln128Row b = ln128_load(u, y, gy, (rb < rows ? rb : ra) * W + lane);
    const float2 oa = ln128_row(a, eps);
    gu[ra * W + lane] = oa.x;
    gu[ra * W + lane + 64] = oa.y;
    const long rn = rb + stride;
    a = ln128_load(u, y, gy, (rn < rows ? rn : ra) * W + lane);
    const float2 ob = ln128_row(b, eps);
    if (rb < rows) {
      gu[rb * W + lane] = ob.x;
      gu[rb * W + lane + 64] = ob.y;
    }
    if (rn >= rows) break;
    ra = rn;
  }
}

int layernorm_tanh_bwd_launch(const float* u, const float* y, const float* gy, float* gu, int rows, int W, float eps,
                              hipStream_t s) {
  if (rows <= 0) return CGAT_OK;
  if (W == 128) {
    hipLaunchKernelGGL(layernorm_tanh_bwd128_kernel, dim3(ln128_wgs(rows)), dim3(256), 0, s, u, y, gy, gu, rows, eps);
    CGAT_LAUNCH_CHECK();
    return CGAT_OK;
  }
  hipLaunchKernelGGL(layernorm_tanh_bwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, s, u, y, gy, gu, rows, W, eps);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// derivative through an activation, expressed with the post-activation value y
__global__ void act_bwd_kernel(const float* __restrict__ y, const float* __restrict__ gy, float* __restrict__ gpre,
                               long n, int act) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float yv = y[i], g = gy[i];
    float d;
    switch (act) {
      case CGAT_ACT_TANH: d = 1.f - yv * yv; break;
      case CGAT_ACT_LEAKY: d = yv > 0.f ? 1.f : 0.01f; break;
      case CGAT_ACT_RELU: d = yv > 0.f ? 1.f : 0.f; break;
      default: d = 1.f;
    }
    gpre[i] = g * d;
  }
}

int act_bwd_launch(const float* y, const float* gy, float* gpre, long n, int act, hipStream_t s);
// the same with max |gpre| folded into gmax[0] (NOT zeroed here): the per-tensor scale the fp16 forms of the kernels
// that consume gpre need (vector-attention backward, edge_hidden_backward_impl); 16-byte vectors, n % 4 == 0
__global__ __launch_bounds__(256) void act_bwd_max_kernel(const float4* __restrict__ y, const float4* __restrict__ gy,
                                                          float4* __restrict__ gpre, long n4, float* __restrict__ gmax) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  float m = 0.f;
  for (; i < n4; i += stride) {
    const float4 yv = y[i], g = gy[i];
    const float4 r = make_float4(g.x * (yv.x > 0.f ? 1.f : 0.01f), g.y * (yv.y > 0.f ? 1.f : 0.01f),
                                 g.z * (yv.z > 0.f ? 1.f : 0.01f), g.w * (yv.w > 0.f ? 1.f : 0.01f));
    gpre[i] = r;
    m = fmaxf(fmaxf(m, fmaxf(fabsf(r.x), fabsf(r.y))), fmaxf(fabsf(r.z), fabsf(r.w)));
  }
  block_absmax_commit(m, gmax);
}

static inline int grid_for(long n) {
  long b = (n + 255) / 256;
  return (int)(b > 4096 ? 4096 : (b < 1 ? 1 : b));
}

// LeakyReLU backward + max |gpre| (gmax zeroed by the caller): the vector form alone.  act_bwd_leaky_max_fast says whether
// it applies; where it does not the caller runs act_bwd_launch and has no maximum
bool act_bwd_leaky_max_fast(const void* y, const void* gy, const void* gpre, long n) {
  return n > 0 && (n % 4) == 0 && ((((uintptr_t)y) | ((uintptr_t)gy) | ((uintptr_t)gpre)) & 15) == 0;
}
int act_bwd_leaky_max_launch(const float* y, const float* gy, float* gpre, long n, float* gmax, hipStream_t s) {
  CGAT_CHECK_ARG(act_bwd_leaky_max_fast(y, gy, gpre, n), "act_bwd_leaky_max: n = %ld or operands not 16-byte aligned", n);
  const long n4 = n / 4;
  long b = (n4 + 255) / 256;
  const int grid = (int)(b > 8192 ? 8192 : (b < 1 ? 1 : b));
  hipLaunchKernelGGL(act_bwd_max_kernel, dim3(grid), dim3(256), 0, s, (const float4*)y, (const float4*)gy, (float4*)gpre, n4,
                     gmax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

int act_bwd_launch(const float* y, const float* gy, float* gpre, long n, int act, hipStream_t s) {
  if (n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, s, y, gy, gpre, n, act);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- column sums: partial[chunk][c] over 128-row chunks, then a second pass of the same shape over the partials, until
// one chunk is left.  The summation order is fixed, hence deterministic, and the same in all three kernels below:
//   lane sum rl (0..3) of (chunk, column) = x[r0 + rl] + x[r0 + rl + 4] + ... in ascending row order, starting from 0.f;
//   partial[chunk][c] = alpha * (red[0] + red[1] + red[2] + red[3]), left to right.
// What differs is how threads map to (chunk, column, row lane). ----
// any shape: 64 columns x 4 row lanes per workgroup, one chunk per blockIdx.y
__global__ void colsum_partial_kernel(const float* __restrict__ x, long ldx, int rows, int cols,
                                      float* __restrict__ partial, float alpha) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int r0 = blockIdx.y * COLSUM_ROWS, r1 = min(rows, r0 + COLSUM_ROWS);
  float s = 0.f;
  if (c < cols)
    for (int r = r0 + rl; r < r1; r += 4) s += x[(long)r * ldx + c];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < cols) partial[(long)blockIdx.y * cols + c] = alpha * (red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
}
// narrow form (cols <= COLSUM_NARROW = 16, rowops_grid.h): the (chunk, column) pairs are numbered chunk * cols + c and a workgroup takes 64
// of them, so it covers 64 / cols chunks and all 256 threads have work.  The row lane is the LOW two bits of the thread
// index: one wave instruction reads four adjacent rows of 16 pairs.  Eight rows are requested before the first add.
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* __restrict__ x, long ldx, int rows, int cols,
                                                            long pairs, float* __restrict__ partial, float alpha) {
  __shared__ float red[4][64];
  const int rl = threadIdx.x & 3, sl = threadIdx.x >> 2;
  const long pair = (long)blockIdx.x * 64 + sl;
  float s = 0.f;
  if (pair < pairs) {
    const int chunk = (int)(pair / cols), c = (int)(pair % cols);
    const int r0 = chunk * COLSUM_ROWS, r1 = min(rows, r0 + COLSUM_ROWS);
    const float* xc = x + c;
    int r = r0 + rl;
    for (; r + 28 < r1; r += 32) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = xc[(long)(r + 4 * j) * ldx];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    for (; r < r1; r += 4) s += xc[(long)r * ldx];
  }
  red[rl][sl] = s;
  __syncthreads();
  if (rl == 0 && pair < pairs) partial[pair] = alpha * (red[0][sl] + red[1][sl] + red[2][sl] + red[3][sl]);
}
// wide form (cols % 4 == 0, ldx % 4 == 0, x and partial 16-byte aligned): a thread owns four adjacent columns and reads
// them as one 16-byte load per row.  The (chunk, column quad) pairs are numbered chunk * (cols / 4) + quad, 64 of them per
// workgroup; a wave is one row lane, so a wave instruction reads 1 KiB of one row where cols >= 256.  Eight rows are
// requested before the first add; each of the four columns keeps its own sum, in the order above.
__global__ __launch_bounds__(256) void colsum_wide_kernel(const float* __restrict__ x, long ldx, int rows, int quads,
                                                          long pairs, float* __restrict__ partial, float alpha) {
  __shared__ float4 red[4][64];
  const int sl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const long pair = (long)blockIdx.x * 64 + sl;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (pair < pairs) {
    const int chunk = (int)(pair / quads), q = (int)(pair % quads);
    const int r0 = chunk * COLSUM_ROWS, r1 = min(rows, r0 + COLSUM_ROWS);
    const float* xc = x + 4 * q;
    int r = r0 + rl;
    for (; r + 28 < r1; r += 32) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const float4*>(xc + (long)(r + 4 * j) * ldx);
#pragma unroll
      for (int j = 0; j < 8; ++j) { s.x += v[j].x; s.y += v[j].y; s.z += v[j].z; s.w += v[j].w; }
    }
    for (; r < r1; r += 4) {
      const float4 v = *reinterpret_cast<const float4*>(xc + (long)r * ldx);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[rl][sl] = s;
  __syncthreads();
  if (rl == 0 && pair < pairs) {
    const float4 a = red[0][sl], b = red[1][sl], c = red[2][sl], d = red[3][sl];
    reinterpret_cast<float4*>(partial)[pair] =
        make_float4(alpha * (a.x + b.x + c.x + d.x), alpha * (a.y + b.y + c.y + d.y), alpha * (a.z + b.z + c.z + d.z),
                    alpha * (a.w + b.w + c.w + d.w));
  }
}
size_t colsum_ws_bytes(int rows, int cols) {
  size_t c1 = colsum_chunks(rows), c2 = colsum_chunks((int)c1);
  return ws_round(c1 * cols, 4) + ws_round(c2 * cols, 4);
}
int colsum_launch(const float* x, long ldx, int rows, int cols, float* out, float alpha, void* ws, size_t ws_bytes,
                  hipStream_t s) {
  if (cols <= 0) return CGAT_OK;
  if (!ws || ws_bytes < colsum_ws_bytes(rows, cols)) {
    cgat_set_error("colsum: workspace too small");
    return CGAT_ERR_WORKSPACE;
  }
  float* bufs[2] = {(float*)ws, (float*)((char*)ws + ws_round((size_t)colsum_chunks(rows) * cols, 4))};
  const float* src = x;
  long ld = ldx;
  int n = rows > 0 ? rows : 0, level = 0;
  while (true) {
    int chunks = colsum_chunks(n);
    float* dst = chunks == 1 ? out : bufs[level & 1];
    const float a = level == 0 ? alpha : 1.f;
    const ColsumGrid g = colsum_grid(n, cols, ld, src, dst);
    switch (g.form) {
      case COLSUM_FORM_NARROW:
        hipLaunchKernelGGL(colsum_narrow_kernel, dim3(g.gx), dim3(256), 0, s, src, ld, n, cols, g.pairs, dst, a);
        break;
      case COLSUM_FORM_WIDE:
        hipLaunchKernelGGL(colsum_wide_kernel, dim3(g.gx), dim3(256), 0, s, src, ld, n, cols / 4, g.pairs, dst, a);
        break;
      default:
        hipLaunchKernelGGL(colsum_partial_kernel, dim3(g.gx, g.gy), dim3(256), 0, s, src, ld, n, cols, dst, a);
    }
    CGAT_LAUNCH_CHECK();
    if (chunks == 1) break;
    src = dst;
    ld = cols;
    n = chunks;
    ++level;
  }
  return CGAT_OK;
}

// ---- H_Net hyper input: out = d*a + (1-d)*b, d a device scalar ----
__global__ void mix_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ d,
                           float* __restrict__ out, long n) {
  float dv = d[0];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = dv * a[i] + (1.f - dv) * b[i];
}
int mix_launch(const float* a, const float* b, const float* d, float* out, long n, hipStream_t s) {
  if (n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(mix_kernel, dim3(grid_for(n)), dim3(256), 0, s, a, b, d, out, n);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ga = d*g ; gb += (1-d)*g ; gd = sum g*(a-b)   (block partials -> fixed-order final sum)
// The order is part of the contract: the grid is min(grid_for(n), 1024) workgroups of 256 threads, a thread's elements are
// i, i + stride, ... and it adds their g*(a-b) to its s in that order; wave_sum, then red[0]+red[1]+red[2]+red[3]; the
// workgroup partials are added as ((p[0]+p[1])+p[2])+...  The loop is unrolled by four: the loads of g, a, b, gb of four
// iterations are requested before the arithmetic of the first.  Roundings, pinned: ga = d * g;  gb = fma(1 - d, g, gb);
// s = fma(g, a - b, s).
template <bool GA, bool GB>
__global__ __launch_bounds__(256) void mix_bwd_kernel(const float* __restrict__ g, const float* __restrict__ a,
                                                      const float* __restrict__ b, const float* __restrict__ d,
                                                      float* __restrict__ ga, float* __restrict__ gb, long n,
                                                      float* __restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const float dv = d[0], dc = 1.f - dv;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  float s = 0.f;
  for (; i + 3 * stride < n; i += 4 * stride) {
    float gv[4], av[4], bv[4], gbv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      gv[j] = g[i + j * stride];
      av[j] = a[i + j * stride];
      bv[j] = b[i + j * stride];
      if (GB) gbv[j] = gb[i + j * stride];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (GA) ga[i + j * stride] = dv * gv[j];
      if (GB) gb[i + j * stride] = __builtin_fmaf(dc, gv[j], gbv[j]);
      s = __builtin_fmaf(gv[j], av[j] - bv[j], s);
    }
  }
  for (; i < n; i += stride) {
    float gv = g[i];
    if (GA) ga[i] = dv * gv;
    if (GB) gb[i] = __builtin_fmaf(dc, gv, gb[i]);
    s = __builtin_fmaf(gv, a[i] - b[i], s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// out = ((p[0]+p[1])+p[2])+... : the whole workgroup loads the partials, coalesced, into LDS (tiles of 1024), and thread 0
// adds them from there in index order
__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
  __shared__ float p[1024];
  float s = 0.f;
  for (int base = 0; base < n; base += 1024) {
    const int m = min(n - base, 1024);
    for (int i = threadIdx.x; i < m; i += blockDim.x) p[i] = partial[base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) s += p[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = s;
}
int mix_bwd_launch(const float* g, const float* a, const float* b, const float* d, float* ga, float* gb_accum,
                   float* gd, long n, void* ws, size_t ws_bytes, hipStream_t s) {
  const int blocks = mix_bwd_wgs(n);
  if (!ws || ws_bytes < (size_t)blocks * 4) {
    cgat_set_error("mix_bwd: workspace too small");
    return CGAT_ERR_WORKSPACE;
  }
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, g, a, b, d, ga, gb_accum, n, (float*)ws); };
  if (ga && gb_accum) launch(mix_bwd_kernel<true, true>);
  else if (ga) launch(mix_bwd_kernel<true, false>);
  else if (gb_accum) launch(mix_bwd_kernel<false, true>);
  else launch(mix_bwd_kernel<false, false>);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, (const float*)ws, blocks, gd);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

__global__ void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float alpha, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) y[i] += alpha * x[i];
}
int axpy_launch(float* y, const float* x, float alpha, long n, hipStream_t s) {
  if (n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(axpy_kernel, dim3(grid_for(n)), dim3(256), 0, s, y, x, alpha, n);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// out = alpha * x
__global__ void scale_kernel(const float* __restrict__ x, float alpha, float* __restrict__ out, long n4, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long j = i; j < n4; j += stride) {
    float4 v = reinterpret_cast<const float4*>(x)[j];
    v.x *= alpha; v.y *= alpha; v.z *= alpha; v.w *= alpha;
    reinterpret_cast<float4*>(out)[j] = v;
  }
  for (long j = 4 * n4 + i; j < n; j += stride) out[j] = alpha * x[j];
}
int scale_launch(const float* x, float alpha, float* out, long n, hipStream_t s) {
  if (n <= 0) return CGAT_OK;
  const bool vec = ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0;
  const long n4 = vec ? n / 4 : 0;
  hipLaunchKernelGGL(scale_kernel, dim3(grid_for(n4 > 0 ? n4 : n)), dim3(256), 0, s, x, alpha, out, n4, n);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

__global__ void copy2d_kernel(const float* __restrict__ src, long lds, float* __restrict__ dst, long ldd, int rows,
                              int cols) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)rows * cols;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    long r = i / cols, c = i % cols;
    dst[r * ldd + c] = src[r * lds + c];
  }
}
int copy2d_launch(const float* src, long lds, float* dst, long ldd, int rows, int cols, hipStream_t s) {
  long total = (long)rows * cols;
  if (total <= 0) return CGAT_OK;
  hipLaunchKernelGGL(copy2d_kernel, dim3(grid_for(total)), dim3(256), 0, s, src, lds, dst, ldd, rows, cols);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// up to four such copies in one launch (blockIdx.y = the job): the stacking of MH_A | MH_M first-layer weights and
// biases and the un-stacking of their gradients were four launches per pass (41 per 4-layer step)
// V4: every job's columns, leading dimensions and pointers are multiples of 16 bytes -- four floats per thread (the
// half projections that the bit form of the attention layer keeps are 0.5 GB at 83 340 atoms)
template <bool V4>
__global__ void copy2d_multi_kernel(Copy2DJobs j) {
  const Copy2DJob& b = j.job[blockIdx.y];
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int cols = V4 ? b.cols / 4 : b.cols;
  const long total = (long)b.rows * cols;
  const long stride = (long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const long r = i / cols, c = i % cols;
    if constexpr (V4)
      *reinterpret_cast<float4*>(b.dst + r * b.ldd + 4 * c) = *reinterpret_cast<const float4*>(b.src + r * b.lds + 4 * c);
    else
      b.dst[r * b.ldd + c] = b.src[r * b.lds + c];
  }
}
int copy2d_multi_launch(const Copy2DJobs& j, hipStream_t s) {
  long most = 0;
  bool v4 = true;
  for (int k = 0; k < j.n; ++k) {
    const Copy2DJob& b = j.job[k];
    most = (long)b.rows * b.cols > most ? (long)b.rows * b.cols : most;
    v4 = v4 && b.cols % 4 == 0 && b.lds % 4 == 0 && b.ldd % 4 == 0 && ((((uintptr_t)b.src) | ((uintptr_t)b.dst)) & 15) == 0;
  }
  if (j.n <= 0 || most <= 0) return CGAT_OK;
  if (v4) hipLaunchKernelGGL(copy2d_multi_kernel<true>, dim3(grid_for(most / 4), j.n), dim3(256), 0, s, j);
  else hipLaunchKernelGGL(copy2d_multi_kernel<false>, dim3(grid_for(most), j.n), dim3(256), 0, s, j);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// Also the library's memset: NO hipMemsetAsync anywhere in the library (round 4).  A 4-byte hipMemsetAsync captured into a
// hipGraph (cgat_amd.GraphedStep) was not reliably in effect before the kernel that followed it on the SECOND replay
// (ROCm 7.2, memory from the capture's private pool): the slot of a maximum kept the bits a later operator of the
// previous replay had left in the reused block, atomicMax compared against them, the operand scale came out wrong and the
// step returned NaN -- replay 0 and every eager run were fine.  The same zeroing as a kernel node replays bit-identically
// (tests/test_capture.py).
// The library's one slab sum: item t = blockIdx.y, i < count,
//   out[t][(i >> 7) * ldo + (i & 127)] = sum_z slabs[t * item_stride + z * stride + i],
// z = 0 .. n-1 in that order, starting from 0.f (what n accumulating passes over a zero-filled buffer produce, bit for
// bit); four independent loads per round trip, added in slab order.  ldo = 128: out[t][i].
__global__ void sum_slabs_kernel(const float* __restrict__ slabs, int n, long stride, long item_stride, long count,
                                 SlabSumOut o, long ldo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const float* sl = slabs + (long)blockIdx.y * item_stride + i;
  float s = 0.f;
  int z = 0;
  for (; z + 4 <= n; z += 4) {
    const float v0 = sl[(long)z * stride], v1 = sl[(long)(z + 1) * stride];
    const float v2 = sl[(long)(z + 2) * stride], v3 = sl[(long)(z + 3) * stride];
    s += v0; s += v1; s += v2; s += v3;
  }
  for (; z < n; ++z) s += sl[(long)z * stride];
  o.out[blockIdx.y][(i >> 7) * ldo + (i & 127)] = s;
}
int sum_slabs_batch_launch(const float* slabs, int n, long stride, long count, int items, long item_stride,
                           float* const* out, long ldo, hipStream_t s) {
  if (count <= 0 || items <= 0) return CGAT_OK;
  CGAT_CHECK_ARG(items <= SLAB_SUM_MAX, "sum_slabs: too many items");
  SlabSumOut o = {};
  for (int t = 0; t < items; ++t) o.out[t] = out[t];
  hipLaunchKernelGGL(sum_slabs_kernel, dim3(cdiv(count, 256), items), dim3(256), 0, s, slabs, n, stride, item_stride, count,
                     o, ldo);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
int sum_slabs_launch(const float* slabs, int n, long stride, float* out, long count, hipStream_t s) {
  return sum_slabs_batch_launch(slabs, n, stride, count, 1, 0, &out, 128, s);
}

__global__ void fill_kernel(float* __restrict__ p, float v, long n) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}
int fill_launch(float* p, float v, long n, hipStream_t s) {
  if (n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, v, n);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
