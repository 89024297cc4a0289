// Operand images: every kernel and launcher that lays an fp32 operand out in the form a matrix-core kernel reads -- three
// bf16 planes, two fp16 planes with a power-of-two scale, the f16x3c chunks with their 6-bit images -- and the maxima those
// scales come from.  The consumers are the hypernetwork contractions (bilinear.hip: bilinear_prepare_T and its batch
// form), the per-edge and dense-layer kernels (edgez.hip, edgebwd.hip), the layer chains (chain.hip) and the
// orchestrators (layers.hip).  The plane layout itself: plane_image_offset, mfma_bf16.h.
#include <stdlib.h>

#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

// sgn(a) T[a] (sgn = (-1)^a if alternate, else 1) split into three bf16 planes in the ring kernels' fragment order
// (plane_image_put, mfma_bf16.h); element (a, b, c) of the [NA,128,128] operand is src[a*sa + b*sb + c*sc].
// NP = 2: two fp16 planes of st sgn(a) T[a], st = 2^k from max |T| (pow2_scale); NP = 3: st = 1.  Item i < NA * 16384.
template <int NP>
__device__ __forceinline__ void prepare_T_item(const float* __restrict__ src, void* __restrict__ dst, long i, long sa,
                                               long sb, long sc, int alternate, float st) {
  // thread order follows the fastest source stride so that reads coalesce
  int a = (int)(i >> 14), b, c;
  if (sc == 1) { b = (int)((i >> 7) & 127); c = (int)(i & 127); }
  else { c = (int)((i >> 7) & 127); b = (int)(i & 127); }
  float v = src[a * sa + b * sb + c * sc];
  if (alternate && (a & 1)) v = -v;
  if constexpr (NP == 2) v *= st;
  plane_image_put<NP>(dst, a, b, c, v);
}
// F16: the two fp16 planes, 2^k from tmax[0] = max |T|
// blockIdx.y = head of a multi-head layer: source + head * s_head, image + head * image_elems (0, 0: one operand)
template <bool F16>
__global__ void prepare_T_bf16_kernel(const float* __restrict__ src, __bf16* __restrict__ dst, int NA, long sa, long sb,
                                      long sc, int alternate, const float* __restrict__ tmax, long s_head = 0,
                                      long image_elems = 0) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)NA * 128 * 128) return;
  float st = 1.f, it;
  if constexpr (F16) pow2_scale(tmax[0], st, it);
  prepare_T_item<F16 ? 2 : 3>(src + (long)blockIdx.y * s_head, dst + (long)blockIdx.y * image_elems, i, sa, sb, sc,
                              alternate, st);
}

// The same three-plane image (NA = 1, no sign alternation) for SEVERAL 128 x 128 weights in one launch: the operands of the
// dense-layer kernel (edgez.hip, linear128_launch) in the 24-bit modes -- the hypernetwork's linear terms prepared their
// weight per product: 12 launches of 4.5 us per predicted-layer block and direction (round 5: one launch).
// Element (k, o) of item i is src[i][o * sc[i] + k * sb[i]]; image i at dst + i * 24576 floats.
__global__ void prepare_T_bf16_batch_kernel(WPrepBatch b, __bf16* __restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;            // 16384 elements per item
  prepare_T_item<3>(b.src[blockIdx.y], dst + (size_t)blockIdx.y * 49152, i, 0, b.sb[blockIdx.y], b.sc[blockIdx.y], 0, 1.f);
}
int prepare_T_bf16_batch_launch(const WPrepBatch& b, float* dst, hipStream_t stream) {
  if (b.n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(prepare_T_bf16_batch_kernel, dim3(64, b.n), dim3(256), 0, stream, b, (__bf16*)dst);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// f16x3c (mfma_bf16.h): the prepared T of the contraction kernels' 24-bit form.  One chunk = (a, column half, pair of
// 16-column blocks) = everything the forward kernel needs for 32 output columns of one `a`, 25 KB contiguous:
//   [k-step s = b/32 (4)][plane: h, l (2)][cb2 (2)][lane 64 x 16 B]          two fp16 planes of 2^k sgn(a) T[a]  (16 KB)
//   [cb2 (2)][term: 0 t6, 1 h6, 2 l6 (3)][lane 64 x 16 B | lane 64 x 8 B]    6-bit images for the correction terms (9 KB)
// lane = 16 kg + c % 16 holds, per plane fragment, b = 32 s + 8 kg + j (j = 0..7) and, per 6-bit fragment, all 32 values
// b = 32 s + 8 kg + j <-> element 8 s + j: the order in which the contraction kernels hold their row operand.
// One thread per (a, column c, k-group kg).  max |T| (tmax) lies behind the last chunk.
__device__ __forceinline__ void prepare_T_f16c_item(const float* __restrict__ src, uint4* __restrict__ dst, long i, long sa,
                                                    long sb, long sc, int alternate, float tm) {
  // thread order follows the fastest source stride where it can: c fastest when sc == 1
  int a = (int)(i >> 9), c, kg;
  if (sc == 1) { c = (int)(i & 127); kg = (int)((i >> 7) & 3); }
  else { kg = (int)(i & 3); c = (int)((i >> 2) & 127); }
  float st, it;
  pow2_scale(tm, st, it);
  if (alternate && (a & 1)) st = -st;
  float v[32];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * s + j] = src[a * sa + (long)(32 * s + 8 * kg + j) * sb + c * sc] * st;
  const int half = c >> 6, cbp = (c & 63) >> 5, cb2 = (c >> 4) & 1, lane = 16 * kg + (c & 15);
  uint4* chunk = dst + (((long)a * 2 + half) * 2 + cbp) * F16C_CHUNK16;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float w[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = v[8 * s + j];
    bf16x8 h, l;
    split2_x8_f16(w, h, l);
    chunk[((s * 2 + 0) * 2 + cb2) * 64 + lane] = __builtin_bit_cast(uint4, h);
    chunk[((s * 2 + 1) * 2 + cb2) * 64 + lane] = __builtin_bit_cast(uint4, l);
  }
  frag6 l6, h6, t6;
  f16c_pack32(v, l6, h6, t6);
  unsigned* blk = reinterpret_cast<unsigned*>(chunk + 1024) + cb2 * 1152;
#pragma unroll
  for (int term = 0; term < 3; ++term) {
    const frag6& f = term == 0 ? t6 : (term == 1 ? h6 : l6);
    *reinterpret_cast<uint4*>(blk + term * 384 + lane * 4) = make_uint4(f.w[0], f.w[1], f.w[2], f.w[3]);
    *reinterpret_cast<uint2*>(blk + term * 384 + 256 + lane * 2) = make_uint2(f.w[4], f.w[5]);
  }
}
__global__ void prepare_T_f16c_kernel(const float* __restrict__ src, uint4* __restrict__ dst, int NA, long sa, long sb,
                                      long sc, int alternate, const float* __restrict__ tmax, int per_a = 0) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)NA * 512) return;
  prepare_T_f16c_item(src, dst, i, sa, sb, sc, alternate, tmax[per_a ? (int)(i >> 9) : 0]);   // per_a: one scale per block a
}
// Weight operands of the edge / dense kernels in the fp16 form: one workgroup per 128 x 128 block keeps the block in
// registers, takes its largest magnitude, and writes the two planes of 2^k W in the bf16 kernel's order with two planes
// per k-step; max |W| goes to *wmax (the consumer undoes 2^k per column block).  No atomics, no second pass, one launch.
// Element (k = b, c) of the block is src[b * sb + c * sc]; its planes are block 0 of the image at dst.
__device__ __forceinline__ void prepare_W_f16_block(const float* __restrict__ src, long sb, long sc, void* __restrict__ dst,
                                                    float* __restrict__ wmax) {
  __shared__ float wm[4];
  const int tid = threadIdx.x;
  float v[64];
  float m = 0.f;
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    const int i = r * 256 + tid;                 // thread order follows the fastest source stride
    int b, c;
    if (sc == 1) { b = i >> 7; c = i & 127; }
    else { c = i >> 7; b = i & 127; }
    v[r] = src[b * sb + c * sc];
    m = fmaxf(m, fabsf(v[r]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) wm[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  if (tid == 0) *wmax = m;
  float st, it;
  pow2_scale(m, st, it);
#pragma unroll
  for (int r = 0; r < 64; ++r) {
    const int i = r * 256 + tid;
    int b, c;
    if (sc == 1) { b = i >> 7; c = i & 127; }
    else { c = i >> 7; b = i & 127; }
    plane_image_put<2>(dst, 0, b, c, v[r] * st);
  }
}
// block a = blockIdx.x of [NA,128,128] (element (a, b, c) at src[a*sa + b*sb + c*sc]), max |W[a]| to wmax[a] behind the
// planes (blockIdx.y = head of a batch of weights: per-head source and image offsets, see prepare_W_f16_launch)
__global__ __launch_bounds__(256) void prepare_W_f16_kernel(const float* __restrict__ src, _Float16* __restrict__ dst,
                                                            long sa, long sb, long sc, float* __restrict__ wmax,
                                                            long s_head, long image_floats) {
  const int a = blockIdx.x;
  prepare_W_f16_block(src + (long)blockIdx.y * s_head + a * sa, sb, sc,
                      dst + (long)blockIdx.y * image_floats * 2 + (long)a * 32768,
                      wmax + (long)blockIdx.y * image_floats + a);
}
// Many 128 x 128 weights in ONE launch (a dense layer's own prepare is a single workgroup: 11 us of latency per layer,
// 48 layers per hypernetwork step): item i = (src, sb, sc) goes to dst + i * WPREP_IMAGE_FLOATS, wmax behind its planes.
__global__ __launch_bounds__(256) void prepare_W_f16_batch_kernel(WPrepBatch b, float* __restrict__ dst) {
  float* img = dst + (size_t)blockIdx.x * WPREP_IMAGE_FLOATS;
  prepare_W_f16_block(b.src[blockIdx.x], b.sb[blockIdx.x], b.sc[blockIdx.x], img, img + 16384);
}
int prepare_W_f16_batch_launch(const WPrepBatch& b, float* dst, hipStream_t stream) {
  if (b.n <= 0) return CGAT_OK;
  hipLaunchKernelGGL(prepare_W_f16_batch_kernel, dim3(b.n), dim3(256), 0, stream, b, dst);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
int prepare_W_f16_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, hipStream_t stream, int heads,
                         long s_head, long image_floats) {
  if (NA <= 0 || heads <= 0) return CGAT_OK;
  hipLaunchKernelGGL(prepare_W_f16_kernel, dim3(NA, heads), dim3(256), 0, stream, src, (_Float16*)dst, sa, sb, sc,
                     (float*)dst + (size_t)NA * 16384, s_head, image_floats);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// out[0] = max |.| over a [rows, 128] view with row stride ld (absmax_rows128) and the `tail` < 128 floats behind its
// last row (out[0] zeroed before; non-negative floats order like their bit patterns, and a maximum does not depend on
// the order it is taken in: deterministic)
__global__ void absmax_kernel(const float* __restrict__ src, long ld, long rows, int tail, float* __restrict__ out) {
  float m = absmax_rows128(src, ld, rows, blockIdx.x, gridDim.x);
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) m = fmaxf(m, fabsf(src[rows * ld + threadIdx.x]));
  block_absmax_commit(m, out);
}
int absmax_rows128_wgs_launch(const float* t, long ld, int rows, float* out, int wgs, hipStream_t stream) {
  hipLaunchKernelGGL(absmax_kernel, dim3(wgs), dim3(256), 0, stream, t, ld, (long)rows, 0, out);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
// max |t[n, 0..127]| over rows of stride ld folded into out[0] (NOT zeroed here)
int absmax_rows128_launch(const float* t, long ld, int rows, float* out, hipStream_t stream) {
  if (rows <= 0) return CGAT_OK;
  CGAT_CHECK_ARG((ld % 4) == 0 && (((uintptr_t)t) & 15) == 0, "absmax_rows128: rows must be 16-byte aligned");
  return absmax_rows128_wgs_launch(t, ld, rows, out, rows < 8192 ? (rows + 7) / 8 : 1024, stream);
}
int absmax_launch(const float* src, long n, float* out, hipStream_t stream) {
  CGAT_TRY(fill_launch(out, 0.f, 1, stream));   // (a kernel, not hipMemsetAsync: see fill_launch in rowops.hip)
  if (n <= 0) return CGAT_OK;
  CGAT_CHECK_ARG((((uintptr_t)src) & 15) == 0, "absmax: source must be 16-byte aligned");
  const int blocks = (int)(cdiv(n, 4 * 256) < 512 ? cdiv(n, 4 * 256) : 512);
  hipLaunchKernelGGL(absmax_kernel, dim3(blocks), dim3(256), 0, stream, src, 128l, n >> 7, (int)(n & 127), out);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// Row-gathered variant for operands whose k index is a row number: element (a, b, c) = rows[gather[128 a + b]][c]
// for 128 a + b < nrows, zero beyond (the last block is padded).
// F16: two fp16 planes of 2^k rows, 2^k from emax[0] = max |rows|
template <bool F16>
__global__ void prepare_T_bf16_rows_kernel(const float* __restrict__ rows, long ld, const int* __restrict__ gather,
                                           int nrows, uint4* __restrict__ dst, int NA, const float* __restrict__ emax) {
  // one thread per 16-byte fragment piece: (a, k-step s, kg, column c) -> the 8 rows t = 128 a + 32 s + 8 kg + j of
  // column c; lanes run over c, so the eight row reads are coalesced and the three stores are 16 B at 16-B pitch
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)NA * 16 * 128) return;
  const int c = (int)(i & 127), kg = (int)((i >> 7) & 3), s = (int)((i >> 9) & 3);
  const long a = i >> 11;
  const long t0 = a * 128 + 32 * s + 8 * kg;
  bf16x8 x1, x2, x3;
  float vv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long t = t0 + j;
    vv[j] = t < nrows ? rows[(gather ? (long)gather[t] : t) * ld + c] : 0.f;
  }
  if constexpr (F16) {
    float se, ie;
    pow2_scale(emax[0], se, ie);
#pragma unroll
    for (int j = 0; j < 8; ++j) vv[j] *= se;
    split2_x8_f16(vv, x1, x2);
  } else {
    split3_x8(vv, x1, x2, x3);
  }
  constexpr int NP = F16 ? 2 : 3;
  const long in = plane_image_offset<NP>(a, 32 * s + 8 * kg, c) / 8;   // j = 0: whole 16-byte pieces, 256 per plane
  dst[in] = __builtin_bit_cast(uint4, x1);
  dst[in + 256] = __builtin_bit_cast(uint4, x2);
  if constexpr (!F16) dst[in + 512] = __builtin_bit_cast(uint4, x3);
}

// emax != null: the fp16 form (two planes of 2^k rows, 2^k from emax[0])
int prepare_T_bf16_rows_launch(const float* rows, long ld, const int* gather, int nrows, void* dst, int NA,
                               hipStream_t stream, const float* emax) {
  long total = (long)NA * 16 * 128;
  if (total <= 0) return CGAT_OK;
  if (emax)
    hipLaunchKernelGGL(prepare_T_bf16_rows_kernel<true>, dim3(cdiv(total, 256)), dim3(256), 0, stream, rows, ld, gather,
                       nrows, (uint4*)dst, NA, emax);
  else
    hipLaunchKernelGGL(prepare_T_bf16_rows_kernel<false>, dim3(cdiv(total, 256)), dim3(256), 0, stream, rows, ld, gather, nrows,
                     (uint4*)dst, NA, emax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// The plane image of `heads` operands in one launch: head h reads src + h * s_head and writes (float*)dst + h *
// image_floats.  tmax == null: three bf16 planes; else the fp16 form with the maximum already known (tmax[0], device
// memory).  Strided sources.
int prepare_T_planes_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, int alternate,
                            hipStream_t stream, const float* tmax, int heads, long s_head, long image_floats) {
  const long total = (long)NA * 128 * 128;
  if (total <= 0 || heads <= 0) return CGAT_OK;
  const auto kernel = tmax ? prepare_T_bf16_kernel<true> : prepare_T_bf16_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(cdiv(total, 256), heads), dim3(256), 0, stream, src, (__bf16*)dst, NA, sa, sb, sc,
                     alternate, tmax, s_head, image_floats * 2);   // the kernel counts the image in 2-byte elements
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
// The six-pass image of edge_ge_launch's weight (alternate = 1) whose first nAb blocks -- the attention half of the
// rebuilt gZ rows, edgebwd.hip -- hold W'[128 a + b][c] = wA[128 a + b] * W[128 a + b][c] (ONE fp32 rounding, then the
// exact split) instead of W: the row operand of those blocks is then the stored bit of LeakyReLU' alone.  The last H
// workgroups form cs[h][c] = sgn * sum_b W'[h Hd + b][c] in a fixed order (eight runs of Hd / 8 columns, added 0..7),
// sgn = the sign the image gives the head's LAST block, i.e. the one the accumulators carry when the head is flushed.
__global__ __launch_bounds__(256) void prepare_T_bf16_attn_kernel(const float* __restrict__ src, __bf16* __restrict__ dst,
                                                                  int NA, long sa, long sb, long sc,
                                                                  const float* __restrict__ wA, int nAb, int Hd,
                                                                  float* __restrict__ cs, int nprep) {
  if ((int)blockIdx.x < nprep) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)NA * 128 * 128) return;
    int a = (int)(i >> 14), b, c;
    if (sc == 1) { b = (int)((i >> 7) & 127); c = (int)(i & 127); }
    else { c = (int)((i >> 7) & 127); b = (int)(i & 127); }
    float v = src[a * sa + b * sb + c * sc];
    if (a < nAb) v = __fmul_rn(wA[128 * a + b], v);
    if (a & 1) v = -v;
    plane_image_put<3>(dst, a, b, c, v);
    return;
  }
  __shared__ float run[8][128];
  const int h = blockIdx.x - nprep, k4 = threadIdx.x & 31, seg = threadIdx.x >> 5, per = Hd / 8;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < per; ++j) {
    const long col = (long)h * Hd + seg * per + j;
    const float w = wA[col];
    const float* p = src + (col >> 7) * sa + (col & 127) * sb + 4 * k4 * sc;
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] = __fadd_rn(s[u], __fmul_rn(w, p[u * sc]));
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) run[seg][4 * k4 + u] = s[u];
  __syncthreads();
  if (threadIdx.x < 128) {
    float t = run[0][threadIdx.x];
#pragma unroll
    for (int g = 1; g < 8; ++g) t = __fadd_rn(t, run[g][threadIdx.x]);
    const int a_last = ((h + 1) * Hd) / 128 - 1;
    cs[h * 128 + threadIdx.x] = (a_last & 1) ? -t : t;
  }
}
int prepare_T_bf16_attn_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, const float* wA, int H,
                               int Hd, float* cs, hipStream_t stream) {
  const long total = (long)NA * 128 * 128;
  if (total <= 0) return CGAT_OK;
  CGAT_CHECK_ARG(H > 0 && Hd % 128 == 0 && (long)H * Hd <= (long)NA * 128, "prepare_T_bf16_attn: H = %d, Hd = %d", H, Hd);
  const int nprep = (int)cdiv(total, 256);
  hipLaunchKernelGGL(prepare_T_bf16_attn_kernel, dim3(nprep + H), dim3(256), 0, stream, src, (__bf16*)dst, NA, sa, sb, sc,
                     wA, H * Hd / 128, Hd, cs, nprep);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
// fp16 form: the whole [NA,128,128] source is contiguous (any index order); max |T| goes behind the planes
int prepare_T_f16_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, int alternate,
                         hipStream_t stream) {
  long total = (long)NA * 128 * 128;
  if (total <= 0) return CGAT_OK;
  float* tmax = (float*)dst + total;
  CGAT_TRY(absmax_launch(src, total, tmax, stream));
  return prepare_T_planes_launch(src, dst, NA, sa, sb, sc, alternate, stream, tmax);
}

// f16x3c form (layout at prepare_T_f16c_kernel): NA * F16C_A_FLOATS floats, max |T| behind them; contiguous source
int prepare_T_f16c_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, int alternate,
                          hipStream_t stream) {
  const long total = (long)NA * 128 * 128;
  if (total <= 0) return CGAT_OK;
  float* tmax = (float*)dst + (size_t)NA * F16C_A_FLOATS;
  CGAT_TRY(absmax_launch(src, total, tmax, stream));
  hipLaunchKernelGGL(prepare_T_f16c_kernel, dim3(cdiv((long)NA * 512, 256)), dim3(256), 0, stream, src, (uint4*)dst, NA,
                     sa, sb, sc, alternate, (const float*)tmax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- the same for several [NA,128,128] tensors at once (the predicted layers of a hypernetwork: 4 x (memset + absmax +
// prepare) = 12 launches of ~8 us each with a dispatch gap between every pair -> 2 launches).  Maxima without atomics:
// stage 1 writes one partial maximum per workgroup, every workgroup of stage 2 folds the 64 partials of its tensor.
#define TPREP_PARTS 64
__global__ void absmax_partial_batch_kernel(TPrepBatch b, long total, float* __restrict__ part) {
  float m = absmax_rows128(b.src[blockIdx.y], 128, total >> 7, blockIdx.x, gridDim.x);   // total = NA * 16384
  __shared__ float wm[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.y * TPREP_PARTS + blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}
// the fp16 image (prepare_T_bf16_kernel<true>) of several tensors: blockIdx.y = tensor, its maximum folded from the partials
__global__ void prepare_T_f16_batch_kernel(TPrepBatch b, int NA, long sa, long sb, long sc, int alternate,
                                           const float* __restrict__ part) {
  float tm = part[blockIdx.y * TPREP_PARTS + (threadIdx.x & 63)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));
  const long total = (long)NA * 128 * 128;
  if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<float*>(b.dst[blockIdx.y])[total] = tm;   // behind the planes
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  float st, it;
  pow2_scale(tm, st, it);
  prepare_T_item<2>(b.src[blockIdx.y], b.dst[blockIdx.y], i, sa, sb, sc, alternate, st);
}
// the f16x3c image (prepare_T_f16c_kernel) of several tensors: blockIdx.y = tensor, its maximum folded from the partials
__global__ void prepare_T_f16c_batch_kernel(TPrepBatch b, int NA, long sa, long sb, long sc, int alternate,
                                            const float* __restrict__ part) {
  float tm = part[blockIdx.y * TPREP_PARTS + (threadIdx.x & 63)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) tm = fmaxf(tm, __shfl_xor(tm, o, 64));
  float* img = reinterpret_cast<float*>(b.dst[blockIdx.y]);
  if (blockIdx.x == 0 && threadIdx.x == 0) img[(size_t)NA * F16C_A_FLOATS] = tm;   // behind the last chunk
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)NA * 512) return;
  prepare_T_f16c_item(b.src[blockIdx.y], reinterpret_cast<uint4*>(img), i, sa, sb, sc, alternate, tm);
}
size_t bilinear_prepare_T_batch_ws_floats(int n) { return (size_t)(n > 0 ? n : 1) * TPREP_PARTS; }
// f16x3 / f16x3c modes, 128-wide interleaved layout only (returns CGAT_ERR_UNSUPPORTED otherwise: prepare one by one);
// dst[i]: bilinear_T_floats(...) floats each; part: bilinear_prepare_T_batch_ws_floats(n) floats
// does the batched form exist for these sources?  Host only: a caller that decides its route before its first launch asks
// this; bilinear_prepare_T_batch answers CGAT_ERR_UNSUPPORTED exactly where it says no.
bool bilinear_prepare_T_batch_takes(int n, const float* const* src, int n0, int n1, int n2, int perm1, int perm2) {
  const int dims[3] = {n0, n1, n2};
  static int off = -1;   // CGAT_NO_TPREP_BATCH=1 (debug): prepare the operands one by one
  if (off < 0) { const char* e = getenv("CGAT_NO_TPREP_BATCH"); off = (e && e[0] == '1') ? 1 : 0; }
  if (off || n < 1 || n > TPREP_MAX || !mode_f16_T() || !bilinear_T_interleaved(dims[perm1], dims[perm2])) return false;
  for (int i = 0; i < n; ++i)
    if ((((uintptr_t)src[i]) & 15) != 0) return false;
  return true;
}
int bilinear_prepare_T_batch(int n, const float* const* src, float* const* dst, int n0, int n1, int n2, int perm0,
                             int perm1, int perm2, float* part, hipStream_t stream, int alternate) {
  const int dims[3] = {n0, n1, n2};
  if (!bilinear_prepare_T_batch_takes(n, src, n0, n1, n2, perm1, perm2)) return CGAT_ERR_UNSUPPORTED;
  const long st[3] = {(long)n1 * n2, (long)n2, 1};
  const int NA = dims[perm0];
  const long total = (long)NA * 128 * 128;
  TPrepBatch b;
  b.n = n;
  for (int i = 0; i < n; ++i) { b.src[i] = src[i]; b.dst[i] = dst[i]; }
  hipLaunchKernelGGL(absmax_partial_batch_kernel, dim3(TPREP_PARTS, n), dim3(256), 0, stream, b, total, part);
  CGAT_LAUNCH_CHECK();
  if (mode_f16c())
    hipLaunchKernelGGL(prepare_T_f16c_batch_kernel, dim3(cdiv((long)NA * 512, 256), n), dim3(256), 0, stream, b, NA,
                       st[perm0], st[perm1], st[perm2], alternate, (const float*)part);
  else
    hipLaunchKernelGGL(prepare_T_f16_batch_kernel, dim3(cdiv(total, 256), n), dim3(256), 0, stream, b, NA, st[perm0],
                       st[perm1], st[perm2], alternate, (const float*)part);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

bool bilinear_T_interleaved(int NB, int NC) { return NB == 128 && NC == 128; }

// floats of workspace the prepared T occupies (the bf16 form stores three 2-byte planes, the fp16 form two and its scale,
// the f16x3c form the fp16 form + 18 bits per element of 6-bit images)
size_t bilinear_T_floats(int NA, int NB, int NC) {
  size_t n = (size_t)NA * NB * NC;
  if (!bilinear_T_interleaved(NB, NC) || !mode_split()) return n;
  if (mode_f16c()) return (size_t)NA * F16C_A_FLOATS + 4;
  return mode_f16() ? n + 4 : (n * 3 + 1) / 2;
}

size_t bilinear_T_floats_max(int NA, int NB, int NC) {   // the mode may change between a size query and the call
  const size_t n = (size_t)NA * NB * NC, a = n * 3 / 2 + 4, b = (size_t)NA * F16C_A_FLOATS + 4;
  return (bilinear_T_interleaved(NB, NC) && b > a) ? b : a;
}

// dst = src with its three indices permuted: dst dims are (n[perm0], n[perm1], n[perm2]).
// interleave != 0 (last dst dim == 128): column c of every dst row is stored at (c % 32) * 4 + c / 32.
__global__ void permute3_kernel(const float* __restrict__ src, float* __restrict__ dst, int n0, int n1, int n2,
                                int perm0, int perm1, int perm2, int interleave) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long total = (long)n0 * n1 * n2;
  if (i >= total) return;
  int dims[3] = {n0, n1, n2};
  int d1 = dims[perm1], d2 = dims[perm2];
  int zs = (int)(i % d2);              // stored position inside the dst row
  int z = interleave ? ((zs & 3) * 32 + (zs >> 2)) : zs;
  int y = (int)((i / d2) % d1);
  int x = (int)(i / ((long)d2 * d1));
  int idx[3];
  idx[perm0] = x; idx[perm1] = y; idx[perm2] = z;
  dst[i] = src[((long)idx[0] * n1 + idx[1]) * n2 + idx[2]];
}

int permute3_launch(const float* src, float* dst, int n0, int n1, int n2, int perm0, int perm1, int perm2,
                    int interleave, hipStream_t stream) {
  long total = (long)n0 * n1 * n2;
  if (total <= 0) return CGAT_OK;
  hipLaunchKernelGGL(permute3_kernel, dim3(cdiv(total, 256)), dim3(256), 0, stream, src, dst, n0, n1, n2, perm0, perm1,
                     perm2, interleave);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// The B operand of bilinear_rows for a [n0,n1,n2] tensor viewed with permuted indices.
int bilinear_prepare_T(const float* src, float* dst, int n0, int n1, int n2, int perm0, int perm1, int perm2,
                       hipStream_t stream) {
  int dims[3] = {n0, n1, n2};
  if (bilinear_T_interleaved(dims[perm1], dims[perm2]) && mode_split()) {
    long st[3] = {(long)n1 * n2, (long)n2, 1};   // source strides of dims 0, 1, 2
    if (mode_f16()) return prepare_T_f16_launch(src, dst, dims[perm0], st[perm0], st[perm1], st[perm2], 1, stream);
    if (mode_f16c()) return prepare_T_f16c_launch(src, dst, dims[perm0], st[perm0], st[perm1], st[perm2], 1, stream);
    return prepare_T_planes_launch(src, dst, dims[perm0], st[perm0], st[perm1], st[perm2], 1, stream);
  }
  return permute3_launch(src, dst, n0, n1, n2, perm0, perm1, perm2,
                         bilinear_T_interleaved(dims[perm1], dims[perm2]) ? 1 : 0, stream);
}
