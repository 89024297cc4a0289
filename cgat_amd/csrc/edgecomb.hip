// Head combination of the per-edge hypernetwork edge update (reference CGAT.py:214-223): the softmax over the HEADS of
// an edge (exp, sum over heads, one true division; no max-subtraction), the attention dropout's keep-mask, the product
// with the messages, the mean over the heads and the permutation back to the caller's edge order -- one kernel per
// direction instead of seven elementwise / reduction passes over [E, H, Co] tensors.
//
//   alpha[t,h,c'] = exp(sa[t,h,c']) / sum_h' exp(sa[t,h',c'])            c' = c (vector attention) or 0 (scalar)
//   out[perm[t], c] = (sum_h (alpha[t,h,c'] * keep[t,h,c']) * sm[t,h,c]) / H
//
// Backward recomputes alpha from sa (nothing but the inputs is saved); with g = g_out[perm[t], :] / H
//   g_sm[t,h,c]  = g[c] * (alpha_h * keep_h)
//   q_h[c']      = sum over the channels that share c' of g[c] * sm[t,h,c] * keep_h
//   g_sa[t,h,c'] = alpha_h * (q_h - sum_h' alpha_h' * q_h')
// For scalar attention the channel sum is a butterfly over the row's lane group (a fixed order, no atomics), and g_sa --
// E * H values, each a difference of Co-term dot products -- is formed in fp64 and rounded once.
//
// Work split: one group of next_pow2(Co / 4) lanes per row (a float4 of channels per lane), 256 / group rows per
// workgroup and grid-stride step, at most EC_MAX_BLOCKS workgroups.  The heads are a run-time count (<= EC_MAX_H)
// over an unrolled, guarded loop, so that the per-head values stay in registers.  Element offsets are 64-bit.
#include "kernels.h"

#define EC_THREADS 256
#define EC_MAX_BLOCKS 2048
#define EC_MAX_H 8

static __device__ __forceinline__ float4 ec_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
static __device__ __forceinline__ void ec_st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
static __device__ __forceinline__ float4 ec_exp4(float4 a) { return make_float4(expf(a.x), expf(a.y), expf(a.z), expf(a.w)); }
static __device__ __forceinline__ float4 ec_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
static __device__ __forceinline__ float4 ec_sub4(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
static __device__ __forceinline__ float4 ec_mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
static __device__ __forceinline__ float4 ec_div4(float4 a, float4 b) {
  return make_float4(__fdiv_rn(a.x, b.x), __fdiv_rn(a.y, b.y), __fdiv_rn(a.z, b.z), __fdiv_rn(a.w, b.w));
}
static __device__ __forceinline__ float4 ec_divs(float4 a, float s) {
  return make_float4(__fdiv_rn(a.x, s), __fdiv_rn(a.y, s), __fdiv_rn(a.z, s), __fdiv_rn(a.w, s));
}
static __device__ __forceinline__ float4 ec_muls(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
static __device__ __forceinline__ float4 ec_set4(float s) { return make_float4(s, s, s, s); }

// VEC: one logit per head and channel (aF == Co); otherwise one per head (aF == 1)
template <bool VEC>
__global__ __launch_bounds__(EC_THREADS) void edge_combine_fwd_kernel(const float* __restrict__ sa,
                                                                       const float* __restrict__ sm,
                                                                       const float* __restrict__ keep,
                                                                       const int* __restrict__ perm,
                                                                       float* __restrict__ out, long E, int H, int Co,
                                                                       int grp) {
  const int rows = EC_THREADS / grp;
  const int c = (threadIdx.x & (grp - 1)) * 4;
  if (c >= Co) return;                                   // lanes past the row's width (Co / 4 not a power of two)
  const float fH = (float)H;
  for (long t = (long)blockIdx.x * rows + threadIdx.x / grp; t < E; t += (long)gridDim.x * rows) {
    const long ms = t * H * Co + c;                      // sm[t, 0, c]
    const long as = VEC ? ms : t * H;                    // sa / keep[t, 0, c']
    float4 w[EC_MAX_H];                                  // exp(logit), then alpha * keep
    float4 den = ec_set4(0.f);
#pragma unroll
    for (int h = 0; h < EC_MAX_H; ++h) {
      if (h < H) {
        w[h] = VEC ? ec_exp4(ec_ld4(sa + as + (long)h * Co)) : ec_set4(expf(sa[as + h]));
        den = ec_add4(den, w[h]);
      }
    }
    float4 acc = ec_set4(0.f);
#pragma unroll
    for (int h = 0; h < EC_MAX_H; ++h) {
      if (h < H) {
        float4 a = ec_div4(w[h], den);
        if (keep) a = ec_mul4(a, VEC ? ec_ld4(keep + as + (long)h * Co) : ec_set4(keep[as + h]));
        acc = ec_add4(acc, ec_mul4(a, ec_ld4(sm + ms + (long)h * Co)));
      }
    }
    const long row = perm ? (long)perm[t] : t;
    ec_st4(out + row * Co + c, ec_divs(acc, fH));
  }
}

template <bool VEC>
__global__ __launch_bounds__(EC_THREADS) void edge_combine_bwd_kernel(const float* __restrict__ sa,
                                                                       const float* __restrict__ sm,
                                                                       const float* __restrict__ keep,
                                                                       const int* __restrict__ perm,
                                                                       const float* __restrict__ g_out,
                                                                       float* __restrict__ g_sa,
                                                                       float* __restrict__ g_sm, long E, int H, int Co,
                                                                       int grp) {
  const int rows = EC_THREADS / grp;
  const int lane = threadIdx.x & (grp - 1);
  const int c = lane * 4;
  const bool in_row = c < Co;
  const float fH = (float)H;
  // every lane of a wave walks the same number of steps: the scalar form's butterfly needs all lanes of a group
  const long steps = (E + (long)gridDim.x * rows - 1) / ((long)gridDim.x * rows);
  for (long it = 0; it < steps; ++it) {
    const long t = (it * gridDim.x + blockIdx.x) * rows + threadIdx.x / grp;
    const bool live = in_row && t < E;
    const long ms = live ? t * H * Co + c : 0;
    const long as = live ? (VEC ? ms : t * H) : 0;
    float4 g = ec_set4(0.f);
    if (live) g = ec_divs(ec_ld4(g_out + (perm ? (long)perm[t] : t) * Co + c), fH);
    float4 w[EC_MAX_H];                                  // exp(logit), then alpha
    float4 den = ec_set4(0.f);
#pragma unroll
    for (int h = 0; h < EC_MAX_H; ++h) {
      if (h < H) {
        w[h] = ec_set4(1.f);
        if (live) w[h] = VEC ? ec_exp4(ec_ld4(sa + as + (long)h * Co)) : ec_set4(expf(sa[as + h]));
        den = ec_add4(den, w[h]);
      }
    }
    if constexpr (VEC) {
      float4 q[EC_MAX_H];
      float4 S = ec_set4(0.f);                           // sum_h alpha_h q_h
#pragma unroll
      for (int h = 0; h < EC_MAX_H; ++h) {
        if (h < H) {
          w[h] = ec_div4(w[h], den);
          if (live) {
            const float4 m = ec_ld4(sm + ms + (long)h * Co);
            float4 ak = w[h];
            q[h] = ec_mul4(g, m);
            if (keep) {
              const float4 k = ec_ld4(keep + as + (long)h * Co);
              ak = ec_mul4(ak, k);
              q[h] = ec_mul4(q[h], k);
            }
            if (g_sm) ec_st4(g_sm + ms + (long)h * Co, ec_mul4(g, ak));
            S = ec_add4(S, ec_mul4(w[h], q[h]));
          }
        }
      }
      if (!g_sa || !live) continue;
#pragma unroll
      for (int h = 0; h < EC_MAX_H; ++h)
        if (h < H) ec_st4(g_sa + as + (long)h * Co, ec_mul4(w[h], ec_sub4(q[h], S)));
    } else {
      // One logit per head: its gradient alpha_h (q_h - sum alpha q) is a difference of Co-term dot products.  The dot
      // products, the softmax they are weighted with and the difference are formed in fp64 and rounded once -- E * H
      // values, no memory traffic of their own -- so that the result carries the rounding of its inputs and of the
      // final store only.  Where the fp32 softmax of the forward is not finite (a logit past exp's range: no
      // max-subtraction), the row's logit gradient is NaN, as the forward's row is.
      const bool finite = den.x > 0.f && den.x < __builtin_inff();
      double ad[EC_MAX_H], qd[EC_MAX_H];
      double dend = 0.0;
#pragma unroll
      for (int h = 0; h < EC_MAX_H; ++h) {
        if (h < H) {
          ad[h] = live ? exp((double)sa[as + h]) : 1.0;
          dend += ad[h];
        }
      }
      double gd[4] = {0.0, 0.0, 0.0, 0.0};
      if (live) {
        const float4 go = ec_ld4(g_out + (perm ? (long)perm[t] : t) * Co + c);
        gd[0] = (double)go.x / H; gd[1] = (double)go.y / H; gd[2] = (double)go.z / H; gd[3] = (double)go.w / H;
      }
      double S = 0.0;
#pragma unroll
      for (int h = 0; h < EC_MAX_H; ++h) {
        if (h < H) {
          w[h] = ec_div4(w[h], den);
          ad[h] = ad[h] / dend;
          const float k = (keep && live) ? keep[as + h] : 1.f;
          double d = 0.0;
          if (live) {
            const float4 m = ec_ld4(sm + ms + (long)h * Co);
            if (g_sm) ec_st4(g_sm + ms + (long)h * Co, ec_muls(g, keep ? w[h].x * k : w[h].x));
            d = (gd[0] * m.x + gd[1] * m.y) + (gd[2] * m.z + gd[3] * m.w);
          }
          for (int o = grp >> 1; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);     // fixed order: bitwise reproducible
          qd[h] = keep ? d * k : d;
          S += ad[h] * qd[h];
        }
      }
      if (!g_sa || !live || lane != 0) continue;
#pragma unroll
      for (int h = 0; h < EC_MAX_H; ++h)
        if (h < H) g_sa[as + h] = finite ? (float)(ad[h] * (qd[h] - S)) : __builtin_nanf("");
    }
  }
}

bool edge_combine_ok(int H, int aF, int Co) {
  return Co > 0 && Co % 4 == 0 && Co <= 256 && H >= 1 && H <= EC_MAX_H && (aF == 1 || aF == Co);
}
static int ec_group(int Co) {
  int g = 1;
  while (g < Co / 4) g <<= 1;
  return g;
}
static unsigned ec_grid(long E, int grp) {
  const long need = (E + EC_THREADS / grp - 1) / (EC_THREADS / grp);
  return (unsigned)(need < EC_MAX_BLOCKS ? need : EC_MAX_BLOCKS);
}
static bool ec_aligned(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int edge_combine_fwd_launch(const float* sa, int aF, const float* sm, const float* keep, const int* perm, long E, int H,
                            int Co, float* out, hipStream_t s) {
  CGAT_CHECK_ARG(E >= 0, "edge_head_combine: negative edge count");
  if (E == 0) return CGAT_OK;
  CGAT_CHECK_ARG(edge_combine_ok(H, aF, Co), "edge_head_combine: unsupported shape (H=%d, aF=%d, Co=%d)", H, aF, Co);
  CGAT_CHECK_ARG(sa && sm && out, "edge_head_combine: null operand");
  const bool vec = aF != 1;
  CGAT_CHECK_ARG(ec_aligned(sm) && ec_aligned(out) && (!vec || (ec_aligned(sa) && ec_aligned(keep))),
                 "edge_head_combine: operands must be 16-byte aligned");
  const int grp = ec_group(Co);
  CGAT_PROF("edge_combine", s);
  if (vec)
    hipLaunchKernelGGL(edge_combine_fwd_kernel<true>, dim3(ec_grid(E, grp)), dim3(EC_THREADS), 0, s, sa, sm, keep, perm,
                       out, E, H, Co, grp);
  else
    hipLaunchKernelGGL(edge_combine_fwd_kernel<false>, dim3(ec_grid(E, grp)), dim3(EC_THREADS), 0, s, sa, sm, keep, perm,
                       out, E, H, Co, grp);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

int edge_combine_bwd_launch(const float* sa, int aF, const float* sm, const float* keep, const int* perm,
                            const float* g_out, long E, int H, int Co, float* g_sa, float* g_sm, hipStream_t s) {
  CGAT_CHECK_ARG(E >= 0, "edge_head_combine backward: negative edge count");
  if (E == 0 || (!g_sa && !g_sm)) return CGAT_OK;
  CGAT_CHECK_ARG(edge_combine_ok(H, aF, Co), "edge_head_combine backward: unsupported shape (H=%d, aF=%d, Co=%d)", H, aF,
                 Co);
  CGAT_CHECK_ARG(sa && sm && g_out, "edge_head_combine backward: null operand");
  const bool vec = aF != 1;
  CGAT_CHECK_ARG(ec_aligned(sm) && ec_aligned(g_out) && ec_aligned(g_sm) &&
                     (!vec || (ec_aligned(sa) && ec_aligned(keep) && ec_aligned(g_sa))),
                 "edge_head_combine backward: operands must be 16-byte aligned");
  const int grp = ec_group(Co);
  CGAT_PROF("edge_combine", s);
  if (vec)
    hipLaunchKernelGGL(edge_combine_bwd_kernel<true>, dim3(ec_grid(E, grp)), dim3(EC_THREADS), 0, s, sa, sm, keep, perm,
                       g_out, g_sa, g_sm, E, H, Co, grp);
  else
    hipLaunchKernelGGL(edge_combine_bwd_kernel<false>, dim3(ec_grid(E, grp)), dim3(EC_THREADS), 0, s, sa, sm, keep, perm,
                       g_out, g_sa, g_sm, E, H, Co, grp);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
