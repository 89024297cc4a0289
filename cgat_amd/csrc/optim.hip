// Fused multi-tensor optimiser steps and the losses: the per-step work after the hot path.
//   * AdamW   -- the reference's default optimiser: torch.optim.AdamW(lr, weight_decay) at
//                CGAT/lightning_module.py:328-331 (decoupled decay, bias-corrected moments, eps outside the sqrt)
//   * Adam    -- torch.optim.Adam(lr, weight_decay) at lightning_module.py:325-327: the same kernel with the decay
//                coupled into the gradient (L2) instead of applied to the parameter
//   * SGD     -- torch.optim.SGD(lr, weight_decay, momentum) at lightning_module.py:320-323 (dampening 0, no Nesterov)
//   * LAMB    -- CGAT/lambs.py:155-181 lamb_kernel as driven by JITLamb.step (226-262): no bias correction,
//                weight norm clamped to [0, 10], trust ratio = |w| / (|adam_step| + eps) with zero guards
//   * RobustL1 / RobustL2 -- CGAT/utils.py:30-47 (Lorentzian / Gaussian aleatoric losses), value and gradients
//   * loss + step metrics -- the criterion (robust or nn.L1Loss / nn.MSELoss, lightning_module.py:131-142), its gradients
//                and mae / rmse of the de-normalised prediction (lines 153-159, 240-243) in one one-workgroup launch
// One launch covers every parameter tensor: the host uploads a table of (param, grad, exp_avg, exp_avg_sq, n) and a
// list of (tensor, offset) chunks; a workgroup owns one chunk.  HBM-bound: 16 B read + 12 B written per parameter
// (Adam, AdamW), 12 + 8 (SGD with momentum), 8 + 4 (SGD without).
// LAMB needs two norms per tensor before the update: phase 1 updates the moments and writes per-chunk partial sums,
// a per-tensor reduction in chunk order (fixed -> deterministic) forms the trust ratio, phase 2 applies it.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "kernels.h"

#define MT_CHUNK 16384   // elements per workgroup

__device__ __forceinline__ float block_sum_256(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sh[wave] = v;
  __syncthreads();
  const float t = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return t;
}

// L2 = false: AdamW (decoupled decay on the parameter); L2 = true: Adam (decay added to the gradient before the moments)
template <bool L2>
__global__ __launch_bounds__(256) void adam_mt_kernel(const cgat_mt_tensor* __restrict__ tab,
                                                      const int32_t* __restrict__ ch_tensor,
                                                      const int64_t* __restrict__ ch_off, float lr, float beta1,
                                                      float beta2, float eps, float wd, float bc1, float bc2_sqrt) {
  const cgat_mt_tensor t = tab[ch_tensor[blockIdx.x]];
  const int64_t o = ch_off[blockIdx.x];
  const int64_t end = o + MT_CHUNK < t.n ? o + MT_CHUNK : t.n;
  const float step_size = lr / bc1;
  for (int64_t i = o + threadIdx.x; i < end; i += 256) {
    float g = t.g[i];
    float p = t.p[i];
    if (L2) g = g + wd * p;                             // grad.add(param, alpha=weight_decay)
    else p = p * (1.f - lr * wd);                       // decoupled weight decay
    float m = t.m[i];
    m = m + (g - m) * (1.f - beta1);                    // exp_avg.lerp_(grad, 1 - beta1)
    const float v = t.v[i] * beta2 + (1.f - beta2) * g * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p -= step_size * (m / denom);
    t.p[i] = p; t.m[i] = m; t.v[i] = v;
  }
}

// torch's first step sets buf = clone(g'); a zero-initialised buffer gives the same bits (momentum * 0 + g' = g'), so
// the kernel needs no first-step flag.  MOM = false: no buffer is read or written (t.m may be null).
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_mt_kernel(const cgat_mt_tensor* __restrict__ tab,
                                                     const int32_t* __restrict__ ch_tensor,
                                                     const int64_t* __restrict__ ch_off, float lr, float momentum,
                                                     float wd) {
  const cgat_mt_tensor t = tab[ch_tensor[blockIdx.x]];
  const int64_t o = ch_off[blockIdx.x];
  const int64_t end = o + MT_CHUNK < t.n ? o + MT_CHUNK : t.n;
  for (int64_t i = o + threadIdx.x; i < end; i += 256) {
    const float p = t.p[i];
    float g = t.g[i] + wd * p;                          // grad.add(param, alpha=weight_decay)
    if (MOM) {
      g = momentum * t.m[i] + g;                        // buf.mul_(momentum).add_(grad)
      t.m[i] = g;
    }
    t.p[i] = p - lr * g;
  }
}

// phase 1: moments, partial sums of |param|^2 and |adam_step|^2 per chunk
__global__ __launch_bounds__(256) void lamb_phase1_kernel(const cgat_mt_tensor* __restrict__ tab,
                                                          const int32_t* __restrict__ ch_tensor,
                                                          const int64_t* __restrict__ ch_off, float beta1, float beta2,
                                                          float eps, float wd, float* __restrict__ partial) {
  __shared__ float sh[4];
  const cgat_mt_tensor t = tab[ch_tensor[blockIdx.x]];
  const int64_t o = ch_off[blockIdx.x];
  const int64_t end = o + MT_CHUNK < t.n ? o + MT_CHUNK : t.n;
  float wn = 0.f, an = 0.f;
  for (int64_t i = o + threadIdx.x; i < end; i += 256) {
    const float g = t.g[i], p = t.p[i];
    const float m = t.m[i] * beta1 + (1.f - beta1) * g;
    const float v = t.v[i] * beta2 + (1.f - beta2) * (g * g);
    t.m[i] = m; t.v[i] = v;
    const float s = m / (sqrtf(v) + eps) + wd * p;
    wn += p * p;
    an += s * s;
  }
  wn = block_sum_256(wn, sh);
  an = block_sum_256(an, sh);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = wn; partial[2 * blockIdx.x + 1] = an; }
}

// one thread per tensor: chunks of a tensor are consecutive in the chunk list
__global__ void lamb_ratio_kernel(const int32_t* __restrict__ first_chunk, int n_tensors,
                                  const float* __restrict__ partial, float eps, float* __restrict__ ratio) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tensors) return;
  float wn = 0.f, an = 0.f;
  for (int c = first_chunk[t]; c < first_chunk[t + 1]; ++c) { wn += partial[2 * c]; an += partial[2 * c + 1]; }
  float weight_norm = fminf(fmaxf(sqrtf(wn), 0.f), 10.f);
  const float adam_norm = sqrtf(an);
  float r = weight_norm / (adam_norm + eps);
  if (weight_norm == 0.f) r = 1.f;
  if (adam_norm == 0.f) r = 1.f;
  ratio[t] = r;
}

__global__ __launch_bounds__(256) void lamb_phase2_kernel(const cgat_mt_tensor* __restrict__ tab,
                                                          const int32_t* __restrict__ ch_tensor,
                                                          const int64_t* __restrict__ ch_off, float lr, float eps,
                                                          float wd, const float* __restrict__ ratio) {
  const int ti = ch_tensor[blockIdx.x];
  const cgat_mt_tensor t = tab[ti];
  const int64_t o = ch_off[blockIdx.x];
  const int64_t end = o + MT_CHUNK < t.n ? o + MT_CHUNK : t.n;
  const float scale = lr * ratio[ti];
  for (int64_t i = o + threadIdx.x; i < end; i += 256) {
    const float p = t.p[i];
    const float s = t.m[i] / (sqrtf(t.v[i]) + eps) + wd * p;
    t.p[i] = p - scale * s;
  }
}

extern "C" int32_t cgat_mt_chunk_elems(void) { return MT_CHUNK; }

extern "C" int cgat_adamw_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off,
                               int32_t n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int64_t step, void* stream) {
  CGAT_CHECK_ARG(n_chunks >= 0 && step >= 1, "adamw_step: bad arguments");
  if (n_chunks == 0) return CGAT_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  CGAT_PROF("adamw", (hipStream_t)stream);
  hipLaunchKernelGGL(adam_mt_kernel<false>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_off,
                     lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2));
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

extern "C" int cgat_adam_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off,
                              int32_t n_chunks, float lr, float beta1, float beta2, float eps, float weight_decay,
                              int64_t step, void* stream) {
  CGAT_CHECK_ARG(n_chunks >= 0 && step >= 1, "adam_step: bad arguments");
  if (n_chunks == 0) return CGAT_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  CGAT_PROF("adam", (hipStream_t)stream);
  hipLaunchKernelGGL(adam_mt_kernel<true>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_off,
                     lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2));
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

extern "C" int cgat_sgd_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off,
                             int32_t n_chunks, float lr, float momentum, float weight_decay, void* stream) {
  CGAT_CHECK_ARG(n_chunks >= 0, "sgd_step: bad arguments");
  if (n_chunks == 0) return CGAT_OK;
  CGAT_PROF("sgd", (hipStream_t)stream);
  if (momentum != 0.f)
    hipLaunchKernelGGL(sgd_mt_kernel<true>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor,
                       chunk_off, lr, momentum, weight_decay);
  else
    hipLaunchKernelGGL(sgd_mt_kernel<false>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor,
                       chunk_off, lr, momentum, weight_decay);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

extern "C" int cgat_lamb_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off,
                              int32_t n_chunks, const int32_t* first_chunk, int32_t n_tensors, float lr, float beta1,
                              float beta2, float eps, float weight_decay, float* ws /* 2*n_chunks + n_tensors floats */,
                              void* stream) {
  CGAT_CHECK_ARG(n_chunks >= 0 && n_tensors >= 0, "lamb_step: bad arguments");
  if (n_chunks == 0) return CGAT_OK;
  float* partial = ws;
  float* ratio = ws + 2 * (size_t)n_chunks;
  hipStream_t s = (hipStream_t)stream;
  CGAT_PROF("lamb", s);
  hipLaunchKernelGGL(lamb_phase1_kernel, dim3(n_chunks), dim3(256), 0, s, table, chunk_tensor, chunk_off, beta1, beta2, eps,
                     weight_decay, partial);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(lamb_ratio_kernel, dim3(cdiv(n_tensors, 64)), dim3(64), 0, s, first_chunk, n_tensors, partial, eps,
                     ratio);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(lamb_phase2_kernel, dim3(n_chunks), dim3(256), 0, s, table, chunk_tensor, chunk_off, lr, eps,
                     weight_decay, ratio);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- robust losses: per-row loss terms and gradients (the mean and its 1/n factor are applied by the caller) ----
// kind 1: sqrt(2) |o - t| exp(-s) + s       kind 2: 0.5 (o - t)^2 exp(-2 s) + s
__global__ void robust_loss_kernel(const float* __restrict__ o, const float* __restrict__ s, const float* __restrict__ t,
                                   int n, int kind, float* __restrict__ loss, float* __restrict__ go,
                                   float* __restrict__ gs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float d = o[i] - t[i], ls = s[i];
  if (kind == 1) {
    const float e = expf(-ls), a = 1.41421356237309515f * fabsf(d) * e;   // np.sqrt(2.0) rounded to fp32 by the product
    loss[i] = a + ls;
    go[i] = 1.41421356237309515f * e * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    gs[i] = 1.f - a;
  } else {
    const float e = expf(-2.f * ls), a = 0.5f * d * d * e;
    loss[i] = a + ls;
    go[i] = d * e;
    gs[i] = 1.f - 2.f * a;
  }
}

extern "C" int cgat_robust_loss(const float* output, const float* log_std, const float* target, int32_t n, int32_t kind,
                                float* loss_terms, float* g_output, float* g_log_std, void* stream) {
  CGAT_CHECK_ARG(n >= 0 && (kind == 1 || kind == 2), "robust_loss: kind must be 1 (L1) or 2 (L2)");
  if (n == 0) return CGAT_OK;
  hipLaunchKernelGGL(robust_loss_kernel, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, output, log_std, target,
                     n, kind, loss_terms, g_output, g_log_std);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- criterion + step metrics in one launch (one workgroup: n is crystals per batch, 64 ... 50 000) ----
// t_n = (target - mean) / std, pred = o * std + mean.  kind 1 / 2: the robust terms above on (o, t_n); kind 3: |o - t_n|;
// kind 4: (o - t_n)^2.  go / gs are the gradients of the MEAN loss; out3 = {mean loss, mean |pred - target|,
// sqrt(mean (pred - target)^2)}.  Each thread strides over the rows and sums in double, the 256 partial sums are added
// in a fixed tree and rounded to fp32 once: deterministic, no atomics, independent of the order up to fp64 rounding.
// No contraction into FMAs here: every per-row product and difference is rounded as written (pred is torch's
// mul-then-add).  robust_loss_kernel is compiled under the compiler's default contraction, and as built today its
// gradients are unfused too, so go / gs of kinds 1 and 2 equal its gradients times 1/n bit for bit; that equality is
// a property of the build, pinned by tests/test_optim_family.py, not a guarantee of this kernel.
__global__ __launch_bounds__(256) void loss_metrics_kernel(const float* __restrict__ o, const float* __restrict__ s,
                                                           const float* __restrict__ t, int n, int kind, float mean,
                                                           float std, float* __restrict__ go, float* __restrict__ gs,
                                                           float* __restrict__ out3) {
#pragma clang fp contract(off)
  __shared__ double sh[3][256];
  const float inv_n = 1.f / (float)n;
  double sl = 0.0, sa = 0.0, sq = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float oi = o[i], ti = t[i];
    const float d = oi - (ti - mean) / std;
    const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    float l;
    if (kind == 1) {
      const float ls = s[i], e = expf(-ls), a = 1.41421356237309515f * fabsf(d) * e;
      l = a + ls;
      go[i] = (1.41421356237309515f * e * sgn) * inv_n;
      gs[i] = (1.f - a) * inv_n;
    } else if (kind == 2) {
      const float ls = s[i], e = expf(-2.f * ls), a = 0.5f * d * d * e;
      l = a + ls;
      go[i] = (d * e) * inv_n;
      gs[i] = (1.f - 2.f * a) * inv_n;
    } else if (kind == 3) {
      l = fabsf(d);
      go[i] = sgn * inv_n;
    } else {
      l = d * d;
      go[i] = (2.f * d) * inv_n;
    }
    const float err = (oi * std + mean) - ti;
    sl += (double)l;
    sa += (double)fabsf(err);
    sq += (double)err * (double)err;
  }
  sh[0][threadIdx.x] = sl; sh[1][threadIdx.x] = sa; sh[2][threadIdx.x] = sq;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out3[0] = (float)(sh[0][0] / (double)n);
    out3[1] = (float)(sh[1][0] / (double)n);
    out3[2] = (float)sqrt(sh[2][0] / (double)n);
  }
}

extern "C" int cgat_loss_metrics(const float* output, const float* log_std, const float* target, int32_t n, int32_t kind,
                                 float mean, float std, float* g_output, float* g_log_std, float* out3, void* stream) {
  CGAT_CHECK_ARG(n >= 1 && kind >= 1 && kind <= 4,
                 "loss_metrics: n >= 1 and kind 1 (RobustL1), 2 (RobustL2), 3 (L1) or 4 (L2)");
  CGAT_CHECK_ARG(output && target && g_output && out3 && (kind >= 3 || (log_std && g_log_std)),
                 "loss_metrics: null pointer");
  CGAT_PROF("loss_metrics", (hipStream_t)stream);
  hipLaunchKernelGGL(loss_metrics_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, output, log_std, target, n, kind,
                     mean, std, g_output, g_log_std, out3);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
