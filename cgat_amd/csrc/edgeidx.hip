// Per-edge phase of the scalar-attention forward without grad when edge_attr is a table lookup: edge_attr[e] = table[idx[e]]
// with R rows (the shell embedding and every edge update of the shipped network: DESIGN.md section 4).  The edge term of
// the pre-activation is then one of R rows of Te = table W_e^T [R, W2], formed once, and
//     z[t, :] = Te[idx[perm[t]], :] + Pi[dst[t], :] + Pj[src[t], :]                (destination-sorted slot t)
// is a sum of three gathered rows: no matrix instruction on the per-edge path (reference CGAT.py:319-329).
//
//   edge_idx_logits   a[t,h]      = b_A[h] + sum_c wA[h,c] leaky(z[t, h Hd + c])                  (attention columns)
//   edge_idx_wsum     S[n,(h,c)]  = sum_{t -> n} alpha[t,h] leaky(z[t, H Hd + h Hd + c])          (message columns)
//
// Both give every destination segment to one wave: Pi[n] is read once per segment and stays in registers, the Pj / Te rows
// of IDX_U slots are in flight together, and each S element is one chain fma(leaky(z), alpha, acc) over its segment in
// ascending t.  Segments above SEG_LONG rows are left to the workgroups behind the ordinary ones: the 16 waves of such a
// workgroup take rows r0 + g, r0 + g + 16, ... of ONE segment and their partial sums are added through LDS in wave order
// -- a fixed split, so the results do not depend on the launch shape.  No atomics on memory, no workspace.
#include "common.h"
#include "kernels.h"

#define IDX_THREADS 1024
#define IDX_WAVES 16      // waves per workgroup = segments per ordinary workgroup = row groups of a long segment
#define IDX_U 4           // slots in flight per wave

__device__ __forceinline__ float idx_wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float idx_leaky(float v) { return v > 0.f ? v : 0.01f * v; }
__device__ __forceinline__ float4 idx_ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// table row of slot t, clamped into [0, R): the Python surface validates the index once per object; with validation
// switched off a bad value must still stay inside the table
__device__ __forceinline__ size_t idx_row(const int64_t* __restrict__ idx, const int* __restrict__ perm, int t, int R) {
  const int64_t r = idx[perm[t]];
  return (size_t)(r < 0 ? 0 : (r >= R ? R - 1 : r));
}

// the long segments among segments [T b, T b + T) for workgroups of T threads: ids into list[] (LDS); each is processed on its own, so the
// order of the list does not reach any result
__device__ __forceinline__ int idx_collect_long(const int* __restrict__ rowptr, int N, int* list, int* count, int b) {
  if (threadIdx.x == 0) *count = 0;
  __syncthreads();
  const int s = b * (int)blockDim.x + (int)threadIdx.x;
  if (s < N && rowptr[s + 1] - rowptr[s] > SEG_LONG) list[atomicAdd(count, 1)] = s;
  __syncthreads();
  return *count;
}

// Logits of slots t0, t0 + step, ... < t1 of destination n, by one wave.  Lane l owns column quads 64 k + l (k < KQ) of
// the attention half; quad q lies in head 4 q / Hd (Hd % 4 == 0).
template <int KQ>
__device__ __forceinline__ void idx_logits_rows(const float* __restrict__ Te, int R, const int64_t* __restrict__ idx,
                                                const int* __restrict__ perm, const float* __restrict__ Pi,
                                                const float* __restrict__ Pj, const int* __restrict__ srci, long W2,
                                                const float* __restrict__ wA, const float* __restrict__ bA, int H, int Hd,
                                                int HHd, int n, int t0, int t1, int step, float* __restrict__ a) {
  constexpr int U = KQ <= 2 ? 4 : (KQ <= 4 ? 2 : 1);
  const int lane = threadIdx.x & 63;
  float4 pi[KQ], w[KQ];
  int head[KQ];
#pragma unroll
  for (int k = 0; k < KQ; ++k) {
    const int f = 4 * (64 * k + lane);
    const bool live = f < HHd;
    pi[k] = live ? idx_ld4(Pi + (size_t)n * W2 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    w[k] = live ? idx_ld4(wA + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    head[k] = live ? f / Hd : -1;
  }
  for (int t = t0; t < t1; t += U * step) {
    float4 te[U][KQ], pj[U][KQ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tt = t + u * step < t1 ? t + u * step : t1 - 1;   // (clamped: a valid slot of this segment)
      const float* ter = Te + idx_row(idx, perm, tt, R) * W2;
      const float* pjr = Pj + (size_t)srci[tt] * W2;
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        const int f = 4 * (64 * k + lane);
        const bool live = f < HHd;
        te[u][k] = live ? idx_ld4(ter + f) : make_float4(0.f, 0.f, 0.f, 0.f);
        pj[u][k] = live ? idx_ld4(pjr + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t + u * step >= t1) break;                               // (wave-uniform)
      float p[KQ];
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        // the three terms in the dense route's order: part + Pi + Pj
        float s = w[k].x * idx_leaky(te[u][k].x + pi[k].x + pj[u][k].x);
        s = fmaf(w[k].y, idx_leaky(te[u][k].y + pi[k].y + pj[u][k].y), s);
        s = fmaf(w[k].z, idx_leaky(te[u][k].z + pi[k].z + pj[u][k].z), s);
        s = fmaf(w[k].w, idx_leaky(te[u][k].w + pi[k].w + pj[u][k].w), s);
        p[k] = s;
      }
      for (int h = 0; h < H; ++h) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KQ; ++k) v += head[k] == h ? p[k] : 0.f;
        v = idx_wave_sum64(v);
        if (lane == 0) a[(size_t)(t + u * step) * H + h] = v + bA[h];
      }
    }
  }
}

// (more than 4 x 64 quads per lane set: 8 waves per workgroup, for the 256 registers that Pi, wA and one slot's rows take.
// A logit is one slot's own sum, so the number of waves reaches no result.)
template <int KQ>
constexpr int idx_logits_waves() { return KQ <= 4 ? IDX_WAVES : IDX_WAVES / 2; }
template <int KQ>
__global__ __launch_bounds__(64 * idx_logits_waves<KQ>()) void edge_idx_logits_kernel(
    const float* __restrict__ Te, int R, const int64_t* __restrict__ idx, const int* __restrict__ perm,
    const float* __restrict__ Pi, const float* __restrict__ Pj, const int* __restrict__ srci, long W2,
    const float* __restrict__ wA, const float* __restrict__ bA, int H, int Hd, const int* __restrict__ rowptr, int N,
    int main_blocks, float* __restrict__ a) {
  constexpr int WAVES = idx_logits_waves<KQ>();
  const int wave = threadIdx.x >> 6, HHd = H * Hd;
  if ((int)blockIdx.x < main_blocks) {
    const int n = blockIdx.x * WAVES + wave;
    if (n >= N) return;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 > SEG_LONG || r1 <= r0) return;      // long: the workgroups behind; empty: no logits
    idx_logits_rows<KQ>(Te, R, idx, perm, Pi, Pj, srci, W2, wA, bA, H, Hd, HHd, n, r0, r1, 1, a);
    return;
  }
  __shared__ int list[IDX_THREADS];
  __shared__ int count;
  const int nl = idx_collect_long(rowptr, N, list, &count, blockIdx.x - main_blocks);
  for (int k = 0; k < nl; ++k) {
    const int n = list[k], r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r0 + wave < r1)
      idx_logits_rows<KQ>(Te, R, idx, perm, Pi, Pj, srci, W2, wA, bA, H, Hd, HHd, n, r0 + wave, r1, WAVES, a);
  }
}

// Weighted sum over slots t0, t0 + step, ... < t1 of destination n for this lane's column quad f of the message half
// (Pi, Pj, Te point at column H Hd of their rows): the chain in ascending t.  live == false: nothing is read.
__device__ __forceinline__ float4 idx_wsum_rows(const float* __restrict__ Te, int R, const int64_t* __restrict__ idx,
                                                const int* __restrict__ perm, const float* __restrict__ Pi,
                                                const float* __restrict__ Pj, const int* __restrict__ srci, long W2,
                                                const float* __restrict__ alpha, int H, int h, int f, bool live, int n,
                                                int t0, int t1, int step) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!live) return acc;
  const float4 pi = idx_ld4(Pi + (size_t)n * W2 + f);
  for (int t = t0; t < t1; t += IDX_U * step) {
    float4 te[IDX_U], pj[IDX_U];
    float al[IDX_U];
#pragma unroll
    for (int u = 0; u < IDX_U; ++u) {
      const int tt = t + u * step < t1 ? t + u * step : t1 - 1;
      te[u] = idx_ld4(Te + idx_row(idx, perm, tt, R) * W2 + f);
      pj[u] = idx_ld4(Pj + (size_t)srci[tt] * W2 + f);
      al[u] = alpha[(size_t)tt * H + h];
    }
#pragma unroll
    for (int u = 0; u < IDX_U; ++u)
      if (t + u * step < t1) {
        acc.x = fmaf(idx_leaky(te[u].x + pi.x + pj[u].x), al[u], acc.x);
        acc.y = fmaf(idx_leaky(te[u].y + pi.y + pj[u].y), al[u], acc.y);
        acc.z = fmaf(idx_leaky(te[u].z + pi.z + pj[u].z), al[u], acc.z);
        acc.w = fmaf(idx_leaky(te[u].w + pi.w + pj[u].w), al[u], acc.w);
      }
  }
  return acc;
}

__global__ __launch_bounds__(IDX_THREADS) void edge_idx_wsum_kernel(
    const float* __restrict__ Te, int R, const int64_t* __restrict__ idx, const int* __restrict__ perm,
    const float* __restrict__ Pi, const float* __restrict__ Pj, const int* __restrict__ srci, long W2,
    const float* __restrict__ alpha, int H, int Hd, const int* __restrict__ rowptr, int N, int main_blocks,
    float* __restrict__ S) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, HHd = H * Hd;
  const int chunks = (HHd + 255) / 256;              // 64 column quads per wave and pass
  if ((int)blockIdx.x < main_blocks) {
    const int n = blockIdx.x * IDX_WAVES + wave;
    if (n >= N) return;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 > SEG_LONG) return;                  // the workgroups behind
    for (int k = 0; k < chunks; ++k) {               // (an empty segment writes zeros)
      const int f = 4 * (64 * k + lane);
      if (f >= HHd) continue;
      const float4 acc = idx_wsum_rows(Te, R, idx, perm, Pi, Pj, srci, W2, alpha, H, f / Hd, f, true, n, r0, r1, 1);
      *reinterpret_cast<float4*>(S + (size_t)n * HHd + f) = acc;
    }
    return;
  }
  __shared__ int list[IDX_THREADS];
  __shared__ int count;
  __shared__ float4 part[IDX_THREADS];
  const int nl = idx_collect_long(rowptr, N, list, &count, blockIdx.x - main_blocks);
  for (int j = 0; j < nl; ++j) {
    const int n = list[j], r0 = rowptr[n], r1 = rowptr[n + 1];
    for (int k = 0; k < chunks; ++k) {               // (uniform trip count: the barriers below)
      const int f = 4 * (64 * k + lane);
      const bool live = f < HHd;
      const float4 acc = idx_wsum_rows(Te, R, idx, perm, Pi, Pj, srci, W2, alpha, H, live ? f / Hd : 0, f, live, n, r0 + wave,
                                       r1, IDX_WAVES);
      __syncthreads();
      part[threadIdx.x] = acc;
      __syncthreads();
      if (wave == 0 && live) {
        float4 t = part[lane];
        for (int g = 1; g < IDX_WAVES; ++g) {        // wave order
          const float4 o = part[g * 64 + lane];
          t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        *reinterpret_cast<float4*>(S + (size_t)n * HHd + f) = t;
      }
    }
  }
}

// Shapes both launches take: whole column quads inside one head, at most 8 x 64 quads per half, 64-bit row offsets (no
// bound on N * W2).  Host only.
bool edge_idx_ok(int H, int Hd, int R) {
  return H >= 1 && H <= 8 && Hd >= 4 && Hd % 4 == 0 && (long)H * Hd <= 2048 && R >= 1 && R <= EDGE_IDX_MAX_ROWS;
}

static bool idx_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0;
}

int edge_idx_logits_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                           const int* srci, int W2, const float* wA, const float* bA, int H, int Hd, const int* rowptr,
                           int N, int E, float* a, hipStream_t stream) {
  CGAT_CHECK_ARG(W2 == 2 * H * Hd && edge_idx_ok(H, Hd, R) && idx && perm && srci && rowptr && a && bA &&
                 idx_aligned16(Te, Pi, Pj, wA),
                 "edge_idx_logits: needs Hd %% 4 == 0, H <= 8, H * Hd <= 2048 and 16-byte aligned rows and fc_out_A's weight");
  if (N <= 0 || E <= 0) return CGAT_OK;
  const int KQ = cdiv(H * Hd, 256);
  CGAT_PROF("edge_idx_logits", stream);
#define IDX_LOGITS(K)                                                                                                    \
  case K: {                                                                                                              \
    constexpr int WAVES = idx_logits_waves<K>();                                                                         \
    const int main_blocks = cdiv(N, WAVES), blocks = main_blocks + cdiv(N, 64 * WAVES);                                  \
    hipLaunchKernelGGL(edge_idx_logits_kernel<K>, dim3(blocks), dim3(64 * WAVES), 0, stream, Te, R, idx, perm, Pi, Pj,   \
                       srci, (long)W2, wA, bA, H, Hd, rowptr, N, main_blocks, a);                                        \
    break;                                                                                                               \
  }
  switch (KQ) {
    IDX_LOGITS(1) IDX_LOGITS(2) IDX_LOGITS(3) IDX_LOGITS(4) IDX_LOGITS(5) IDX_LOGITS(6) IDX_LOGITS(7) IDX_LOGITS(8)
    default: cgat_set_error("edge_idx_logits: H * Hd = %d", H * Hd); return CGAT_ERR_ARG;
  }
#undef IDX_LOGITS
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

int edge_idx_wsum_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                         const int* srci, int W2, const float* alpha, int H, int Hd, const int* rowptr, int N, int E,
                         float* S, hipStream_t stream) {
  const int HHd = H * Hd;
  CGAT_CHECK_ARG(W2 == 2 * HHd && edge_idx_ok(H, Hd, R) && rowptr && (E <= 0 || (idx && perm && srci && alpha)) &&
                 idx_aligned16(Te, Pi, Pj, S),
                 "edge_idx_wsum: needs Hd %% 4 == 0, H <= 8, H * Hd <= 2048 and 16-byte aligned rows");
  if (N <= 0) return CGAT_OK;
  const int main_blocks = cdiv(N, IDX_WAVES), blocks = main_blocks + cdiv(N, IDX_THREADS);
  CGAT_PROF("edge_idx_wsum", stream);
  hipLaunchKernelGGL(edge_idx_wsum_kernel, dim3(blocks), dim3(IDX_THREADS), 0, stream, Te + HHd, R, idx, perm, Pi + HHd,
                     Pj + HHd, srci, (long)W2, alpha, H, Hd, rowptr, N, main_blocks, S);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
