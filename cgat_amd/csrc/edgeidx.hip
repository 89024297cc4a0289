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
//
// The training form of the same route (second half of this file) keeps no Z either: the backward forms z again from the
// same three rows through the same function idx_z, so its LeakyReLU' pattern is the forward's by construction.
//   edge_idx_bwd_msg  g_alpha, the message half's sign bits and its share of Gi        (seg_bwd_msg_kernel's step on z)
//   edge_idx_bwd_att  the attention half: sign bits, Gi share, partial sums of grad fc_out_A  (seg_bwd_att_kernel's)
//   edge_idx_class_sum  gT[r, :] = sum of the rebuilt gZ rows of class r: grad table = gT W_e, grad W_e = gT^T table
//
// The vector-attention first layer on the same lookup (last part of this file) stores what its second layers read:
//   edge_idx_hidden   hidden[t, :] = leaky(z[t, :]) over all W2 columns, max |hidden| folded in; its backward takes gT
//                     from a STORED gZ (the second form of edge_idx_class_sum)
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"   // block_absmax_commit

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

// THE pre-activation of slot t at column quad f: Te[shell] + Pi[dst] + Pj[src], added in that order (the dense route's:
// part + Pi + Pj).  `pi` is the destination's quad, which every caller holds per segment; Te / Pj may point at a column
// offset of their rows (the message half), f counts from there.  Forward, backward and the debug reader of the signs all
// form z here and nowhere else.
struct IdxSrc {
  const float* Te;
  const float* Pj;
  const int64_t* idx;
  const int* perm;
  const int* srci;
  long W2;
  int R;
};
__device__ __forceinline__ float4 idx_z(const IdxSrc& s, int t, int f, const float4 pi) {
  const float4 te = idx_ld4(s.Te + idx_row(s.idx, s.perm, t, s.R) * s.W2 + f);
  const float4 pj = idx_ld4(s.Pj + (size_t)s.srci[t] * s.W2 + f);
  return make_float4(te.x + pi.x + pj.x, te.y + pi.y + pj.y, te.z + pi.z + pj.z, te.w + pi.w + pj.w);
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
__device__ __forceinline__ void idx_logits_rows(const IdxSrc& src, const float* __restrict__ Pi,
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
    pi[k] = live ? idx_ld4(Pi + (size_t)n * src.W2 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    w[k] = live ? idx_ld4(wA + f) : make_float4(0.f, 0.f, 0.f, 0.f);
    head[k] = live ? f / Hd : -1;
  }
  for (int t = t0; t < t1; t += U * step) {
    float4 z[U][KQ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int tt = t + u * step < t1 ? t + u * step : t1 - 1;   // (clamped: a valid slot of this segment)
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        const int f = 4 * (64 * k + lane);
        z[u][k] = f < HHd ? idx_z(src, tt, f, pi[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t + u * step >= t1) break;                               // (wave-uniform)
      float p[KQ];
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        float s = w[k].x * idx_leaky(z[u][k].x);
        s = fmaf(w[k].y, idx_leaky(z[u][k].y), s);
        s = fmaf(w[k].z, idx_leaky(z[u][k].z), s);
        s = fmaf(w[k].w, idx_leaky(z[u][k].w), s);
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
    const IdxSrc src, const float* __restrict__ Pi, const float* __restrict__ wA, const float* __restrict__ bA, int H,
    int Hd, const int* __restrict__ rowptr, int N, int main_blocks, float* __restrict__ a) {
  constexpr int WAVES = idx_logits_waves<KQ>();
  const int wave = threadIdx.x >> 6, HHd = H * Hd;
  if ((int)blockIdx.x < main_blocks) {
    const int n = blockIdx.x * WAVES + wave;
    if (n >= N) return;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 > SEG_LONG || r1 <= r0) return;      // long: the workgroups behind; empty: no logits
    idx_logits_rows<KQ>(src, Pi, wA, bA, H, Hd, HHd, n, r0, r1, 1, a);
    return;
  }
  __shared__ int list[IDX_THREADS];
  __shared__ int count;
  const int nl = idx_collect_long(rowptr, N, list, &count, blockIdx.x - main_blocks);
  for (int k = 0; k < nl; ++k) {
    const int n = list[k], r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r0 + wave < r1)
      idx_logits_rows<KQ>(src, Pi, wA, bA, H, Hd, HHd, n, r0 + wave, r1, WAVES, a);
  }
}

// Weighted sum over slots t0, t0 + step, ... < t1 of destination n for this lane's column quad f of the message half
// (Pi, Pj, Te point at column H Hd of their rows): the chain in ascending t.  live == false: nothing is read.
__device__ __forceinline__ float4 idx_wsum_rows(const IdxSrc& src, const float* __restrict__ Pi,
                                                const float* __restrict__ alpha, int H, int h, int f, bool live, int n,
                                                int t0, int t1, int step) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (!live) return acc;
  const float4 pi = idx_ld4(Pi + (size_t)n * src.W2 + f);
  for (int t = t0; t < t1; t += IDX_U * step) {
    float4 z[IDX_U];
    float al[IDX_U];
#pragma unroll
    for (int u = 0; u < IDX_U; ++u) {
      const int tt = t + u * step < t1 ? t + u * step : t1 - 1;
      z[u] = idx_z(src, tt, f, pi);
      al[u] = alpha[(size_t)tt * H + h];
    }
#pragma unroll
    for (int u = 0; u < IDX_U; ++u)
      if (t + u * step < t1) {
        acc.x = fmaf(idx_leaky(z[u].x), al[u], acc.x);
        acc.y = fmaf(idx_leaky(z[u].y), al[u], acc.y);
        acc.z = fmaf(idx_leaky(z[u].z), al[u], acc.z);
        acc.w = fmaf(idx_leaky(z[u].w), al[u], acc.w);
      }
  }
  return acc;
}

__global__ __launch_bounds__(IDX_THREADS) void edge_idx_wsum_kernel(
    const IdxSrc src, const float* __restrict__ Pi, const float* __restrict__ alpha, int H, int Hd,
    const int* __restrict__ rowptr, int N, int main_blocks, float* __restrict__ S) {
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
      const float4 acc = idx_wsum_rows(src, Pi, alpha, H, f / Hd, f, true, n, r0, r1, 1);
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
      const float4 acc = idx_wsum_rows(src, Pi, alpha, H, live ? f / Hd : 0, f, live, n, r0 + wave, r1, IDX_WAVES);
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
  const IdxSrc src = {Te, Pj, idx, perm, srci, (long)W2, R};
  CGAT_PROF("edge_idx_logits", stream);
#define IDX_LOGITS(K)                                                                                                    \
  case K: {                                                                                                              \
    constexpr int WAVES = idx_logits_waves<K>();                                                                         \
    const int main_blocks = cdiv(N, WAVES), blocks = main_blocks + cdiv(N, 64 * WAVES);                                  \
    hipLaunchKernelGGL(edge_idx_logits_kernel<K>, dim3(blocks), dim3(64 * WAVES), 0, stream, src, Pi, wA, bA, H, Hd,     \
                       rowptr, N, main_blocks, a);                                                                       \
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
  const IdxSrc src = {Te + HHd, Pj + HHd, idx, perm, srci, (long)W2, R};   // the message half of the rows
  hipLaunchKernelGGL(edge_idx_wsum_kernel, dim3(blocks), dim3(IDX_THREADS), 0, stream, src, Pi + HHd, alpha, H, Hd, rowptr,
                     N, main_blocks, S);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// =====================================================================================================================
// The training form: the segment backward on recomputed z, the class sum, the debug reader of the signs.
// The three steps are those of segbwd.hip's three-kernel form (seg_bwd_msg_kernel, seg_bwd_soft_kernel -- launched as it
// is --, seg_bwd_att_kernel): the same operations in the same order per output element, with idx_z where they read Z and
// any Hd % 4 == 0 (whole 32-column mask words per half: H * Hd % 32 == 0).  No atomics on memory.
// =====================================================================================================================
#define IDX_SEGB_NODES 8    // destination segments per workgroup of the attention-half kernel = rows of partialW per launch
#define IDX_PIECE_ROWS 256  // rows of one piece of a class in the class sum (compile-time: the bits follow from E, R alone)

// the sign bits of four columns per lane, eight lanes per 32-column word, OR-ed across the eight lanes (two quad
// permutations and the half-row mirror): every lane of the group returns the word (segbwd.hip)
__device__ __forceinline__ unsigned idx_sign_word(const float4 z, int lane) {
  unsigned w = ((z.x > 0.f ? 1u : 0u) | (z.y > 0.f ? 2u : 0u) | (z.z > 0.f ? 4u : 0u) | (z.w > 0.f ? 8u : 0u)) << (4 * (lane & 7));
  w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
  w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
  w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x141, 0xF, 0xF, true);   // row_half_mirror
  return w;
}

// (waves per workgroup by the registers a lane's KQ quads of Pi, gS and the Gi sums take, as idx_logits_waves; every
// output is one slot's or one segment's own, and the split of a long segment is this constant of the dims)
template <int KQ>
constexpr int idx_bwd_waves() { return KQ <= 2 ? IDX_WAVES : (KQ <= 4 ? IDX_WAVES / 2 : IDX_WAVES / 4); }

// Step 1 over slots t0, t0 + step, ... < t1 of destination n, by one wave; lane l owns column quads 64 k + l of the message
// half (src / Pi / gS rows at that half).  Per slot: g_alpha[t, h] = leaky(zM[t, h, :]) . gS[n, h, :] + gs[n, h] -> tt, the
// sign words of the message half -> mask, and gim += alpha[t, h] gS[n] leaky'(zM): this wave's share of Gi in ascending t.
template <int KQ>
__device__ __forceinline__ void idx_bwd_msg_rows(const IdxSrc& src, const float4 (&pi)[KQ], const float4 (&g)[KQ],
                                                 const int (&head)[KQ], const float* __restrict__ alpha,
                                                 const float* __restrict__ gsn, int H, int HHd, int nw, int t0, int t1,
                                                 int step, float* __restrict__ tt, unsigned* __restrict__ mask,
                                                 float4 (&gim)[KQ]) {
  constexpr int U = KQ <= 2 ? 4 : 2;
  const int lane = threadIdx.x & 63;
  for (int t = t0; t < t1; t += U * step) {
    float4 z[U][KQ];
    float al[U][KQ];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ts = t + u * step < t1 ? t + u * step : t1 - 1;   // (clamped: a valid slot of this segment)
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        const bool live = head[k] >= 0;
        z[u][k] = live ? idx_z(src, ts, 4 * (64 * k + lane), pi[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
        al[u][k] = live ? alpha[(size_t)ts * H + head[k]] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t + u * step >= t1) break;                               // (wave-uniform)
      const size_t row = (size_t)(t + u * step);
      float p[KQ];
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        const float4 zz = z[u][k], gg = g[k];
        p[k] = (zz.x > 0.f ? zz.x : 0.01f * zz.x) * gg.x + (zz.y > 0.f ? zz.y : 0.01f * zz.y) * gg.y +
               (zz.z > 0.f ? zz.z : 0.01f * zz.z) * gg.z + (zz.w > 0.f ? zz.w : 0.01f * zz.w) * gg.w;
        const float a_ = al[u][k];
        gim[k].x += a_ * gg.x * (zz.x > 0.f ? 1.f : 0.01f); gim[k].y += a_ * gg.y * (zz.y > 0.f ? 1.f : 0.01f);
        gim[k].z += a_ * gg.z * (zz.z > 0.f ? 1.f : 0.01f); gim[k].w += a_ * gg.w * (zz.w > 0.f ? 1.f : 0.01f);
        const unsigned w = idx_sign_word(zz, lane);
        // (a word's eight lanes are live together: H * Hd % 32 == 0)
        if ((lane & 7) == 0 && head[k] >= 0) mask[row * nw + ((HHd + 4 * (64 * k + lane)) >> 5)] = w;
      }
      for (int h = 0; h < H; ++h) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < KQ; ++k) v += head[k] == h ? p[k] : 0.f;
        v = idx_wave_sum64(v);
        if (lane == 0) tt[row * H + h] = v + gsn[h];
      }
    }
  }
}

template <int KQ>
__global__ __launch_bounds__(64 * idx_bwd_waves<KQ>()) void edge_idx_bwd_msg_kernel(
    const IdxSrc src, const float* __restrict__ Pi, const float* __restrict__ alpha, const float* __restrict__ gS,
    const float* __restrict__ gs, int H, int Hd, const int* __restrict__ rowptr, int N, int main_blocks,
    float* __restrict__ tt, unsigned* __restrict__ mask, float* __restrict__ Gi) {
  constexpr int WAVES = idx_bwd_waves<KQ>();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, HHd = H * Hd, nw = (int)(src.W2 >> 5);
  float4 pi[KQ], g[KQ], gim[KQ];
  int head[KQ];
  if ((int)blockIdx.x < main_blocks) {
    const int n = blockIdx.x * WAVES + wave;
    if (n >= N) return;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 > SEG_LONG) return;                  // the workgroups behind
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      const int f = 4 * (64 * k + lane);
      const bool live = f < HHd;
      pi[k] = live ? idx_ld4(Pi + (size_t)n * src.W2 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      g[k] = live ? idx_ld4(gS + (size_t)n * HHd + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      head[k] = live ? f / Hd : -1;
      gim[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    idx_bwd_msg_rows<KQ>(src, pi, g, head, alpha, gs + (size_t)n * H, H, HHd, nw, r0, r1, 1, tt, mask, gim);
#pragma unroll
    for (int k = 0; k < KQ; ++k)                     // (an empty segment writes zeros)
      if (head[k] >= 0) *reinterpret_cast<float4*>(Gi + (size_t)n * src.W2 + 4 * (64 * k + lane)) = gim[k];
    return;
  }
  __shared__ int list[IDX_THREADS];
  __shared__ int count;
  __shared__ float4 part[IDX_THREADS];
  const int nl = idx_collect_long(rowptr, N, list, &count, blockIdx.x - main_blocks);
  for (int j = 0; j < nl; ++j) {
    const int n = list[j], r0 = rowptr[n], r1 = rowptr[n + 1];
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
      const int f = 4 * (64 * k + lane);
      const bool live = f < HHd;
      pi[k] = live ? idx_ld4(Pi + (size_t)n * src.W2 + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      g[k] = live ? idx_ld4(gS + (size_t)n * HHd + f) : make_float4(0.f, 0.f, 0.f, 0.f);
      head[k] = live ? f / Hd : -1;
      gim[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // rows r0 + wave, r0 + wave + WAVES, ...: the fixed split; the partial sums through LDS in wave order
    idx_bwd_msg_rows<KQ>(src, pi, g, head, alpha, gs + (size_t)n * H, H, HHd, nw, r0 + wave, r1, WAVES, tt, mask, gim);
#pragma unroll
    for (int k = 0; k < KQ; ++k) {                   // (uniform trip count: the barriers)
      __syncthreads();
      part[threadIdx.x] = gim[k];
      __syncthreads();
      if (wave == 0 && head[k] >= 0) {
        float4 t = part[lane];
        for (int w = 1; w < WAVES; ++w) {
          const float4 o = part[w * 64 + lane];
          t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w;
        }
        *reinterpret_cast<float4*>(Gi + (size_t)n * src.W2 + 4 * (64 * k + lane)) = t;
      }
    }
  }
}

// Step 3, the attention half: one workgroup per IDX_SEGB_NODES destination segments, a thread per column quad; per
// (segment, quad) Pi[n] and wA are loaded once, the slots four at a time in ascending order.  g = ga wA leaky'(z) -> sign
// words, Gi; ps += ga leaky(z) -> partialW[workgroup][H Hd], the direct sum of grad fc_out_A (z is here with its values).
__global__ __launch_bounds__(256) void edge_idx_bwd_att_kernel(const IdxSrc src, const float* __restrict__ Pi,
                                                               const float* __restrict__ ga, const int* __restrict__ rowptr,
                                                               const float* __restrict__ wA, int N, int H, int Hd,
                                                               float* __restrict__ Gi, float* __restrict__ partialW,
                                                               unsigned* __restrict__ mask) {
  extern __shared__ float pw[];                    // [HHd] per-column partial sums of g_a * leaky(zA)
  const int HHd = H * Hd, nw = (int)(src.W2 >> 5);
  const int tid = threadIdx.x, lane = tid & 63;
  for (int c = tid; c < HHd; c += 256) pw[c] = 0.f;
  __syncthreads();
  const int n0 = blockIdx.x * IDX_SEGB_NODES, n1 = min(N, n0 + IDX_SEGB_NODES);
  for (int n = n0; n < n1; ++n) {
    const int r0 = __builtin_amdgcn_readfirstlane(rowptr[n]), r1 = __builtin_amdgcn_readfirstlane(rowptr[n + 1]);
    if (r1 == r0) {  // no incoming edge: zero row of the segment sum (the message half: edge_idx_bwd_msg_kernel)
      for (int c = tid; c < HHd; c += 256) Gi[(size_t)n * src.W2 + c] = 0.f;
      continue;
    }
    for (int c4 = tid; c4 < HHd / 4; c4 += 256) {
      const int col = 4 * c4;
      const int h = col / Hd;
      const float4 wv = idx_ld4(wA + col);
      const float4 pi = idx_ld4(Pi + (size_t)n * src.W2 + col);
      float4 gi = make_float4(0.f, 0.f, 0.f, 0.f), ps = gi;
      for (int tb = r0; tb < r1; tb += 4) {
        float4 zv[4];
        float cf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = tb + u < r1 ? tb + u : r1 - 1;
          zv[u] = idx_z(src, t, col, pi);
          cf[u] = ga[(size_t)t * H + h];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = tb + u;
          if (t < r1) {
            const float4 z = zv[u];
            const float4 d = make_float4(z.x > 0.f ? 1.f : 0.01f, z.y > 0.f ? 1.f : 0.01f, z.z > 0.f ? 1.f : 0.01f,
                                         z.w > 0.f ? 1.f : 0.01f);
            const float gav = cf[u];
            const float4 g = make_float4(gav * wv.x * d.x, gav * wv.y * d.y, gav * wv.z * d.z, gav * wv.w * d.w);
            ps.x += gav * z.x * d.x; ps.y += gav * z.y * d.y; ps.z += gav * z.z * d.z; ps.w += gav * z.w * d.w;
            const unsigned w = idx_sign_word(z, lane);
            if ((lane & 7) == 0) mask[(size_t)t * nw + (col >> 5)] = w;
            gi.x += g.x; gi.y += g.y; gi.z += g.z; gi.w += g.w;
          }
        }
      }
      *reinterpret_cast<float4*>(Gi + (size_t)n * src.W2 + col) = gi;
      pw[col] += ps.x; pw[col + 1] += ps.y; pw[col + 2] += ps.z; pw[col + 3] += ps.w;
    }
  }
  __syncthreads();
  for (int c = tid; c < HHd; c += 256) partialW[(size_t)blockIdx.x * HHd + c] = pw[c];
}

bool edge_idx_train_ok(int H, int Hd, int R) { return edge_idx_ok(H, Hd, R) && ((long)H * Hd) % 32 == 0; }
int edge_idx_bwd_chunks(int N) { return cdiv(N > 0 ? N : 1, IDX_SEGB_NODES); }

int edge_idx_bwd_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                        const int* srci, int W2, const float* alpha, const float* gS, const float* gs, const float* wA,
                        int H, int Hd, const int* rowptr, int N, int E, float* tt, float* ga, unsigned* mask, float* Gi,
                        float* partialW, hipStream_t stream) {
  const int HHd = H * Hd;
  CGAT_CHECK_ARG(W2 == 2 * HHd && edge_idx_train_ok(H, Hd, R) && N > 0 && E > 0 && idx && perm && srci && rowptr && alpha &&
                 gs && tt && ga && mask && partialW && idx_aligned16(Te, Pi, Pj, Gi) && idx_aligned16(gS, wA, gS, wA),
                 "edge_idx_bwd: needs Hd %% 4 == 0, H * Hd %% 32 == 0, H <= 8, H * Hd <= 2048 and 16-byte aligned rows");
  const int KQ = cdiv(HHd, 256);
  {
    const IdxSrc src = {Te + HHd, Pj + HHd, idx, perm, srci, (long)W2, R};   // the message half of the rows
    CGAT_PROF("edge_idx_bwd_msg", stream);
#define IDX_BWD_MSG(K)                                                                                                   \
  case K: {                                                                                                              \
    constexpr int WAVES = idx_bwd_waves<K>();                                                                            \
    const int main_blocks = cdiv(N, WAVES), blocks = main_blocks + cdiv(N, 64 * WAVES);                                  \
    hipLaunchKernelGGL(edge_idx_bwd_msg_kernel<K>, dim3(blocks), dim3(64 * WAVES), 0, stream, src, Pi + HHd, alpha, gS,  \
                       gs, H, Hd, rowptr, N, main_blocks, tt, mask, Gi + HHd);                                           \
    break;                                                                                                               \
  }
    switch (KQ) {
      IDX_BWD_MSG(1) IDX_BWD_MSG(2) IDX_BWD_MSG(3) IDX_BWD_MSG(4) IDX_BWD_MSG(5) IDX_BWD_MSG(6) IDX_BWD_MSG(7) IDX_BWD_MSG(8)
      default: cgat_set_error("edge_idx_bwd: H * Hd = %d", HHd); return CGAT_ERR_ARG;
    }
#undef IDX_BWD_MSG
    CGAT_LAUNCH_CHECK();
  }
  CGAT_TRY(seg_bwd_soft_launch(alpha, tt, rowptr, N, H, ga, stream));
  const IdxSrc src = {Te, Pj, idx, perm, srci, (long)W2, R};
  CGAT_PROF("edge_idx_bwd_att", stream);
  hipLaunchKernelGGL(edge_idx_bwd_att_kernel, dim3(edge_idx_bwd_chunks(N)), dim3(256), (size_t)HHd * sizeof(float), stream,
                     src, Pi, ga, rowptr, wA, N, H, Hd, Gi, partialW, mask);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- the class sum: gT[r, :] = sum over the slots of class r of the rebuilt gZ rows, in two levels ----
// Slots grouped by class by a stable counting sort (cls_pos [E]: edge_idx_class_plan_launch below, once per batch);
// every class cut into pieces of IDX_PIECE_ROWS rows.  Level 1: edge_gj_kernel over the piece-level row pointer sums each
// piece in ascending order into a partial row.  Level 2: the partials of a class in piece order, in fp64, rounded once.
// At most ceil(E / IDX_PIECE_ROWS) + R pieces: every size follows from E and R.
int edge_idx_class_pieces(int E, int R) { return cdiv(E > 0 ? E : 1, IDX_PIECE_ROWS) + R; }

// The grouping itself: a stable counting sort of the slots by class for FEW classes of MANY rows each (cgat_csr_from_keys
// sorts every segment by one workgroup at best, by one lane beyond 8 192 rows: its segments are atoms).  Slots in blocks of
// IDX_CLS_BLOCK: per-block class counts (integer LDS atomics: order-free), a prefix over the blocks per class, then every
// slot's rank among the earlier slots of its class in its block -- cls_pos lists each class in ascending slot order.
#define IDX_CLS_BLOCK 256
__global__ __launch_bounds__(IDX_CLS_BLOCK) void edge_idx_class_count_kernel(const int64_t* __restrict__ idx,
                                                                             const int* __restrict__ perm, int E, int R,
                                                                             int nb, int* __restrict__ counts) {
  __shared__ int cnt[EDGE_IDX_MAX_ROWS];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * IDX_CLS_BLOCK + threadIdx.x;
  if (t < E) atomicAdd(&cnt[(int)idx_row(idx, perm, t, R)], 1);
  __syncthreads();
  if ((int)threadIdx.x < R) counts[(size_t)threadIdx.x * nb + blockIdx.x] = cnt[threadIdx.x];   // class-major
}
// one workgroup per class: counts[r][0..nb) -> exclusive prefix in place, total[r]
__global__ __launch_bounds__(256) void edge_idx_class_scan_kernel(int* __restrict__ counts, int nb, int* __restrict__ total) {
  __shared__ int part[257];
  int* c = counts + (size_t)blockIdx.x * nb;
  const int per = (nb + 255) / 256, b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += c[b];
  part[threadIdx.x + 1] = sum;
  if (threadIdx.x == 0) part[0] = 0;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 0; i < 256; ++i) part[i + 1] += part[i];
  __syncthreads();
  int run = part[threadIdx.x];
  for (int b = b0; b < b1; ++b) { const int v = c[b]; c[b] = run; run += v; }
  if (threadIdx.x == 0) total[blockIdx.x] = part[256];
}
// one workgroup: cls_rowptr [R + 1] from the totals; piece_start [R + 1] (pieces before class r); piece_rowptr
// [n_max + 1] (first row of piece p in cls_pos; the unused pieces behind the last one are empty)
__global__ __launch_bounds__(EDGE_IDX_MAX_ROWS) void edge_idx_pieces_kernel(const int* __restrict__ total, int R, int n_max,
                                                                            int* __restrict__ cls_rowptr,
                                                                            int* __restrict__ piece_start,
                                                                            int* __restrict__ piece_rowptr) {
  __shared__ int off[EDGE_IDX_MAX_ROWS + 1], row[EDGE_IDX_MAX_ROWS + 1];
  const int r = threadIdx.x;
  const int n = r < R ? total[r] : 0;
  const int c = (n + IDX_PIECE_ROWS - 1) / IDX_PIECE_ROWS;
  off[r + 1] = c;
  row[r + 1] = n;
  if (r == 0) off[0] = row[0] = 0;
  __syncthreads();
  if (r == 0)
    for (int i = 0; i < R; ++i) { off[i + 1] += off[i]; row[i + 1] += row[i]; }
  __syncthreads();
  if (r < R) {
    cls_rowptr[r] = row[r];
    piece_start[r] = off[r];
    for (int j = 0; j < c && off[r] + j < n_max; ++j) piece_rowptr[off[r] + j] = row[r] + IDX_PIECE_ROWS * j;
  }
  if (r == 0) { piece_start[R] = off[R] < n_max ? off[R] : n_max; cls_rowptr[R] = row[R]; }
  for (int p = off[R] + r; p <= n_max; p += EDGE_IDX_MAX_ROWS) piece_rowptr[p] = row[R];
}
__global__ __launch_bounds__(IDX_CLS_BLOCK) void edge_idx_class_fill_kernel(const int64_t* __restrict__ idx,
                                                                            const int* __restrict__ perm, int E, int R,
                                                                            int nb, const int* __restrict__ prefix,
                                                                            const int* __restrict__ cls_rowptr,
                                                                            int* __restrict__ cls_pos) {
  __shared__ int key[IDX_CLS_BLOCK];
  const int t = blockIdx.x * IDX_CLS_BLOCK + threadIdx.x;
  const int k = t < E ? (int)idx_row(idx, perm, t, R) : -1;
  key[threadIdx.x] = k;
  __syncthreads();
  if (k < 0) return;
  int rank = 0;
  for (int j = 0; j < (int)threadIdx.x; ++j) rank += key[j] == k ? 1 : 0;
  cls_pos[cls_rowptr[k] + prefix[(size_t)k * nb + blockIdx.x] + rank] = t;
}
size_t edge_idx_class_plan_ws_bytes(int E, int R) {
  return ws_round((size_t)R * cdiv(E > 0 ? E : 1, IDX_CLS_BLOCK), 4) + 2 * ws_round((size_t)R + 1, 4);
}
int edge_idx_class_plan_launch(const int64_t* idx, const int* perm, int E, int R, int* cls_pos, int* piece_start,
                               int* piece_rowptr, void* ws, size_t ws_bytes, hipStream_t stream) {
  CGAT_CHECK_ARG(R >= 1 && R <= EDGE_IDX_MAX_ROWS && E > 0 && idx && perm && cls_pos && piece_start && piece_rowptr,
                 "edge_idx_class_plan: 1 <= R <= %d, E > 0", EDGE_IDX_MAX_ROWS);
  const int nb = cdiv(E, IDX_CLS_BLOCK);
  Workspace w(ws, ws_bytes);
  int* counts = w.take<int>((size_t)R * nb);
  int* total = w.take<int>((size_t)R + 1);
  int* cls_rowptr = w.take<int>((size_t)R + 1);
  if (!w.ok) {
    cgat_set_error("edge_idx_class_plan: workspace too small (%zu < %zu)", ws_bytes, w.off);
    return CGAT_ERR_WORKSPACE;
  }
  hipLaunchKernelGGL(edge_idx_class_count_kernel, dim3(nb), dim3(IDX_CLS_BLOCK), 0, stream, idx, perm, E, R, nb, counts);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_idx_class_scan_kernel, dim3(R), dim3(256), 0, stream, counts, nb, total);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_idx_pieces_kernel, dim3(1), dim3(EDGE_IDX_MAX_ROWS), 0, stream, total, R,
                     edge_idx_class_pieces(E, R), cls_rowptr, piece_start, piece_rowptr);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_idx_class_fill_kernel, dim3(nb), dim3(IDX_CLS_BLOCK), 0, stream, idx, perm, E, R, nb, counts,
                     cls_rowptr, cls_pos);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

__global__ __launch_bounds__(256) void edge_idx_class_reduce_kernel(const float* __restrict__ part,
                                                                    const int* __restrict__ piece_start, int n_max, int W2,
                                                                    float* __restrict__ gT) {
  const int r = blockIdx.y, col = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (col >= W2) return;
  const int p0 = min(piece_start[r], n_max), p1 = min(piece_start[r + 1], n_max);
  double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;         // (an unused class: exact zeros)
  for (int pb = p0; pb < p1; pb += 8) {
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = idx_ld4(part + (size_t)(pb + u < p1 ? pb + u : p1 - 1) * W2 + col);
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (pb + u < p1) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
  }
  *reinterpret_cast<float4*>(gT + (size_t)r * W2 + col) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
}

int edge_idx_class_sum_launch(const EdgeRC& rc, const int* piece_rowptr, const int* piece_start, const int* cls_pos, int R,
                              int E, int W2, float* partials, float* gT, hipStream_t stream) {
  CGAT_CHECK_ARG(R >= 1 && R <= EDGE_IDX_MAX_ROWS && W2 % 4 == 0 && piece_rowptr && piece_start && cls_pos &&
                 idx_aligned16(partials, gT, partials, gT), "edge_idx_class_sum: 1 <= R <= %d, 16-byte aligned rows",
                 EDGE_IDX_MAX_ROWS);
  const int n_max = edge_idx_class_pieces(E, R);
  CGAT_PROF("edge_idx_class_sum", stream);
  CGAT_TRY(edge_gj_launch(rc, piece_rowptr, cls_pos, n_max, W2, partials, W2, stream));
  hipLaunchKernelGGL(edge_idx_class_reduce_kernel, dim3(cdiv(W2 / 4, 256), R), dim3(256), 0, stream, partials, piece_start,
                     n_max, W2, gT);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ... over a STORED gZ [E, W2] (row-major, destination-sorted slots: the vector-attention first layer, whose gZ autograd
// hands over).  Level 1: one workgroup per piece, a thread per column quad, the piece's rows gathered through cls_pos four
// at a time and added in ascending order in fp64, rounded once per piece; level 2 the reduction above.  (seg_wsum_launch
// with cls_pos as its row gather -- the launch that forms Gj from a stored gZ -- computes the same partial rows by an
// fp32 chain of up to IDX_PIECE_ROWS terms; with every slot in one class that chain left grad W_e 2.7 x the dense
// product's error, outside the ratio rule of the tests.  The adds hide behind the gather either way.)
__global__ __launch_bounds__(256) void edge_idx_class_piece_kernel(const float* __restrict__ gZ, long ld,
                                                                   const int* __restrict__ cls_pos,
                                                                   const int* __restrict__ piece_rowptr, int W2,
                                                                   float* __restrict__ part) {
  const int p = blockIdx.x;
  const int r0 = piece_rowptr[p], r1 = piece_rowptr[p + 1];
  for (int f = 4 * threadIdx.x; f < W2; f += 4 * blockDim.x) {
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;       // (an empty piece: zeros)
    for (int r = r0; r < r1; r += 4) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = idx_ld4(gZ + (size_t)cls_pos[r + u < r1 ? r + u : r1 - 1] * ld + f);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (r + u < r1) { a0 += (double)v[u].x; a1 += (double)v[u].y; a2 += (double)v[u].z; a3 += (double)v[u].w; }
    }
    *reinterpret_cast<float4*>(part + (size_t)p * W2 + f) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
  }
}
int edge_idx_class_sum_launch(const float* gZ, const int* piece_rowptr, const int* piece_start, const int* cls_pos, int R,
                              int E, int W2, float* partials, float* gT, hipStream_t stream) {
  CGAT_CHECK_ARG(R >= 1 && R <= EDGE_IDX_MAX_ROWS && W2 > 0 && W2 % 4 == 0 && E > 0 && gZ && piece_rowptr && piece_start &&
                 cls_pos && partials && gT && idx_aligned16(partials, gT, gZ, gZ),
                 "edge_idx_class_sum: 1 <= R <= %d, E > 0, W2 %% 4 == 0, 16-byte aligned rows", EDGE_IDX_MAX_ROWS);
  const int n_max = edge_idx_class_pieces(E, R);
  CGAT_PROF("edge_idx_class_sum", stream);
  const int threads = W2 / 4 >= 256 ? 256 : cdiv(W2 / 4, 64) * 64;
  hipLaunchKernelGGL(edge_idx_class_piece_kernel, dim3(n_max), dim3(threads), 0, stream, gZ, (long)W2, cls_pos, piece_rowptr,
                     W2, partials);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(edge_idx_class_reduce_kernel, dim3(cdiv(W2 / 4, 256), R), dim3(256), 0, stream, partials, piece_start,
                     n_max, W2, gT);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// =====================================================================================================================
// The vector-attention first layer on the same lookup: hidden[t, :] = leaky(z[t, :]) over ALL W2 columns, stored (the second
// layers need every row), and max |hidden| folded into the launch (their fp16 scale, as edge_z_launch gives it to the
// dense op).  A flat decomposition: a workgroup takes IDX_HID_ROWS consecutive slots and its threads walk the
// IDX_HID_ROWS x W2 / 4 column quads of the tile row by row, IDX_HID_U quads in flight per thread.  Nothing is summed over
// a segment here, so a segment per wave would only buy Pi[n] in registers -- which the L2 serves anyway (the slots of a
// destination are neighbours) -- at the price of the long-segment split; flat, every workgroup has the same work whatever
// the degrees are, and the stores of a tile are one contiguous stream.  Column-wise: no bound on W2.
// =====================================================================================================================
#define IDX_HID_THREADS 256
#define IDX_HID_ROWS 8
#define IDX_HID_U 4

__global__ __launch_bounds__(IDX_HID_THREADS) void edge_idx_hidden_kernel(const IdxSrc src, const float* __restrict__ Pi,
                                                                          const int* __restrict__ dsti, int E, int Q,
                                                                          float* __restrict__ hidden,
                                                                          float* __restrict__ hmax) {
  const int t0 = blockIdx.x * IDX_HID_ROWS;
  const int rows = min(IDX_HID_ROWS, E - t0);
  const int items = rows * Q;                        // (<= 8 * W2 / 4: an int)
  float m = 0.f;
  for (int j0 = threadIdx.x; j0 < items; j0 += IDX_HID_U * IDX_HID_THREADS) {
    float4 z[IDX_HID_U];
    int tt[IDX_HID_U], ff[IDX_HID_U];
#pragma unroll
    for (int u = 0; u < IDX_HID_U; ++u) {
      const int j = j0 + u * IDX_HID_THREADS < items ? j0 + u * IDX_HID_THREADS : j0;   // (clamped: a valid item)
      const int r = j / Q;
      tt[u] = t0 + r;
      ff[u] = 4 * (j - r * Q);
      z[u] = idx_z(src, tt[u], ff[u], idx_ld4(Pi + (size_t)dsti[tt[u]] * src.W2 + ff[u]));
    }
#pragma unroll
    for (int u = 0; u < IDX_HID_U; ++u)
      if (j0 + u * IDX_HID_THREADS < items) {
        const float4 h = make_float4(idx_leaky(z[u].x), idx_leaky(z[u].y), idx_leaky(z[u].z), idx_leaky(z[u].w));
        *reinterpret_cast<float4*>(hidden + (size_t)tt[u] * src.W2 + ff[u]) = h;
        m = fmaxf(m, fmaxf(fmaxf(fabsf(h.x), fabsf(h.y)), fmaxf(fabsf(h.z), fabsf(h.w))));
      }
  }
  // one integer atomic max per workgroup on the bit image of a non-negative float: order-free
  if (hmax) block_absmax_commit(m, hmax);
}

// Shapes the launch takes: whole column quads, 1 <= R <= EDGE_IDX_MAX_ROWS; 64-bit row offsets.  Host only.
bool edge_idx_hidden_ok(int W2, int R) { return W2 >= 4 && W2 % 4 == 0 && R >= 1 && R <= EDGE_IDX_MAX_ROWS; }

int edge_idx_hidden_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                           const int* srci, const int* dsti, int W2, int E, float* hidden, float* hmax,
                           hipStream_t stream) {
  CGAT_CHECK_ARG(edge_idx_hidden_ok(W2, R) && Te && Pi && Pj && idx && perm && srci && dsti && hidden &&
                 idx_aligned16(Te, Pi, Pj, hidden),
                 "edge_idx_hidden: needs W2 %% 4 == 0, 1 <= R <= %d and 16-byte aligned rows", EDGE_IDX_MAX_ROWS);
  if (E <= 0) return CGAT_OK;
  const IdxSrc src = {Te, Pj, idx, perm, srci, (long)W2, R};
  CGAT_PROF("edge_idx_hidden", stream);
  hipLaunchKernelGGL(edge_idx_hidden_kernel, dim3(cdiv(E, IDX_HID_ROWS)), dim3(IDX_HID_THREADS), 0, stream, src, Pi, dsti, E,
                     W2 / 4, hidden, hmax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- debug: mask[perm[t]][c] = (z[t, c] > 0) in original edge order, through idx_z ----
__global__ __launch_bounds__(256) void edge_idx_signs_kernel(const IdxSrc src, const float* __restrict__ Pi,
                                                             const int* __restrict__ dsti, long E, int W2,
                                                             uint8_t* __restrict__ mask) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Q = W2 / 4;
  if (i >= E * Q) return;
  const int t = (int)(i / Q), f = 4 * (int)(i - (long)t * Q);
  const float4 z = idx_z(src, t, f, idx_ld4(Pi + (size_t)dsti[t] * W2 + f));
  *reinterpret_cast<uchar4*>(mask + (size_t)src.perm[t] * W2 + f) =
      make_uchar4(z.x > 0.f ? 1 : 0, z.y > 0.f ? 1 : 0, z.z > 0.f ? 1 : 0, z.w > 0.f ? 1 : 0);
}
int edge_idx_signs_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                          const int* srci, const int* dsti, int W2, long E, uint8_t* mask, hipStream_t stream) {
  CGAT_CHECK_ARG(W2 % 4 == 0 && R >= 1 && idx && perm && srci && dsti && mask && idx_aligned16(Te, Pi, Pj, mask),
                 "edge_idx_signs: W2 %% 4 == 0 and 16-byte aligned rows");
  if (E <= 0) return CGAT_OK;
  const IdxSrc src = {Te, Pj, idx, perm, srci, (long)W2, R};
  hipLaunchKernelGGL(edge_idx_signs_kernel, dim3((unsigned)cdiv(E * (W2 / 4), 256)), dim3(256), 0, stream, src, Pi, dsti, E,
                     W2, mask);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
