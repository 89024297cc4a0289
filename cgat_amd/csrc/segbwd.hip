// The segment backward of the scalar-attention layer (GATConvNodes): g_alpha, softmax backward, the pre-activation
// gradient gZ (or its sign bits), the destination-side segment sum Gi and the partial sums for grad fc_out_A -- kernels
// and their launchers; layers.hip decides the route's predicates and calls edge_seg_bwd_launch.
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

// Node-aligned fused edge backward.  One workgroup owns SEGB_NODES consecutive destination
// segments (whole segments, CSR order), so everything that PyG's softmax/scatter backward needs
// per destination is local: per node n
//   1. g_alpha[t,h] = leaky(zM[t,h,:]) . gS[n,h,:] + gs[n,h]            (block reductions)
//   2. g_a[t,h]     = alpha[t,h] * (g_alpha[t,h] - sum_seg alpha * g_alpha)   (softmax backward)
//   3. gZ[t,:]      = [ g_a * wA_out * leaky'(zA) | alpha * gS[n] * leaky'(zM) ],
//      Gi[n,:]      = sum_seg gZ[t,:]   (the x_i-side segment sum),  partial sums of g_a*leaky(zA)
//      for the gradient of MH_A.fc_out.weight.
// gS[n] is read once per node instead of gathered per edge; Z is read twice but the second
// read of a 70 KB segment hits L2.  No atomics; fixed summation order.
#define SEGB_NODES 8
#define SEGB_LONG 256   // rows above which the softmax backward of a segment is done by the whole workgroup
__device__ __forceinline__ float wave_sum_l(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// ZB (with VEC and mask): Z is read as bf16 (the "bf16" edge-storage mode; offsets count elements either way)
template <bool VEC, bool ZB = false>
__global__ __launch_bounds__(256) void edge_seg_bwd_kernel(const float* __restrict__ Z, float* __restrict__ gZ,
                                                           long gz_block, const float* __restrict__ alpha,
                                                           const float* __restrict__ gS, const float* __restrict__ gs,
                                                           const int* __restrict__ rowptr,
                                                           const float* __restrict__ wA_out, int N, int H, int Hd,
                                                           float* __restrict__ tt, float* __restrict__ ga,
                                                           float* __restrict__ Gi, float* __restrict__ partialW,
                                                           float* __restrict__ gzmax, unsigned* __restrict__ mask,
                                                           float* __restrict__ gimax) {
  // gimax (optional, VEC path): max |Gi| is folded into gimax[0] the same way -- the scale of the node-side products
  // mask (optional, VEC path, W2 % 256 == 0): gZ is NOT written; instead bit (col & 31) of mask[t][col >> 5] records
  // Z[t, col] > 0, from which -- with ga, alpha, gS, wA -- the consumers rebuild the row (struct EdgeRC, kernels.h)
  // gzmax (optional, VEC path): max |gZ| is folded into gzmax[0] (zeroed before) -- the per-tensor scale the fp16
  // forms of the two kernels that consume gZ need (edgebwd.hip); a maximum does not depend on the order it is taken in
  extern __shared__ float pw[];  // [HHd] per-column partial sums of g_a * leaky(zA)
  float gm = 0.f, gim_max = 0.f;
  const int HHd = H * Hd, W2 = 2 * HHd;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < HHd; c += 256) pw[c] = 0.f;
  const int n0 = blockIdx.x * SEGB_NODES, n1 = min(N, n0 + SEGB_NODES);
  // The three steps run over ALL segments of the workgroup before the next one starts: two barriers per workgroup
  // instead of three per node.
  // With the sign-bit output and Hd = 256 (one float4 of a head per lane) step 1 also produces everything the MESSAGE
  // half of gZ contributes -- its sign bits, its share of Gi, its maximum: they need alpha only, not the softmax
  // backward -- so that step 3 reads only the attention half of Z (Z is then read once, not 1.5 times).  A wave owns
  // head h = wave, wave + 4, ... of EVERY row of a segment, so its lanes accumulate Gi over the rows in the order
  // step 3 used to (no cross-wave sum).
  const bool fuse_m = VEC && mask != nullptr && Hd == 256;
  // ---- 1. g_alpha: one wave per edge row, wave-level reductions only ----
  if (fuse_m) {
    for (int n = n0; n < n1; ++n) {
      const int r0 = rowptr[n], r1 = rowptr[n + 1];
      if (r1 == r0) continue;                    // (step 3 zero-fills the whole Gi row of an empty segment)
      for (int h = wave; h < H; h += 4) {
        const int wcol = HHd + h * Hd + 4 * lane;                            // this lane's four columns of the row
        const float4 g = *reinterpret_cast<const float4*>(gS + (long)n * HHd + h * Hd + 4 * lane);
        const float gsn = gs[(long)n * H + h];
        float4 gim = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int tb = r0; tb < r1; tb += 4) {
          float4 zv[4];
          float al[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = tb + u < r1 ? tb + u : r1 - 1;
            zv[u] = ZB ? load4_bf16(reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + wcol)
                       : *reinterpret_cast<const float4*>(Z + (long)t * W2 + wcol);
            al[u] = alpha[(long)t * H + h];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = tb + u;
            if (t < r1) {
              const float4 z = zv[u];
              float part = (z.x > 0.f ? z.x : 0.01f * z.x) * g.x + (z.y > 0.f ? z.y : 0.01f * z.y) * g.y +
                           (z.z > 0.f ? z.z : 0.01f * z.z) * g.z + (z.w > 0.f ? z.w : 0.01f * z.w) * g.w;
              part = wave_sum_l(part);
              if (lane == 0) tt[(long)t * H + h] = part + gsn;
              const float a_ = al[u];
              const float4 gz = make_float4(a_ * g.x * (z.x > 0.f ? 1.f : 0.01f), a_ * g.y * (z.y > 0.f ? 1.f : 0.01f),
                                            a_ * g.z * (z.z > 0.f ? 1.f : 0.01f), a_ * g.w * (z.w > 0.f ? 1.f : 0.01f));
              gm = fmaxf(fmaxf(gm, fmaxf(fabsf(gz.x), fabsf(gz.y))), fmaxf(fabsf(gz.z), fabsf(gz.w)));
              gim.x += gz.x; gim.y += gz.y; gim.z += gz.z; gim.w += gz.w;
              unsigned w = ((z.x > 0.f ? 1u : 0u) | (z.y > 0.f ? 2u : 0u) | (z.z > 0.f ? 4u : 0u) | (z.w > 0.f ? 8u : 0u))
                           << (4 * (lane & 7));
              w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
              w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
              w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x141, 0xF, 0xF, true);   // row_half_mirror
              if ((lane & 7) == 0) mask[(long)t * (W2 >> 5) + (wcol >> 5)] = w;
            }
          }
        }
        *reinterpret_cast<float4*>(Gi + (long)n * W2 + wcol) = gim;
        gim_max = fmaxf(fmaxf(gim_max, fmaxf(fabsf(gim.x), fabsf(gim.y))), fmaxf(fabsf(gim.z), fabsf(gim.w)));
      }
    }
  } else
  for (int n = n0; n < n1; ++n) {
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    const float* gSn = gS + (long)n * HHd;
    for (int t = r0 + wave; t < r1; t += 4) {
      const float* zM = Z + (long)t * W2 + HHd;
      for (int h = 0; h < H; ++h) {
        float part = 0.f;
        if (VEC) {
          const float4* z4 = reinterpret_cast<const float4*>(zM + h * Hd);
          const __bf16* z16 = reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + HHd + h * Hd;
          const float4* g4 = reinterpret_cast<const float4*>(gSn + h * Hd);
          for (int j = lane; j < Hd / 4; j += 64) {
            float4 z = ZB ? load4_bf16(z16 + 4 * j) : z4[j], g = g4[j];
            part += (z.x > 0.f ? z.x : 0.01f * z.x) * g.x + (z.y > 0.f ? z.y : 0.01f * z.y) * g.y +
                    (z.z > 0.f ? z.z : 0.01f * z.z) * g.z + (z.w > 0.f ? z.w : 0.01f * z.w) * g.w;
          }
        } else {
          for (int j = lane; j < Hd; j += 64) {
            float z = zM[h * Hd + j];
            part += (z > 0.f ? z : 0.01f * z) * gSn[h * Hd + j];
          }
        }
        part = wave_sum_l(part);
        if (lane == 0) tt[(long)t * H + h] = part + gs[(long)n * H + h];
      }
    }
  }
  __syncthreads();
  // ---- 2. softmax backward, one thread per (segment, head) ----
  if (tid < (n1 - n0) * H) {
    const int n = n0 + tid / H, h = tid % H;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 <= SEGB_LONG) {
      float dot = 0.f;
      for (int t = r0; t < r1; ++t) dot += alpha[(long)t * H + h] * tt[(long)t * H + h];
      for (int t = r0; t < r1; ++t) ga[(long)t * H + h] = alpha[(long)t * H + h] * (tt[(long)t * H + h] - dot);
    }
  }
  // a long segment (a hub atom: 20 000 incoming edges in the test): the whole workgroup strides over its rows, the dot
  // product through wavefront + LDS reductions in a fixed order -- one thread walking 2 x 20 000 dependent loads per
  // head took milliseconds
  for (int n = n0; n < n1; ++n) {                  // (uniform: every thread sees the same segment lengths)
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 <= SEGB_LONG) continue;
    __shared__ float red4[4];
    for (int h = 0; h < H; ++h) {
      float dot = 0.f;
      for (int t = r0 + tid; t < r1; t += 256) dot += alpha[(long)t * H + h] * tt[(long)t * H + h];
      dot = wave_sum_l(dot);
      __syncthreads();
      if (lane == 0) red4[wave] = dot;
      __syncthreads();
      dot = (red4[0] + red4[1]) + (red4[2] + red4[3]);
      for (int t = r0 + tid; t < r1; t += 256) ga[(long)t * H + h] = alpha[(long)t * H + h] * (tt[(long)t * H + h] - dot);
    }
  }
  __syncthreads();
  // ---- 3. gZ rows, their segment sum, partial sums for grad wA_out (a thread keeps its columns for all segments) ----
  for (int n = n0; n < n1; ++n) {
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 == r0) {  // no incoming edge: zero row of the segment sum
      for (int c = tid; c < W2; c += 256) Gi[(long)n * W2 + c] = 0.f;
      continue;
    }
    const float* gSn = gS + (long)n * HHd;
    if (VEC) {  // four consecutive columns per thread (a head boundary is a multiple of 4); rows four at a time
      for (int c4 = tid; c4 < (fuse_m ? HHd : W2) / 4; c4 += 256) {   // (fuse_m: the message half is done)
        const int col = 4 * c4;
        const bool isA = col < HHd;
        const int cc = isA ? col : col - HHd;
        const int h = cc / Hd;
        const float4 wv = isA ? *reinterpret_cast<const float4*>(wA_out + cc) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 gsv = isA ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4*>(gSn + cc);
        const float* coef = isA ? ga : alpha;
        float4 gi = make_float4(0.f, 0.f, 0.f, 0.f), ps = gi;
        // Rows four at a time, the NEXT four loaded before this batch's gZ stores are issued: vmcnt retires in order
        // and counts stores, so a load issued after a store cannot be waited for without draining that store -- with
        // load / store / load / ... every batch paid the full write latency.
        float4 zn[4];
        float cn[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = r0 + u < r1 ? r0 + u : r1 - 1;
          zn[u] = ZB ? load4_bf16(reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + col)
                     : *reinterpret_cast<const float4*>(Z + (long)t * W2 + col);
          cn[u] = coef[(long)t * H + h];
        }
        for (int tb = r0; tb < r1; tb += 4) {
          float4 zv[4];
          float cf[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { zv[u] = zn[u]; cf[u] = cn[u]; }
          if (tb + 4 < r1) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int t = tb + 4 + u < r1 ? tb + 4 + u : r1 - 1;
              zn[u] = ZB ? load4_bf16(reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + col)
                         : *reinterpret_cast<const float4*>(Z + (long)t * W2 + col);
              cn[u] = coef[(long)t * H + h];
            }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = tb + u;
            if (t < r1) {
              const float4 z = zv[u];
              const float4 d = make_float4(z.x > 0.f ? 1.f : 0.01f, z.y > 0.f ? 1.f : 0.01f, z.z > 0.f ? 1.f : 0.01f,
                                           z.w > 0.f ? 1.f : 0.01f);
              float4 g;
              if (isA) {
                const float gav = cf[u];
                g = make_float4(gav * wv.x * d.x, gav * wv.y * d.y, gav * wv.z * d.z, gav * wv.w * d.w);
                ps.x += gav * z.x * d.x; ps.y += gav * z.y * d.y; ps.z += gav * z.z * d.z; ps.w += gav * z.w * d.w;
              } else {
                const float al = cf[u];
                g = make_float4(al * gsv.x * d.x, al * gsv.y * d.y, al * gsv.z * d.z, al * gsv.w * d.w);
              }
              if (mask) {
                // four sign bits per lane, eight lanes per 32-column word: OR across the eight lanes (two quad
                // permutations and the half-row mirror), lane 0 of each group stores the word
                unsigned w = ((z.x > 0.f ? 1u : 0u) | (z.y > 0.f ? 2u : 0u) | (z.z > 0.f ? 4u : 0u) | (z.w > 0.f ? 8u : 0u))
                             << (4 * (lane & 7));
                w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
                w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
                w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x141, 0xF, 0xF, true);   // row_half_mirror
                if ((lane & 7) == 0) mask[(long)t * (W2 >> 5) + (col >> 5)] = w;
              } else {
                const long doff = gz_block ? (long)(col >> 7) * gz_block + (long)t * 128 + (col & 127) : (long)t * W2 + col;
                *reinterpret_cast<float4*>(gZ + doff) = g;
              }
              gm = fmaxf(fmaxf(gm, fmaxf(fabsf(g.x), fabsf(g.y))), fmaxf(fabsf(g.z), fabsf(g.w)));
              gi.x += g.x; gi.y += g.y; gi.z += g.z; gi.w += g.w;
            }
          }
        }
        *reinterpret_cast<float4*>(Gi + (long)n * W2 + col) = gi;
        gim_max = fmaxf(fmaxf(gim_max, fmaxf(fabsf(gi.x), fabsf(gi.y))), fmaxf(fabsf(gi.z), fabsf(gi.w)));
        if (isA) {
          pw[cc] += ps.x; pw[cc + 1] += ps.y; pw[cc + 2] += ps.z; pw[cc + 3] += ps.w;
        }
      }
    } else {
      for (int col = tid; col < W2; col += 256) {
        const bool isA = col < HHd;
        const int cc = isA ? col : col - HHd;
        const int h = cc / Hd;
        const float wv = isA ? wA_out[cc] : 0.f;
        const float gsv = isA ? 0.f : gSn[cc];
        float gi = 0.f, ps = 0.f;
        for (int t = r0; t < r1; ++t) {
          const float z = Z[(long)t * W2 + col];
          const float d = z > 0.f ? 1.f : 0.01f;
          float g;
          if (isA) {
            const float gav = ga[(long)t * H + h];
            g = gav * wv * d;
            ps += gav * z * d;
          } else {
            g = alpha[(long)t * H + h] * gsv * d;
          }
          if (gz_block) gZ[(long)(col >> 7) * gz_block + (long)t * 128 + (col & 127)] = g;
          else gZ[(long)t * W2 + col] = g;
          gi += g;
        }
        Gi[(long)n * W2 + col] = gi;
        if (isA) pw[cc] += ps;
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < HHd; c += 256) partialW[(long)blockIdx.x * HHd + c] = pw[c];
  if (VEC && gzmax) block_absmax_commit(gm, gzmax);
  if (VEC && gimax) {
    __syncthreads();                               // (the commit's staging words are shared by the two calls)
    block_absmax_commit(gim_max, gimax);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same backward as THREE small kernels (round 3; sign-bit form at Hd = 256, fp32 Z): the three steps of
// edge_seg_bwd_kernel talk through global memory anyway (tt, ga), and as one kernel it needs 106 VGPRs -- one wave per SIMD
// beside the side stream's dT workgroups (2 x 192 VGPRs), i.e. a quarter of its occupancy when the two share a CU.  At
// <= 64 VGPRs two waves per SIMD fit beside them: the HBM-bound passes over Z then run ON the CUs the matrix-bound
// contraction occupies instead of beside them on the other half of the chip (DESIGN.md §5 Streams).  Same operations in
// the same order per output element: results are bit-identical to the one-kernel form.
//   seg_bwd_msg_kernel   step 1: one wave per (segment, head): g_alpha, the message half's sign bits, its share of Gi
//   seg_bwd_soft_kernel  step 2: softmax backward per (segment, head)
//   seg_bwd_att_kernel   step 3: the attention half: sign bits, Gi share, partial sums for grad fc_out_A
template <bool ZB = false>   // ZB: Z is read as bf16 (the "bf16" edge-storage mode; offsets count elements either way)
__global__ __launch_bounds__(256, 8) void seg_bwd_msg_kernel(const float* __restrict__ Z, const float* __restrict__ alpha,
                                                             const float* __restrict__ gS, const float* __restrict__ gs,
                                                             const int* __restrict__ rowptr, int N, int H,
                                                             float* __restrict__ tt, float* __restrict__ Gi,
                                                             float* __restrict__ gzmax, unsigned* __restrict__ mask,
                                                             float* __restrict__ gimax) {
  constexpr int Hd = 256;
  const int HHd = H * Hd, W2 = 2 * HHd;
  const int tid = threadIdx.x, lane = tid & 63;
  // wave-uniform values are made SCALAR (readfirstlane): the row index, the segment bounds and every row base address then
  // live in SGPRs -- as vector values they cost the 30 VGPRs that did not fit under the 64 this kernel is built for
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  float gm = 0.f, gim_max = 0.f;
  const long ntask = (long)N * H;
  for (long task = (long)blockIdx.x * 4 + wave; task < ntask; task += (long)gridDim.x * 4) {
    const int n = (int)(task / H), h = (int)(task - (long)n * H);
    const int r0 = __builtin_amdgcn_readfirstlane(rowptr[n]), r1 = __builtin_amdgcn_readfirstlane(rowptr[n + 1]);
    if (r1 == r0) continue;                        // (seg_bwd_att_kernel zero-fills the whole Gi row of an empty segment)
    const int wcol = HHd + h * Hd + 4 * lane;
    const float4 g = *reinterpret_cast<const float4*>(gS + (long)n * HHd + h * Hd + 4 * lane);
    const float gsn = gs[(long)n * H + h];
    float4 gim = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int tb = r0; tb < r1; tb += 4) {
      float4 zv[4];
      float al[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = tb + u < r1 ? tb + u : r1 - 1;
        zv[u] = ZB ? load4_bf16(reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + wcol)
                   : *reinterpret_cast<const float4*>(Z + (long)t * W2 + wcol);
        al[u] = alpha[(long)t * H + h];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int t = tb + u;
        if (t < r1) {
          const float4 z = zv[u];
          float part = (z.x > 0.f ? z.x : 0.01f * z.x) * g.x + (z.y > 0.f ? z.y : 0.01f * z.y) * g.y +
                       (z.z > 0.f ? z.z : 0.01f * z.z) * g.z + (z.w > 0.f ? z.w : 0.01f * z.w) * g.w;
          part = wave_sum_l(part);
          if (lane == 0) tt[(long)t * H + h] = part + gsn;
          const float a_ = al[u];
          const float4 gz = make_float4(a_ * g.x * (z.x > 0.f ? 1.f : 0.01f), a_ * g.y * (z.y > 0.f ? 1.f : 0.01f),
                                        a_ * g.z * (z.z > 0.f ? 1.f : 0.01f), a_ * g.w * (z.w > 0.f ? 1.f : 0.01f));
          gm = fmaxf(fmaxf(gm, fmaxf(fabsf(gz.x), fabsf(gz.y))), fmaxf(fabsf(gz.z), fabsf(gz.w)));
          gim.x += gz.x; gim.y += gz.y; gim.z += gz.z; gim.w += gz.w;
          unsigned w = ((z.x > 0.f ? 1u : 0u) | (z.y > 0.f ? 2u : 0u) | (z.z > 0.f ? 4u : 0u) | (z.w > 0.f ? 8u : 0u))
                       << (4 * (lane & 7));
          w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
          w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
          w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x141, 0xF, 0xF, true);   // row_half_mirror
          if ((lane & 7) == 0) mask[(long)t * (W2 >> 5) + (wcol >> 5)] = w;
        }
      }
    }
    *reinterpret_cast<float4*>(Gi + (long)n * W2 + wcol) = gim;
    gim_max = fmaxf(fmaxf(gim_max, fmaxf(fabsf(gim.x), fabsf(gim.y))), fmaxf(fabsf(gim.z), fabsf(gim.w)));
  }
  if (gzmax) block_absmax_commit(gm, gzmax);
  if (gimax) {
    __syncthreads();                               // (the commit's staging words are shared by the two calls)
    block_absmax_commit(gim_max, gimax);
  }
}

__global__ __launch_bounds__(256, 8) void seg_bwd_soft_kernel(const float* __restrict__ alpha, const float* __restrict__ tt,
                                                              const int* __restrict__ rowptr, int N, int H,
                                                              float* __restrict__ ga) {
  __shared__ float red4[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * SEGB_NODES, n1 = min(N, n0 + SEGB_NODES);
  if (tid < (n1 - n0) * H) {
    const int n = n0 + tid / H, h = tid % H;
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 <= SEGB_LONG) {
      float dot = 0.f;
      for (int t = r0; t < r1; ++t) dot += alpha[(long)t * H + h] * tt[(long)t * H + h];
      for (int t = r0; t < r1; ++t) ga[(long)t * H + h] = alpha[(long)t * H + h] * (tt[(long)t * H + h] - dot);
    }
  }
  for (int n = n0; n < n1; ++n) {                  // long segments: the whole workgroup (see edge_seg_bwd_kernel)
    const int r0 = rowptr[n], r1 = rowptr[n + 1];
    if (r1 - r0 <= SEGB_LONG) continue;
    for (int h = 0; h < H; ++h) {
      float dot = 0.f;
      for (int t = r0 + tid; t < r1; t += 256) dot += alpha[(long)t * H + h] * tt[(long)t * H + h];
      dot = wave_sum_l(dot);
      __syncthreads();
      if (lane == 0) red4[wave] = dot;
      __syncthreads();
      dot = (red4[0] + red4[1]) + (red4[2] + red4[3]);
      for (int t = r0 + tid; t < r1; t += 256) ga[(long)t * H + h] = alpha[(long)t * H + h] * (tt[(long)t * H + h] - dot);
    }
  }
}

template <bool ZB = false>
__global__ __launch_bounds__(256, 8) void seg_bwd_att_kernel(const float* __restrict__ Z, const float* __restrict__ ga,
                                                             const int* __restrict__ rowptr,
                                                             const float* __restrict__ wA_out, int N, int H,
                                                             float* __restrict__ Gi, float* __restrict__ partialW,
                                                             float* __restrict__ gzmax, unsigned* __restrict__ mask,
                                                             float* __restrict__ gimax) {
  constexpr int Hd = 256;
  extern __shared__ float pw[];                    // [HHd] per-column partial sums of g_a * leaky(zA)
  const int HHd = H * Hd, W2 = 2 * HHd;
  const int tid = threadIdx.x, lane = tid & 63;
  float gm = 0.f, gim_max = 0.f;
  for (int c = tid; c < HHd; c += 256) pw[c] = 0.f;
  __syncthreads();
  const int n0 = blockIdx.x * SEGB_NODES, n1 = min(N, n0 + SEGB_NODES);
  for (int n = n0; n < n1; ++n) {
    const int r0 = __builtin_amdgcn_readfirstlane(rowptr[n]), r1 = __builtin_amdgcn_readfirstlane(rowptr[n + 1]);
    if (r1 == r0) {  // no incoming edge: zero row of the segment sum (both halves)
      for (int c = tid; c < W2; c += 256) Gi[(long)n * W2 + c] = 0.f;
      continue;
    }
    for (int c4 = tid; c4 < HHd / 4; c4 += 256) {
      const int col = 4 * c4;
      const int h = col / Hd;
      const float4 wv = *reinterpret_cast<const float4*>(wA_out + col);
      float4 gi = make_float4(0.f, 0.f, 0.f, 0.f), ps = gi;
      for (int tb = r0; tb < r1; tb += 4) {
        float4 zv[4];
        float cf[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = tb + u < r1 ? tb + u : r1 - 1;
          zv[u] = ZB ? load4_bf16(reinterpret_cast<const __bf16*>(Z) + (long)t * W2 + col)
                     : *reinterpret_cast<const float4*>(Z + (long)t * W2 + col);
          cf[u] = ga[(long)t * H + h];
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
            unsigned w = ((z.x > 0.f ? 1u : 0u) | (z.y > 0.f ? 2u : 0u) | (z.z > 0.f ? 4u : 0u) | (z.w > 0.f ? 8u : 0u))
                         << (4 * (lane & 7));
            w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
            w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
            w |= (unsigned)__builtin_amdgcn_mov_dpp((int)w, 0x141, 0xF, 0xF, true);   // row_half_mirror
            if ((lane & 7) == 0) mask[(long)t * (W2 >> 5) + (col >> 5)] = w;
            gm = fmaxf(fmaxf(gm, fmaxf(fabsf(g.x), fabsf(g.y))), fmaxf(fabsf(g.z), fabsf(g.w)));
            gi.x += g.x; gi.y += g.y; gi.z += g.z; gi.w += g.w;
          }
        }
      }
      *reinterpret_cast<float4*>(Gi + (long)n * W2 + col) = gi;
      gim_max = fmaxf(fmaxf(gim_max, fmaxf(fabsf(gi.x), fabsf(gi.y))), fmaxf(fabsf(gi.z), fabsf(gi.w)));
      pw[col] += ps.x; pw[col + 1] += ps.y; pw[col + 2] += ps.z; pw[col + 3] += ps.w;
    }
  }
  __syncthreads();
  for (int c = tid; c < HHd; c += 256) partialW[(long)blockIdx.x * HHd + c] = pw[c];
  if (gzmax) block_absmax_commit(gm, gzmax);
  if (gimax) {
    __syncthreads();
    block_absmax_commit(gim_max, gimax);
  }
}

// The attention half under the bit form of the saved buffer (the forward is edge_z6w_kernel<false, 3>):
// no Z_A exists.  The attention columns of the buffer's rows hold, instead,
//   rows n < N        Pi_A[n, :]   the attention half of the x_i projection, bias included   (leading dimension W2)
//   rows N + n        Pj_A[n, :]   ... of the x_j projection
//   rows 2 N + g      the sign words of edge rows 32 g .. 32 g + 31, word-major: word w of row t at [w * 32 + (t & 31)],
//                     bit i of word w = (Z_A[t, 32 w + i] > 0)
// Per (node, four columns) wA and Pi_A[n] are loaded once; per edge of the segment, in ascending order, the mask word,
// g_a[t, h], the source node and four floats of its Pj_A row (a crystal's rows: L2, as in the forward's gathers).
//   * mask: the attention words of the backward's sign mask, in the layout EdgeRC expects -- the loaded word as it is;
//   * Gi: seg_bwd_att_kernel's operations in its order, g = gav * wv * d; gi += g: the same bits;
//   * partialW: sum_t (gav d) (Pi_A + Pj_A), the node part T_ij of grad fc_out_A; the edge part
//     T_e = sum_k W_e u is added by edge_gw_bit_reduce_kernel from the column sums it holds.  LeakyReLU(z) = d z and
//     z = W_e e + Pi + Pj; no division by wA anywhere, so a zero entry of wA keeps its true gradient.
__global__ __launch_bounds__(256, 8) void seg_bwd_attb_kernel(const float* __restrict__ saved, const float* __restrict__ ga,
                                                              const int* __restrict__ rowptr, const int* __restrict__ srcs,
                                                              const float* __restrict__ wA_out, int N, int H,
                                                              float* __restrict__ Gi, float* __restrict__ partialW,
                                                              unsigned* __restrict__ mask) {
  constexpr int Hd = 256;
  extern __shared__ float pw[];                    // [HHd] per-column partial sums
  const int HHd = H * Hd, W2 = 2 * HHd;
  const int tid = threadIdx.x, lane = tid & 63;
  const float* PiA = saved;
  const float* PjA = saved + (long)N * W2;
  const unsigned* zb = reinterpret_cast<const unsigned*>(saved + 2l * N * W2);
  for (int c = tid; c < HHd; c += 256) pw[c] = 0.f;
  __syncthreads();
  const int n0 = blockIdx.x * SEGB_NODES, n1 = min(N, n0 + SEGB_NODES);
  for (int n = n0; n < n1; ++n) {
    const int r0 = __builtin_amdgcn_readfirstlane(rowptr[n]), r1 = __builtin_amdgcn_readfirstlane(rowptr[n + 1]);
    if (r1 == r0) {  // no incoming edge: zero row of the segment sum (both halves)
      for (int c = tid; c < W2; c += 256) Gi[(long)n * W2 + c] = 0.f;
      continue;
    }
    for (int c4 = tid; c4 < HHd / 4; c4 += 256) {
      const int col = 4 * c4;
      const int h = col / Hd;
      const int bit = col & 31;
      const unsigned* zw = zb + (col >> 5) * 32;
      const unsigned woff = (unsigned)(col >> 5) * 4u;
      const float4 wv = *reinterpret_cast<const float4*>(wA_out + col);
      const float4 pi = *reinterpret_cast<const float4*>(PiA + (long)n * W2 + col);
      float4 gi = make_float4(0.f, 0.f, 0.f, 0.f), ps = gi;
      for (int tb = r0; tb < r1; tb += 4) {
        unsigned m[4];
        float cf[4];
        int sn[4];
        float4 pj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = tb + u < r1 ? tb + u : r1 - 1;
          m[u] = zw[(long)(t >> 5) * W2 + (t & 31)];
          cf[u] = ga[(long)t * H + h];
          sn[u] = srcs[t];   // (wave-uniform address: t is)
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)   // (32-bit byte offsets: N * W2 * 4 < 2^32 where the forward takes this form)
          pj[u] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(PjA) +
                                                   ((unsigned)sn[u] * (unsigned)W2 + (unsigned)col) * 4u);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = tb + u;
          if (t < r1) {
            const unsigned mb = m[u] >> bit;
            const float4 d = make_float4((mb & 1u) ? 1.f : 0.01f, (mb & 2u) ? 1.f : 0.01f, (mb & 4u) ? 1.f : 0.01f,
                                         (mb & 8u) ? 1.f : 0.01f);
            const float gav = cf[u];
            const float4 g = make_float4(gav * wv.x * d.x, gav * wv.y * d.y, gav * wv.z * d.z, gav * wv.w * d.w);
            ps.x += (gav * d.x) * (pi.x + pj[u].x); ps.y += (gav * d.y) * (pi.y + pj[u].y);
            ps.z += (gav * d.z) * (pi.z + pj[u].z); ps.w += (gav * d.w) * (pi.w + pj[u].w);
            // (a wave-uniform row base and a 32-bit lane offset, laundered so that no 64-bit lane address per unrolled
            // row is kept across the loop: those spilled to scratch)
            if ((lane & 7) == 0) {
              unsigned wo = woff;
              asm volatile("" : "+v"(wo));
              *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(mask + (long)t * (W2 >> 5)) + wo) = m[u];
            }
            gi.x += g.x; gi.y += g.y; gi.z += g.z; gi.w += g.w;
          }
        }
      }
      *reinterpret_cast<float4*>(Gi + (long)n * W2 + col) = gi;
      pw[col] += ps.x; pw[col + 1] += ps.y; pw[col + 2] += ps.z; pw[col + 3] += ps.w;
    }
  }
  __syncthreads();
  for (int c = tid; c < HHd; c += 256) partialW[(long)blockIdx.x * HHd + c] = pw[c];
}

// ---- debug: the sign pattern of the saved pre-activations in original edge order (include/cgat_hip.h) ----
// zbits (the bit form of the saved buffer): the attention columns' signs are the stored words (see seg_bwd_attb_kernel)
__global__ void attn_signs_kernel(const float* __restrict__ Z, const int* __restrict__ perm, long E, int W2,
                                  uint8_t* __restrict__ mask, const unsigned* __restrict__ zbits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= E * W2) return;
  const long t = i / W2;
  const int c = (int)(i - t * W2);
  if (zbits && c < W2 / 2) mask[(long)perm[t] * W2 + c] = (zbits[(t >> 5) * W2 + (c >> 5) * 32 + (t & 31)] >> (c & 31)) & 1u;
  else mask[(long)perm[t] * W2 + c] = Z[i] > 0.f ? 1 : 0;
}
int attn_signs_launch(const float* Z, const int* perm, long E, int W2, uint8_t* mask, hipStream_t stream,
                      const unsigned* zbits) {
  const long n = E * W2;
  if (n == 0) return CGAT_OK;
  hipLaunchKernelGGL(attn_signs_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, Z, perm, E, W2, mask, zbits);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

int edge_seg_bwd_chunks(int N) { return cdiv(N > 0 ? N : 1, SEGB_NODES); }

// step 2 alone, for the indexed training route (edgeidx.hip), whose steps 1 and 3 form z instead of reading Z
int seg_bwd_soft_launch(const float* alpha, const float* tt, const int* rowptr, int N, int H, float* ga, hipStream_t stream) {
  CGAT_CHECK_ARG(H >= 1 && H <= 16, "seg_bwd_soft: more than 16 heads");
  if (N <= 0) return CGAT_OK;
  CGAT_PROF("edge_idx_bwd_soft", stream);
  hipLaunchKernelGGL(seg_bwd_soft_kernel, dim3(edge_seg_bwd_chunks(N)), dim3(256), 0, stream, alpha, tt, rowptr, N, H, ga);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// the three small kernels (<= 64 VGPRs: they co-reside with the side stream's dT workgroups); bit-identical results
template <bool ZB>
static int seg_bwd_three_launch(const float* Z, const float* alpha, const float* gS, const float* gs, const int* rowptr,
                                const float* wA_out, int N, int H, float* tt, float* ga, float* Gi, float* partialW,
                                float* gzmax, unsigned* mask, float* gimax, hipStream_t stream,
                                const int* srcs = nullptr) {   // srcs: the bit form of the saved buffer (seg_bwd_attb_kernel)
  const int chunks = edge_seg_bwd_chunks(N);
  hipLaunchKernelGGL(seg_bwd_msg_kernel<ZB>, dim3((unsigned)cdiv((long)N * H, 4)), dim3(256), 0, stream, Z, alpha, gS, gs, rowptr,
                     N, H, tt, Gi, gzmax, mask, gimax);
  CGAT_LAUNCH_CHECK();
  hipLaunchKernelGGL(seg_bwd_soft_kernel, dim3(chunks), dim3(256), 0, stream, alpha, tt, rowptr, N, H, ga);
  CGAT_LAUNCH_CHECK();
  if (srcs)
    hipLaunchKernelGGL(seg_bwd_attb_kernel, dim3(chunks), dim3(256), (size_t)H * 256 * sizeof(float), stream, Z, ga, rowptr,
                       srcs, wA_out, N, H, Gi, partialW, mask);
  else
  hipLaunchKernelGGL(seg_bwd_att_kernel<ZB>, dim3(chunks), dim3(256), (size_t)H * 256 * sizeof(float), stream, Z, ga, rowptr,
                     wA_out, N, H, Gi, partialW, gzmax, mask, gimax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

int edge_seg_bwd_launch(const float* Z, float* gZ, long gz_block, const float* alpha, const float* gS, const float* gs,
                        const int* rowptr, const float* wA_out, int N, int H, int Hd, float* tt, float* ga, float* Gi,
                        float* partialW, float* gzmax, unsigned* mask, float* gimax, bool vec, bool zb_6, bool zb,
                        bool rc_shape, bool have_scales, hipStream_t stream, const int* bits_src) {
  CGAT_CHECK_ARG(H <= 16, "nodes_attention_backward: more than 16 heads");
  CGAT_CHECK_ARG(!bits_src || (vec && mask && Hd == 256 && !zb && !zb_6 && !have_scales),
                 "nodes_attention_backward: the bit form of the saved buffer is the three-kernel fp32 route's");
  CGAT_PROF("edge_seg_bwd", stream);
  if (have_scales) CGAT_TRY(fill_launch(gzmax, 0.f, 8, stream));   // the maxima gzmax[0..7] the kernels and the caller fold into
  const int chunks = edge_seg_bwd_chunks(N);
  const size_t shm = (size_t)H * Hd * sizeof(float);
  if (zb_6) {
    CGAT_CHECK_ARG(vec && mask && Hd == 256, "nodes_attention_backward: the bf16 edge storage needs the vector form");
    return seg_bwd_three_launch<true>(Z, alpha, gS, gs, rowptr, wA_out, N, H, tt, ga, Gi, partialW, gzmax, mask, gimax, stream);
  }
  if (zb) {
    CGAT_CHECK_ARG(rc_shape && have_scales, "nodes_attention_backward: the bf16 edge storage needs the vector form");
    hipLaunchKernelGGL((edge_seg_bwd_kernel<true, true>), dim3(chunks), dim3(256), shm, stream, Z, gZ, gz_block, alpha, gS,
                       gs, rowptr, wA_out, N, H, Hd, tt, ga, Gi, partialW, gzmax, mask, gimax);
  } else if (vec && mask && Hd == 256) {
    return seg_bwd_three_launch<false>(Z, alpha, gS, gs, rowptr, wA_out, N, H, tt, ga, Gi, partialW, gzmax, mask, gimax, stream,
                                       bits_src);
  } else if (vec)
    hipLaunchKernelGGL(edge_seg_bwd_kernel<true>, dim3(chunks), dim3(256), shm, stream, Z, gZ, gz_block, alpha, gS, gs,
                       rowptr, wA_out, N, H, Hd, tt, ga, Gi, partialW, gzmax, mask, gimax);
  else
    hipLaunchKernelGGL(edge_seg_bwd_kernel<false>, dim3(chunks), dim3(256), shm, stream, Z, gZ, gz_block, alpha, gS, gs,
                       rowptr, wA_out, N, H, Hd, tt, ga, Gi, partialW, (float*)nullptr, (unsigned*)nullptr, (float*)nullptr);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
