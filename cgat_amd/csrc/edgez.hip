// Edge pre-activations of both message networks, the per-edge part of the operand-split first conv
// (reference CGAT.py:96 MultiHeadNetwork.fc_in applied to cat([x_i, edge_attr, x_j]), CGAT.py:316-318):
//     Z[t, :] = W_e e[perm[t]] + Pi[dst[t], :] + Pj[src[t], :]            t = destination-sorted edge slot
// fused with the attention logits of MH_A (CGAT.py:97-98: fc_out(LeakyReLU(fc_in(.))), one output per head):
//     a[t, h] = b_A[h] + sum_j leaky(Z[t, h*Hd + j]) * w_A[h*Hd + j]
//
// Shape: E x 1536 outputs with K = Ce = 128.  The product runs on the matrix cores in the split-bf16
// arithmetic of bilinear.hip (three bf16 planes per fp32 operand, six v_mfma_f32_16x16x32_bf16 passes,
// fp32 accumulation: fp32-equivalent), organised like the hypernetwork kernel: a wave's 32 edge rows are
// split once and stay in 96 VGPRs, the pre-split weight column blocks stream through a 4-slot LDS ring by
// LDS-DMA (12-KB chunks = one 32-deep k-step of 64 columns), fragments are read one group ahead.  The
// kernel is bound by its epilogue traffic -- per edge 6 KB of Z written and 6 KB of Pj gathered (Pi rows
// are shared by the edges of a destination segment and hit L2) -- so two 4-wave workgroups share a CU:
// while one gathers/stores a 64-column slice, the other one runs MFMAs.
//
// vmcnt bookkeeping: the ring's counted waits assume that the three LDS-DMA loads of the current
// iteration are the youngest vector-memory operations; the epilogue's ordinary loads and stores are older
// than the next iteration's LDS-DMA loads, so a counted wait can only be stricter than needed, never looser
// (vmcnt retires in order).  RAW/WAR reasoning of the ring: bilinear.hip.
//
// Packed math: when hipcc SLP-packs the two rows' logit accumulations into v_pk_mul/v_pk_fma_f32, the logits come
// out slightly wrong and differ from run to run on MI355X (Z, computed from the same registers, stays bit-exact;
// found by tests/test_hip_golden.py::test_determinism_bitwise, bisected with an empty asm between the two
// accumulations).  This file is therefore built with -fno-slp-vectorize and the two accumulators are pinned apart.
//
// Kernels in this file (round 5): edge_z_kernel (below: 128-row workgroups; the per-node projections, the dense layer at
// width 128, and the per-edge launch of shapes / modes the wide-tile kernels do not take), edge_z6w_kernel (the per-edge
// launch of the default 24-bit modes: the same six-pass arithmetic on 256-row workgroups, bit-identical, 3.20 -> 2.84 ms),
// edge_zx_kernel (f16x3 mode, K = 256).
#include "../../include/cgat_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

// ZB (the per-edge launch only): Z is stored as bf16 (the "bf16" edge-storage mode, BASELINE configs[4]; ldz counts
// elements either way).  The logits are formed from the unrounded values.
template <int PASSES, bool ADDS, bool ZB = false>
__global__ __launch_bounds__(256, 2) void edge_z_kernel(const float* __restrict__ e, long lde,
                                                        const int* __restrict__ perm, const uint4* __restrict__ Wq,
                                                        int ncb, const float* __restrict__ Pi,
                                                        const int* __restrict__ dsti, const float* __restrict__ Pj,
                                                        const int* __restrict__ srci, long ld_add,
                                                        float* __restrict__ Z, long ldz, int E,
                                                        const float* __restrict__ wA, const float* __restrict__ bA,
                                                        int H, int cb_per_head, float* __restrict__ a_out, int act,
                                                        int accumulate, float* __restrict__ omax,
                                                        const float* __restrict__ dact, long ld_dact, HeadBatch hb) {
  // grid.y = head of a multi-head second layer (linear128_heads_launch): every operand moves by its per-head offset
  e += (long)blockIdx.y * hb.in;
  Wq += (long)blockIdx.y * hb.w;
  Z += (long)blockIdx.y * hb.out;
  if (Pi) Pi += (long)blockIdx.y * hb.bias;
  if (dact) dact += (long)blockIdx.y * hb.dact;
  if (ADDS) Pj += (long)blockIdx.y * hb.add2;
  constexpr bool F16 = PASSES == 2;             // two fp16 planes, three passes (mfma_bf16.h): rows scaled per row,
  constexpr int NP = F16 ? 2 : 3;               // the weight per 128-column block (wmax behind the planes)
  constexpr int CH16 = NP * 4 * 64;             // 16-byte pieces per chunk = 12 KB (8 KB)
  // DEEP (the per-edge launch in the fp16 form): 8 ring slots, vmcnt allowances that let the epilogue's stores stay
  // in flight, all gathers of a slice before its first store, unconditional stores (see edge_zx_kernel's header)
  constexpr bool DEEP = F16 && ADDS;
  constexpr bool ALT = true;                    // odd k-steps into a second, subtracted accumulator set (see below)
  constexpr int RING = DEEP ? 8 : 4;
  __shared__ uint4 smem[RING * CH16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int row_w = blockIdx.x * 128 + wave * 32;
  const int row_a = row_w + n16, row_b = row_a + 16;
  const int rca = row_a < E ? row_a : E - 1, rcb = row_b < E ? row_b : E - 1;
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + lane;
  const unsigned t_off = (unsigned)tid * 16;
  const long last_chunk = (long)ncb * 8 - 1;

  // the lane's two edge rows, split once: q[plane][2 s + nb] holds e[row(nb), 32 s + 8 kg + 0..7]
  bf16x8 q1[8], q2[8], q3[F16 ? 1 : 8];
  float rs_a = 1.f, rs_b = 1.f;                 // F16: 1 / scale of the lane's two rows
  const float* wmax = reinterpret_cast<const float*>(Wq + (long)ncb * 8 * CH16);   // F16: max |W| per column block
  {
    const long ea = perm ? perm[rca] : rca, eb = perm ? perm[rcb] : rcb;
    if constexpr (F16) {
      float qv[2][32];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float4* qp = reinterpret_cast<const float4*>(e + (nb ? eb : ea) * lde + 32 * s + 8 * kg);
          const float4 t0 = qp[0], t1 = qp[1];
          qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
          qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
        }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
        m = fmaxf(m, __shfl_xor(m, 16));        // the row's 128 values live in the four lanes n16 + 16 kg
        m = fmaxf(m, __shfl_xor(m, 32));
        float sq, iq;
        pow2_scale(m, sq, iq);
        (nb ? rs_b : rs_a) = iq;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = qv[nb][8 * s + j] * sq;
          split2_x8_f16(v, q1[2 * s + nb], q2[2 * s + nb]);
        }
      }
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const float4* qp = reinterpret_cast<const float4*>(e + (nb ? eb : ea) * lde + 32 * s + 8 * kg);
          const float4 t0 = qp[0], t1 = qp[1];
          const float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
          split3_x8(v, q1[2 * s + nb], q2[2 * s + nb], q3[2 * s + nb]);
        }
    }
  }
  // The matrix instruction's accumulator rounds with a sign-independent bias (-0.9e-9 of sum |x||w| on every
  // output of this kernel when the four k-steps of a slice accumulated straight into one accumulator: 50-100 x the
  // statistical level, tools/f16_bias_probe.py).  The odd k-steps therefore multiply the NEGATED row fragments into a
  // second accumulator set that is subtracted before the epilogue: their bias has the opposite sign in the result.
  if constexpr (ALT) {
#pragma unroll
    for (int s = 1; s < 4; s += 2)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        q1[2 * s + nb] = neg_x8(q1[2 * s + nb]);
        q2[2 * s + nb] = neg_x8(q2[2 * s + nb]);
        if constexpr (!F16) q3[2 * s + nb] = neg_x8(q3[2 * s + nb]);
      }
  }
  // ADDS: gathered addends Pi[dst], Pj[src] (the edge kernel).  !ADDS: a plain product plus bias, Pi = the bias
  // vector or null (the per-node projections x W_i^T + b and x W_j^T, same kernel with e = x)
  const float* pia = ADDS ? Pi + (long)dsti[rca] * ld_add : Pi;
  const float* pib = ADDS ? Pi + (long)dsti[rcb] * ld_add : Pi;
  const float* pja = ADDS ? Pj + (long)srci[rca] * ld_add : nullptr;
  const float* pjb = ADDS ? Pj + (long)srci[rcb] * ld_add : nullptr;
  float* za = Z + (long)rca * ldz;
  float* zb = Z + (long)rcb * ldz;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#define EZ_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const uint4* tb = Wq + gi * CH16;                                                          \
    const unsigned dst = wave_t + (unsigned)((gi_) & (RING - 1)) * (CH16 * 16);                \
    glds_b128(tb, t_off, dst);                                                                 \
    glds_b128(tb + 256, t_off, dst + 4096);                                                    \
    if (NP == 3) glds_b128(tb + 512, t_off, dst + 8192);                                       \
  }
  EZ_TLOAD(0l);
  EZ_TLOAD(1l);
  EZ_TLOAD(2l);
  if constexpr (DEEP) { EZ_TLOAD(3l); EZ_TLOAD(4l); EZ_TLOAD(5l); EZ_TLOAD(6l); }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fa3, fb1, fb2, fb3;
  // group = the three planes of one 16-column block of the chunk in ring slot slot_
#define EZ_READ(F1_, F2_, F3_, slot_, cb_)                                                     \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * (CH16) + (cb_) * 64;                                   \
    F1_ = fp[0];                                                                               \
    F2_ = fp[4 * 64];                                                                          \
    if (PASSES >= 6) F3_ = fp[8 * 64];                                                         \
  }
#define EZ_MFMA1(F1_, F2_, F3_, qi_, P_)                                                       \
  {                                                                                            \
    if (PASSES >= 6) {                                                                         \
      P_ = mma16<F16>(F3_, q1[qi_], P_);                                                       \
      P_ = mma16<F16>(F1_, q3[qi_], P_);                                                       \
      P_ = mma16<F16>(F2_, q2[qi_], P_);                                                       \
    }                                                                                          \
    P_ = mma16<F16>(F2_, q1[qi_], P_);                                                         \
    P_ = mma16<F16>(F1_, q2[qi_], P_);                                                         \
    P_ = mma16<F16>(F1_, q1[qi_], P_);                                                         \
  }
#define EZ_MFMA(F1_, F2_, F3_, s_, cb_)                                                        \
  {                                                                                            \
    if (ALT && ((s_) & 1)) {                                                                   \
      EZ_MFMA1(F1_, F2_, F3_, 2 * (s_) + 0, partn[2 * (cb_) + 0])                              \
      EZ_MFMA1(F1_, F2_, F3_, 2 * (s_) + 1, partn[2 * (cb_) + 1])                              \
    } else {                                                                                   \
      EZ_MFMA1(F1_, F2_, F3_, 2 * (s_) + 0, part[2 * (cb_) + 0])                               \
      EZ_MFMA1(F1_, F2_, F3_, 2 * (s_) + 1, part[2 * (cb_) + 1])                               \
    }                                                                                          \
  }
  EZ_READ(fa1, fa2, fa3, 0, 0);
  f32x4 part[8], partn[ALT ? 8 : 1];
  float dot_a = 0.f, dot_b = 0.f, omx = 0.f;
  const int ncbA = a_out ? H * cb_per_head : 0;      // column blocks that belong to the attention network
  const int cb0 = (int)((long)blockIdx.y * hb.ks0);  // column blocks in front of this column group (whole heads; 0: no groups)
  if (wA) wA += (long)cb0 * 128;
  for (int cb = 0; cb < ncb; ++cb) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int i = 0; i < 8; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (ALT) {
#pragma unroll
        for (int i = 0; i < 8; ++i) partn[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {                  // chunk (cb, half, s) sits in ring slot (4 half + s) % RING
        constexpr int SM = RING - 1;
        const int slot = (half * 4 + s) & SM;
        EZ_TLOAD((long)cb * 8 + half * 4 + s + RING - 1);
#pragma unroll
        for (int cbp = 0; cbp < 2; ++cbp) {
          EZ_READ(fb1, fb2, fb3, slot, 2 * cbp + 1);
          __builtin_amdgcn_sched_barrier(0);
          EZ_MFMA(fa1, fa2, fa3, s, 2 * cbp);
          if (cbp == 0) EZ_READ(fa1, fa2, fa3, slot, 2)
          else EZ_READ(fa1, fa2, fa3, (slot + 1) & SM, 0);
          __builtin_amdgcn_sched_barrier(0);
          EZ_MFMA(fb1, fb2, fb3, s, 2 * cbp + 1);
        }
        if constexpr (DEEP) {
          // chunk i + 2 was issued five iterations ago; younger than it: five chunks (10 loads), the eight stores
          // of the epilogue that preceded this slice and, for s == 0, also those of the slice before
          if (s == 0) wait_vmcnt<26>();
          else wait_vmcnt<18>();
        } else if constexpr (F16) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      if constexpr (ALT) {
#pragma unroll
        for (int i = 0; i < 8; ++i) part[i] -= partn[i];
      }
      if constexpr (F16) {                           // undo the row and column-block scales
        float sw, iw;
        pow2_scale(wmax[cb], sw, iw);
        const float ma = rs_a * iw, mb = rs_b * iw;
#pragma unroll
        for (int i = 0; i < 4; ++i) { part[2 * i + 0] = part[2 * i + 0] * ma; part[2 * i + 1] = part[2 * i + 1] * mb; }
      }
      // ---- epilogue of the 64-column slice: z = part + Pi[dst] + Pj[src]; store; logits ----
      const int col0 = cb * 128 + half * 64 + 4 * kg;
      const bool isA = cb + cb0 < ncbA;
      float4 hia[DEEP ? 4 : 1], hja[DEEP ? 4 : 1], hib[DEEP ? 4 : 1], hjb[DEEP ? 4 : 1];
      if constexpr (DEEP) {                          // every gather of the slice before its first store
#pragma unroll
        for (int c16 = 0; c16 < 4; ++c16) {
          hia[c16] = *reinterpret_cast<const float4*>(pia + col0 + 16 * c16);
          hja[c16] = *reinterpret_cast<const float4*>(pja + col0 + 16 * c16);
          hib[c16] = *reinterpret_cast<const float4*>(pib + col0 + 16 * c16);
          hjb[c16] = *reinterpret_cast<const float4*>(pjb + col0 + 16 * c16);
        }
        asm volatile("" ::: "memory");
      }
#pragma unroll
      for (int c16 = 0; c16 < 4; ++c16) {
        const int col = col0 + 16 * c16;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 ia = DEEP ? hia[DEEP ? c16 : 0] : ((ADDS || pia) ? *reinterpret_cast<const float4*>(pia + col) : zero4);
        const float4 ja = DEEP ? hja[DEEP ? c16 : 0] : (ADDS ? *reinterpret_cast<const float4*>(pja + col) : zero4);
        const float4 ib = DEEP ? hib[DEEP ? c16 : 0] : (ADDS ? *reinterpret_cast<const float4*>(pib + col) : ia);
        const float4 jb = DEEP ? hjb[DEEP ? c16 : 0] : (ADDS ? *reinterpret_cast<const float4*>(pjb + col) : zero4);
        const f32x4 pa = part[2 * c16 + 0], pb = part[2 * c16 + 1];
        float4 va = make_float4(pa[0] + ia.x + ja.x, pa[1] + ia.y + ja.y, pa[2] + ia.z + ja.z, pa[3] + ia.w + ja.w);
        float4 vb = make_float4(pb[0] + ib.x + jb.x, pb[1] + ib.y + jb.y, pb[2] + ib.z + jb.z, pb[3] + ib.w + jb.w);
        if (act == CGAT_ACT_LEAKY) {   // store the hidden activations instead of the pre-activations (edge_hidden op)
          va = make_float4(va.x > 0.f ? va.x : 0.01f * va.x, va.y > 0.f ? va.y : 0.01f * va.y,
                           va.z > 0.f ? va.z : 0.01f * va.z, va.w > 0.f ? va.w : 0.01f * va.w);
          vb = make_float4(vb.x > 0.f ? vb.x : 0.01f * vb.x, vb.y > 0.f ? vb.y : 0.01f * vb.y,
                           vb.z > 0.f ? vb.z : 0.01f * vb.z, vb.w > 0.f ? vb.w : 0.01f * vb.w);
        }
        if (!ADDS) {   // the dense-layer form: out = act(x W^T + b) [+ out]
          if (act == CGAT_ACT_TANH) {
            va = make_float4(tanhf(va.x), tanhf(va.y), tanhf(va.z), tanhf(va.w));
            vb = make_float4(tanhf(vb.x), tanhf(vb.y), tanhf(vb.z), tanhf(vb.w));
          }
          if (dact) {   // (kernel argument: uniform) times LeakyReLU'(0.01) at the sign of dact[row, col]: the product IS a
                        // pre-activation gradient (the per-head second layers' input gradient, vector attention)
            const float4 ha = *reinterpret_cast<const float4*>(dact + (long)rca * ld_dact + col);
            const float4 hb = *reinterpret_cast<const float4*>(dact + (long)rcb * ld_dact + col);
            va = make_float4(va.x * (ha.x > 0.f ? 1.f : 0.01f), va.y * (ha.y > 0.f ? 1.f : 0.01f),
                             va.z * (ha.z > 0.f ? 1.f : 0.01f), va.w * (ha.w > 0.f ? 1.f : 0.01f));
            vb = make_float4(vb.x * (hb.x > 0.f ? 1.f : 0.01f), vb.y * (hb.y > 0.f ? 1.f : 0.01f),
                             vb.z * (hb.z > 0.f ? 1.f : 0.01f), vb.w * (hb.w > 0.f ? 1.f : 0.01f));
          }
          if (accumulate) {
            if (row_a < E) { const float4 u = *reinterpret_cast<const float4*>(za + col); va.x += u.x; va.y += u.y; va.z += u.z; va.w += u.w; }
            if (row_b < E) { const float4 u = *reinterpret_cast<const float4*>(zb + col); vb.x += u.x; vb.y += u.y; vb.z += u.z; vb.w += u.w; }
          }
        }
        // DEEP: unconditional (the allowances count eight stores; clamped rows rewrite identical values)
        if constexpr (ZB) {
          if (row_a < E) store4_bf16(reinterpret_cast<__bf16*>(Z) + (long)rca * ldz + col, va);
          if (row_b < E) store4_bf16(reinterpret_cast<__bf16*>(Z) + (long)rcb * ldz + col, vb);
        } else {
          if (DEEP || row_a < E) *reinterpret_cast<float4*>(za + col) = va;
          if (DEEP || row_b < E) *reinterpret_cast<float4*>(zb + col) = vb;
        }
        if (omax) {   // (kernel argument: uniform) max |stored value|: the per-tensor fp16 scale of the kernels that read it
          omx = fmaxf(fmaxf(omx, fmaxf(fabsf(va.x), fabsf(va.y))), fmaxf(fabsf(va.z), fabsf(va.w)));
          omx = fmaxf(fmaxf(omx, fmaxf(fabsf(vb.x), fabsf(vb.y))), fmaxf(fabsf(vb.z), fabsf(vb.w)));
        }
        if (isA) {
          const float4 w = *reinterpret_cast<const float4*>(wA + col);
          dot_a += (va.x > 0.f ? va.x : 0.01f * va.x) * w.x + (va.y > 0.f ? va.y : 0.01f * va.y) * w.y +
                   (va.z > 0.f ? va.z : 0.01f * va.z) * w.z + (va.w > 0.f ? va.w : 0.01f * va.w) * w.w;
          asm volatile("" : "+v"(dot_a));   // keep the two accumulations apart: see the note on packed math above
          dot_b += (vb.x > 0.f ? vb.x : 0.01f * vb.x) * w.x + (vb.y > 0.f ? vb.y : 0.01f * vb.y) * w.y +
                   (vb.z > 0.f ? vb.z : 0.01f * vb.z) * w.z + (vb.w > 0.f ? vb.w : 0.01f * vb.w) * w.w;
          asm volatile("" : "+v"(dot_b));
        }
      }
      if (isA && half == 1 && (cb + 1) % cb_per_head == 0) {   // a head is complete: reduce over the 4 lane groups
        const int h = (cb + cb0) / cb_per_head;
        float da = dot_a, db = dot_b;
        da += __shfl_xor(da, 16, 64); da += __shfl_xor(da, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        if (kg == 0) {
          const float bh = bA ? bA[h] : 0.f;
          if (row_a < E) a_out[(long)row_a * H + h] = da + bh;
          if (row_b < E) a_out[(long)row_b * H + h] = db + bh;
        }
        dot_a = 0.f; dot_b = 0.f;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef EZ_TLOAD
#undef EZ_READ
#undef EZ_MFMA1
#undef EZ_MFMA
  if (omax) block_absmax_commit(omx, omax);
}

// ---------------------------------------------------------------------------------------
// The six-pass per-edge launch on 256-row workgroups (round 5): the SAME arithmetic as edge_z_kernel<6, true> -- three bf16
// planes per operand, the six products in the same order, even / odd k-steps into the two accumulator sets, the same
// epilogue order: bit-identical Z and logits -- with what made the f16x3c per-edge form of round 5 faster (DESIGN.md
// section 10; that form is in the history at 43b4fa4) although the matrix work was never its bound:
//  * 256-row workgroups: half the weight traffic through the ring per row;
//  * every chunk is a finished 32-column slice of the output, so the gathered addends of the NEXT chunk (8 x 16 bytes per
//    lane) are requested a whole chunk of matrix work before their use, into registers the 32-column granularity frees;
//  * counted waits that never wait for a store: per chunk a wave issues, in this order, 3 LDS-DMA pieces for chunk i + 3,
//    the 8 gathers of chunk i + 1, and -- after the matrix work -- the 4 stores of chunk i.  The gathers of chunk i are
//    needed after the matrix work of chunk i: younger than them are the 4 stores of chunk i - 1 and this iteration's
//    3 + 8 loads, so the wait is vmcnt(4 + 3 + 8) = 15 -- it also covers the ring (chunk i + 2's pieces are older still)
//    and leaves every store two chunks of matrix work to drain.  Rows are clamped (below) so that every wave issues
//    exactly these operations.
// edge_z_kernel<6, true> alternates two 128-row workgroups per CU and waits vmcnt(3) per k-step: every wait behind an
// epilogue drains that epilogue's stores (in-order vmcnt) and its gathers are requested where they are used: 3.2 ms at the
// BASELINE shape with 1.9 ms of matrix work and 0.66 of wave cycles waiting on memory.
// Operand: prepare_T_bf16's image as it is (12-KB k-step chunks (a, half, s) = [plane][cb][lane] x 16 B); a ring chunk
// here is (a, half, pair of 16-column blocks) = 24 one-KB pieces [s][plane][cb2] picked out of four of those, three per
// wave.  LDS: 4 slots x 24 KB + fc_out_A's weight.
//
// One 256-row tile of it is z6w_tile below, in three forms (MODE):
//   0  Z stored, logits of the attention blocks (edge_z6w_kernel: the training forward);
//   1  logits only, over the attention column blocks, nothing stored but a [E, H] (the forward without grad);
//   2  the message column blocks: each 32-column slice of z = part + Pi[dst] + Pj[src] is staged in LDS (rounded to bf16
//      first under bf16 edge storage, as mode 0 stores it), and red(a, ch) reduces it into the weighted segment sums
//      (edge_msg_wsum_kernel).  Nothing per edge reaches memory.
//   3  the bit form of the training forward: as mode 0, but an attention chunk stores no Z -- a chunk
//      is one 32-column word of the sign mask (bit i of word w = Z[t, 32 w + i] > 0, seg_bwd_att_kernel's meaning); the words
//      of rows 32 g .. 32 g + 31 go to zbits + g * ldz, word-major [word][row & 31]: one 128-byte line per wave and chunk.
//      Logits by the same statements; the message chunks are mode 0's.
// The logits of head h (of the H heads this tile computes) go to a_out[row * lda + h].
// Rows >= row_lim are clamped to row_lim - 1 (their results are discarded).  The counted wait below allows for the
// stores of mode 0 only; modes 1 and 2 wait for the gathers of the current slice with 4 fewer younger operations (in
// mode 2 the weighted sums' stores of the previous slice are older still: waited for too, never overtaken).  In mode 3 an
// attention chunk issues ONE store (every wave: a wave of clamped rows rewrites row E - 1's word with the identical value),
// so behind an attention chunk the wait counts 1 + 3 + 8 = 12 younger operations, behind a message chunk mode 0's 15: the
// count never includes an operation that was not issued (the logits' stores, where a head ends, only make it wait longer).
// ---------------------------------------------------------------------------------------
constexpr int Z6_CH = 24 * 64;                        // 16-byte pieces per ring chunk (24 KB)
constexpr int Z6_SLOTS = 4;
struct Z6NoRed {
  __device__ void operator()(int, int) const {}
};
template <int MODE, bool ZB, class Red>
__device__ __forceinline__ void z6w_tile(uint4* smem, float* zst, const float* e, long lde,
                                         const int* perm, const uint4* Wq, int ncb,
                                         const float* Pi, const int* dsti,
                                         const float* Pj, const int* srci, long ld_add,
                                         float* Z, long ldz, int row0, int row_lim,
                                         const float* wA, const float* bA, int H,
                                         int cb_per_head, float* a_out, int lda, int act, float* omax,
                                         const Red& red, unsigned* zbits = nullptr) {
  constexpr int CH = Z6_CH;
  constexpr int SLOTS = Z6_SLOTS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int n16 = lane & 15, kg = lane >> 4;
  const int row_w = (unsigned)row0 + wave * 32;
  const int row_a = row_w + n16, row_b = row_w + 16 + n16;
  const int rca = row_a < row_lim ? row_a : row_lim - 1, rcb = row_b < row_lim ? row_b : row_lim - 1;
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + lane;
  const unsigned l_off = (unsigned)lane * 16;
  const long last_chunk = (long)ncb * 4 - 1;
  // this wave's three pieces pc = 3 wave + i of a chunk: (s, plane, cb2) = (pc / 6, (pc % 6) / 2, pc % 2); source offset
  // inside the (a, half) group of four k-step chunks in 16-byte units, destination offset inside the slot in bytes
  int psrc[3];
  unsigned pdst[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int pc = 3 * wave_u + i, s4 = pc / 6, pl = (pc % 6) >> 1, c2 = pc & 1;
    psrc[i] = s4 * 768 + pl * 256 + c2 * 64;
    pdst[i] = __builtin_amdgcn_readfirstlane(sbase + (unsigned)pc * 1024);
  }

  // the lane's two edge rows, split once: q[plane][2 s + nb] holds e[row(nb), 32 s + 8 kg + 0..7]; odd k-steps negated
  bf16x8 q1[8], q2[8], q3[8];
  {
    const long ea = perm ? perm[rca] : rca, eb = perm ? perm[rcb] : rcb;
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float4* qp = reinterpret_cast<const float4*>(e + (nb ? eb : ea) * lde + 32 * s4 + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        const float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        split3_x8(v, q1[2 * s4 + nb], q2[2 * s4 + nb], q3[2 * s4 + nb]);
        if (s4 & 1) {
          q1[2 * s4 + nb] = neg_x8(q1[2 * s4 + nb]);
          q2[2 * s4 + nb] = neg_x8(q2[2 * s4 + nb]);
          q3[2 * s4 + nb] = neg_x8(q3[2 * s4 + nb]);
        }
      }
  }
  // gathered rows as 32-bit byte offsets from Pi / Pj (< 4 GB: checked by the launcher)
  const unsigned oia = (unsigned)(((long)dsti[rca] * ld_add + 4 * kg) * 4), oib = (unsigned)(((long)dsti[rcb] * ld_add + 4 * kg) * 4);
  const unsigned oja = (unsigned)(((long)srci[rca] * ld_add + 4 * kg) * 4), ojb = (unsigned)(((long)srci[rcb] * ld_add + 4 * kg) * 4);
  const int ncbA = (a_out && wA) ? H * cb_per_head : 0;      // column blocks that belong to the attention network
  float* wAs = reinterpret_cast<float*>(smem + SLOTS * CH);
  for (int i = tid; i < ncbA * 128; i += 512) wAs[i] = wA[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // chunk gi = 4 a + ch, ch = 2 half + pair: its 24 pieces live at Wq + ((2 a + half) * 4) * 768 + pair * 128 + psrc
#define Z6_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const uint4* tb = Wq + (gi >> 1) * (4 * 768) + (gi & 1) * 128;                             \
    const unsigned so = (unsigned)((gi_) & 3) * (CH * 16);                                     \
    glds_b128(tb + psrc[0], l_off, pdst[0] + so);                                              \
    glds_b128(tb + psrc[1], l_off, pdst[1] + so);                                              \
    glds_b128(tb + psrc[2], l_off, pdst[2] + so);                                              \
  }
#define Z6_GATHER(G_, gi_)                                                                     \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const unsigned cbyte = (unsigned)(((gi >> 2) * 128 + ((gi >> 1) & 1) * 64 + (gi & 1) * 32) * 4); \
    _Pragma("unroll") for (int cb2 = 0; cb2 < 2; ++cb2) {                                      \
      asm volatile("global_load_dwordx4 %0, %4, %8\n\tglobal_load_dwordx4 %1, %5, %9\n\t"      \
                   "global_load_dwordx4 %2, %6, %8\n\tglobal_load_dwordx4 %3, %7, %9"          \
                   : "=&v"(G_[4 * cb2 + 0]), "=&v"(G_[4 * cb2 + 1]), "=&v"(G_[4 * cb2 + 2]), "=&v"(G_[4 * cb2 + 3]) \
                   : "v"(oia + cbyte + 64 * cb2), "v"(oja + cbyte + 64 * cb2), "v"(oib + cbyte + 64 * cb2),  \
                     "v"(ojb + cbyte + 64 * cb2), "s"(Pi), "s"(Pj)                             \
                   : "memory");                                                                \
    }                                                                                          \
  }
  f32x4 GA[8], GB[8];
  Z6_TLOAD(0l);
  Z6_TLOAD(1l);
  Z6_TLOAD(2l);
  Z6_GATHER(GA, 0l);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fa3, fb1, fb2, fb3;
  // group g = 2 s + cb2: the three planes of 16-column block cb2 at k-step s
#define Z6_READ(F1_, F2_, F3_, slot_, g_)                                                      \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * CH + (((g_) >> 1) * 6 + ((g_) & 1)) * 64;              \
    F1_ = fp[0];                                                                               \
    F2_ = fp[2 * 64];                                                                          \
    F3_ = fp[4 * 64];                                                                          \
  }
  // even k-steps into part, odd ones (negated row fragments) into partn; the six products in edge_z_kernel's order
#define Z6_MFMA(F1_, F2_, F3_, g_)                                                             \
  {                                                                                            \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                         \
      f32x4& P_ = (((g_) >> 1) & 1) ? partn[2 * ((g_) & 1) + nb] : part[2 * ((g_) & 1) + nb];  \
      const int qi_ = 2 * ((g_) >> 1) + nb;                                                    \
      P_ = mma16<false>(F3_, q1[qi_], P_);                                                     \
      P_ = mma16<false>(F1_, q3[qi_], P_);                                                     \
      P_ = mma16<false>(F2_, q2[qi_], P_);                                                     \
      P_ = mma16<false>(F2_, q1[qi_], P_);                                                     \
      P_ = mma16<false>(F1_, q2[qi_], P_);                                                     \
      P_ = mma16<false>(F1_, q1[qi_], P_);                                                     \
    }                                                                                          \
  }
  // epilogue of chunk (a_, ch_): z = (part - partn) + gathered addends; store; logits
#define Z6_EPILOGUE(G_, a_, ch_)                                                               \
  {                                                                                            \
    asm volatile("" : "+v"(G_[0]), "+v"(G_[1]), "+v"(G_[2]), "+v"(G_[3]), "+v"(G_[4]), "+v"(G_[5]), "+v"(G_[6]), "+v"(G_[7])); \
    int ra_ = rca, rb_ = rcb, lk_ = lane;   /* laundered: the 64-bit row addresses are formed HERE, not kept (a scratch \
                                              reload in this loop waits vmcnt(0), i.e. for every store) */                \
    asm volatile("" : "+v"(ra_), "+v"(rb_), "+v"(lk_));                                        \
    const int col0 = (a_) * 128 + ((ch_) >> 1) * 64 + ((ch_) & 1) * 32 + 4 * (lk_ >> 4);       \
    const bool isA = (a_) < ncbA;                                                              \
    unsigned wa_ = 0u, wb_ = 0u;                                                               \
    _Pragma("unroll") for (int cb2 = 0; cb2 < 2; ++cb2) {                                      \
      const int col = col0 + 16 * cb2;                                                         \
      const f32x4 pa = part[2 * cb2 + 0] - partn[2 * cb2 + 0], pb = part[2 * cb2 + 1] - partn[2 * cb2 + 1]; \
      const f32x4 ia = G_[4 * cb2 + 0], ja = G_[4 * cb2 + 1], ib = G_[4 * cb2 + 2], jb = G_[4 * cb2 + 3]; \
      float4 va = make_float4(pa[0] + ia[0] + ja[0], pa[1] + ia[1] + ja[1], pa[2] + ia[2] + ja[2], pa[3] + ia[3] + ja[3]); \
      float4 vb = make_float4(pb[0] + ib[0] + jb[0], pb[1] + ib[1] + jb[1], pb[2] + ib[2] + jb[2], pb[3] + ib[3] + jb[3]); \
      if (act == CGAT_ACT_LEAKY) {   /* (kernel argument: uniform) the hidden activations instead of the pre-activations */ \
        va = make_float4(va.x > 0.f ? va.x : 0.01f * va.x, va.y > 0.f ? va.y : 0.01f * va.y,   \
                         va.z > 0.f ? va.z : 0.01f * va.z, va.w > 0.f ? va.w : 0.01f * va.w);  \
        vb = make_float4(vb.x > 0.f ? vb.x : 0.01f * vb.x, vb.y > 0.f ? vb.y : 0.01f * vb.y,   \
                         vb.z > 0.f ? vb.z : 0.01f * vb.z, vb.w > 0.f ? vb.w : 0.01f * vb.w);  \
      }                                                                                        \
      if constexpr (MODE == 2) {   /* the slice in LDS: [256 rows][32 columns], LeakyReLU applied */ \
        float4 sa = va, sb = vb;                                                               \
        if constexpr (ZB) { sa = unpack4_bf16(pack4_bf16(va)); sb = unpack4_bf16(pack4_bf16(vb)); } \
        sa = make_float4(sa.x > 0.f ? sa.x : 0.01f * sa.x, sa.y > 0.f ? sa.y : 0.01f * sa.y,   \
                         sa.z > 0.f ? sa.z : 0.01f * sa.z, sa.w > 0.f ? sa.w : 0.01f * sa.w);  \
        sb = make_float4(sb.x > 0.f ? sb.x : 0.01f * sb.x, sb.y > 0.f ? sb.y : 0.01f * sb.y,   \
                         sb.z > 0.f ? sb.z : 0.01f * sb.z, sb.w > 0.f ? sb.w : 0.01f * sb.w);  \
        const int cl_ = 16 * cb2 + 4 * (lk_ >> 4);                                             \
        *reinterpret_cast<float4*>(zst + (wave_u * 32 + n16) * 32 + cl_) = sa;                 \
        *reinterpret_cast<float4*>(zst + (wave_u * 32 + 16 + n16) * 32 + cl_) = sb;            \
      } else if constexpr (MODE == 0) {                                                        \
        if constexpr (ZB) {                                                                    \
          store4_bf16(reinterpret_cast<__bf16*>(Z) + (long)ra_ * ldz + col, va);               \
          store4_bf16(reinterpret_cast<__bf16*>(Z) + (long)rb_ * ldz + col, vb);               \
        } else {                                                                               \
          *reinterpret_cast<float4*>(Z + (long)ra_ * ldz + col) = va;                          \
          *reinterpret_cast<float4*>(Z + (long)rb_ * ldz + col) = vb;                          \
        }                                                                                      \
      }                                                                                        \
      if constexpr (MODE == 3) {                                                               \
        if (isA) {   /* four sign bits of each row at the columns' place in the chunk's word */ \
          const int sh_ = 16 * cb2 + 4 * (lk_ >> 4);                                           \
          wa_ |= ((va.x > 0.f ? 1u : 0u) | (va.y > 0.f ? 2u : 0u) | (va.z > 0.f ? 4u : 0u) | (va.w > 0.f ? 8u : 0u)) << sh_; \
          wb_ |= ((vb.x > 0.f ? 1u : 0u) | (vb.y > 0.f ? 2u : 0u) | (vb.z > 0.f ? 4u : 0u) | (vb.w > 0.f ? 8u : 0u)) << sh_; \
        } else {                                                                               \
          *reinterpret_cast<float4*>(Z + (long)ra_ * ldz + col) = va;                          \
          *reinterpret_cast<float4*>(Z + (long)rb_ * ldz + col) = vb;                          \
        }                                                                                      \
      }                                                                                        \
      if (MODE == 0 && omax) {   /* (kernel argument: uniform) max |stored value|; dot_b is free in a launch without logits */ \
        dot_b = fmaxf(fmaxf(dot_b, fmaxf(fabsf(va.x), fabsf(va.y))), fmaxf(fabsf(va.z), fabsf(va.w))); \
        dot_b = fmaxf(fmaxf(dot_b, fmaxf(fabsf(vb.x), fabsf(vb.y))), fmaxf(fabsf(vb.z), fabsf(vb.w))); \
      }                                                                                        \
      if (isA) {                                                                               \
        const float4 w = *reinterpret_cast<const float4*>(wAs + col);                          \
        dot_a += (va.x > 0.f ? va.x : 0.01f * va.x) * w.x + (va.y > 0.f ? va.y : 0.01f * va.y) * w.y + \
                 (va.z > 0.f ? va.z : 0.01f * va.z) * w.z + (va.w > 0.f ? va.w : 0.01f * va.w) * w.w; \
        asm volatile("" : "+v"(dot_a));   /* keep the two accumulations apart: see the note on packed math above */ \
        dot_b += (vb.x > 0.f ? vb.x : 0.01f * vb.x) * w.x + (vb.y > 0.f ? vb.y : 0.01f * vb.y) * w.y + \
                 (vb.z > 0.f ? vb.z : 0.01f * vb.z) * w.z + (vb.w > 0.f ? vb.w : 0.01f * vb.w) * w.w; \
        asm volatile("" : "+v"(dot_b));                                                        \
      }                                                                                        \
    }                                                                                          \
    if constexpr (MODE == 3) if (isA) {                                                        \
      /* OR over the four lane groups in two exchanges: even groups end with row a's word, odd groups with row b's; \
         groups 0 and 1 store them -- lanes 0..31 = rows 0..31 of the wave */                  \
      const bool odd_ = (lk_ >> 4) & 1;                                                        \
      unsigned keep_ = (odd_ ? wb_ : wa_) | (unsigned)__shfl_xor((int)(odd_ ? wa_ : wb_), 16, 64); \
      keep_ |= (unsigned)__shfl_xor((int)keep_, 32, 64);                                       \
      if (lk_ < 32) {                                                                          \
        const int rs_ = odd_ ? rb_ : ra_;                                                      \
        zbits[(long)(rs_ >> 5) * ldz + ((a_) * 4 + (ch_)) * 32 + (rs_ & 31)] = keep_;          \
      }                                                                                        \
    }                                                                                          \
    if (isA && (ch_) == 3 && ((a_) + 1) % cb_per_head == 0) {   /* a head is complete: reduce over the 4 lane groups */ \
      const int h = (a_) / cb_per_head;                                                        \
      float da = dot_a, db = dot_b;                                                            \
      da += __shfl_xor(da, 16, 64); da += __shfl_xor(da, 32, 64);                              \
      db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);                              \
      if ((lk_ >> 4) == 0) {   /* (clamped rows rewrite row E - 1's logits with identical values) */ \
        const float bh = bA ? bA[h] : 0.f;                                                     \
        a_out[(long)ra_ * lda + h] = da + bh;                                                  \
        a_out[(long)rb_ * lda + h] = db + bh;                                                  \
      }                                                                                        \
      dot_a = 0.f; dot_b = 0.f;                                                                \
    }                                                                                          \
  }
  // one chunk: ring prefetch, the next chunk's gathers, 8 groups of 12 matrix instructions (every fragment read one
  // group ahead), the counted wait, the epilogue, the barrier
#define Z6_CHUNK(a_, ch_, GCUR_, GNEXT_)                                                       \
  {                                                                                            \
    constexpr int sl_ = (ch_), sn_ = ((ch_) + 1) & 3;   /* ring slot = chunk index mod 4 = ch_ */ \
    Z6_TLOAD((long)(a_) * 4 + (ch_) + 3);                                                      \
    Z6_GATHER(GNEXT_, (long)(a_) * 4 + (ch_) + 1);                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) { part[i] = f32x4{0.f, 0.f, 0.f, 0.f}; partn[i] = f32x4{0.f, 0.f, 0.f, 0.f}; } \
    _Pragma("unroll") for (int gp = 0; gp < 4; ++gp) {                                         \
      Z6_READ(fb1, fb2, fb3, sl_, 2 * gp + 1);                                                 \
      __builtin_amdgcn_sched_barrier(0);                                                       \
      Z6_MFMA(fa1, fa2, fa3, 2 * gp);                                                          \
      if (gp < 3) Z6_READ(fa1, fa2, fa3, sl_, 2 * gp + 2)                                      \
      else Z6_READ(fa1, fa2, fa3, sn_, 0);                                                     \
      __builtin_amdgcn_sched_barrier(0);                                                       \
      Z6_MFMA(fb1, fb2, fb3, 2 * gp + 1);                                                      \
    }                                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    /* gathers of THIS chunk (issued one iteration ago): younger are the 4 stores of the previous chunk and this       \
       iteration's 3 pieces + 8 gathers; the ring needs nothing more (chunk i + 2's pieces are older still) */          \
    if constexpr (MODE == 3) {   /* (uniform) was the previous chunk an attention chunk: one store, or four */ \
      if ((a_) * 4 + (ch_) <= 4 * ncbA) wait_vmcnt<12>();                                      \
      else wait_vmcnt<15>();                                                                   \
    } else                                                                                     \
    wait_vmcnt<MODE == 0 ? 15 : 11>();                                                         \
    if constexpr (MODE == 2) {   /* every wave is done reducing the previous slice */          \
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                       \
      __builtin_amdgcn_s_barrier();                                                            \
    }                                                                                          \
    Z6_EPILOGUE(GCUR_, a_, ch_)                                                                \
    __builtin_amdgcn_sched_barrier(0);                                                         \
    if constexpr (MODE == 2) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                \
    __builtin_amdgcn_s_barrier();                                                              \
    asm volatile("" ::: "memory");                                                             \
    if constexpr (MODE == 2) red(a_, ch_);                                                     \
  }
  Z6_READ(fa1, fa2, fa3, 0, 0);
  f32x4 part[4], partn[4];
  float dot_a = 0.f, dot_b = 0.f;
  for (int a = 0; a < ncb; ++a) {
    Z6_CHUNK(a, 0, GA, GB)
    Z6_CHUNK(a, 1, GB, GA)
    Z6_CHUNK(a, 2, GA, GB)
    Z6_CHUNK(a, 3, GB, GA)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if constexpr (MODE == 0) if (omax) block_absmax_commit(dot_b, omax);
#undef Z6_TLOAD
#undef Z6_GATHER
#undef Z6_READ
#undef Z6_MFMA
#undef Z6_EPILOGUE
#undef Z6_CHUNK
}

// MODE 0 (the training forward), MODE 3 (its bit form: zbits = the first sign-bit hole) and MODE 1 (logits only: Z, ZB,
// act and omax unused).
// In MODE 1 the heads are dealt to grid.y groups (few row tiles): group y computes heads [y H / gy, (y + 1) H / gy) from
// its ncb = (H / gy) * cb_per_head column blocks; each head's logit is the sum over its own blocks, as in one group.
template <bool ZB, int MODE = 0>
__global__ __launch_bounds__(512, 2) void edge_z6w_kernel(const float* __restrict__ e, long lde, const int* __restrict__ perm,
                                                          const uint4* __restrict__ Wq, int ncb,
                                                          const float* __restrict__ Pi, const int* __restrict__ dsti,
                                                          const float* __restrict__ Pj, const int* __restrict__ srci,
                                                          long ld_add, float* __restrict__ Z, long ldz, int E,
                                                          const float* __restrict__ wA, const float* __restrict__ bA,
                                                          int H, int cb_per_head, float* __restrict__ a_out, int act,
                                                          float* __restrict__ omax, unsigned* __restrict__ zbits) {
  __shared__ uint4 smem[Z6_SLOTS * Z6_CH + 512];      // the ring + fc_out_A's weight (<= 2048 floats)
  if constexpr (MODE == 1) {
    const int hg = H / (int)gridDim.y, h0 = (int)blockIdx.y * hg;
    const long c0 = (long)blockIdx.y * ncb * 128;     // the group's first column
    z6w_tile<1, ZB>(smem, nullptr, e, lde, perm, Wq + c0 / 128 * 6144, ncb, Pi + c0, dsti, Pj + c0, srci, ld_add, Z, ldz,
                    blockIdx.x * 256, E, wA + c0, bA ? bA + h0 : nullptr, hg, cb_per_head, a_out + h0, H, act, omax,
                    Z6NoRed{});
  } else {
    z6w_tile<MODE, ZB>(smem, nullptr, e, lde, perm, Wq, ncb, Pi, dsti, Pj, srci, ld_add, Z, ldz, blockIdx.x * 256, E, wA, bA,
                       H, cb_per_head, a_out, H, act, omax, Z6NoRed{}, zbits);
  }
}

// ---------------------------------------------------------------------------------------
// The message half of the forward without grad (reference CGAT.py:319-329 under torch.no_grad(): predict.py, the
// embeddings of calculate_embeddings.py): with the coefficients alpha [E, H] already formed by seg_softmax_fwd from the
// logits launch above,
//     S[n, c] = sum_{t in seg(n)} leaky(z[t, c]) * alpha[t, c / Hd],   z = the message columns of Z,
// summed in EXACTLY the order of seg_wsum_vec_kernel / seg_wsum_long_kernel (segment.hip), so S -- and everything after
// it -- is bit-identical to the training forward's, without Z ever reaching memory.
//   * Workgroup w owns the destination segments [lb(w R), lb((w + 1) R)), lb(v) = the first segment starting at row >= v
//     (binary search in dst_rowptr), and with them a contiguous row range that starts and ends at segment boundaries.
//     R < 256 (host: 256 minus the mean in-degree rounded up to 16) keeps a range within one 256-row sub-tile for
//     ordinary segments; a longer range is walked in 256-row sub-tiles.  No segment is split between workgroups,
//     workgroups never wait on each other.
//   * Per 32-column slice the tile stages leaky(z) of its 256 rows in LDS (32 KB); 16 x 32 reducer threads (segment
//     part, column) then run the chain acc = fma(leaky(z), alpha, acc) over the part's rows in ascending order, as
//     seg_wsum_vec_kernel does (its update contracts to v_fma_f32).  A segment of more than SEG_LONG rows keeps
//     seg_wsum_long_kernel's G strided row groups (G = 1024 / min(HHd / 4, 256)) and adds them in group order at its end.
//   * Only the part that continues past a sub-tile carries its partial sums (G x the workgroup's columns, LDS) to the
//     next one; it is the last part of one sub-tile and the first of the next, and the thread that finishes one
//     sub-tile's first part also runs its last part -- in that order -- so the carry is read before it is overwritten.
//   * Segments without rows get S = 0 (seg_wsum_vec_kernel writes its zero accumulator for them).
//   * The message column blocks are dealt to grid.y groups: group y owns the ncb blocks from column y * ncb * 128 on,
//     over the same row range as every other group (each column's chain is the same whatever group runs it).  The
//     launcher takes enough groups that the carry, Glong x ncb * 128 floats, fits WSUM_CARRY -- two at H * Hd = 1280 or
//     2048, where Glong = 4 -- and, below 128 row tiles of 256, as many as fill the chip (z_col_groups).  What a group
//     repeats is the edge rows' split (512 bytes a row against 2 x 4 x ncb x 128 gathered) and the part bookkeeping.
// ---------------------------------------------------------------------------------------
constexpr int WSUM_CARRY = 4096;   // floats: Glong * ncb * 128 <= 4096 (the launcher's column groups)
template <bool ZB>
__global__ __launch_bounds__(512, 2) void edge_msg_wsum_kernel(const float* __restrict__ e, long lde,
                                                               const int* __restrict__ perm, const uint4* __restrict__ Wq,
                                                               int ncb, const float* __restrict__ Pi,
                                                               const int* __restrict__ dsti, const float* __restrict__ Pj,
                                                               const int* __restrict__ srci, long ld_add, int H, int Hd,
                                                               const float* __restrict__ alpha,
                                                               const int* __restrict__ rowptr, int N, int R,
                                                               float* __restrict__ S) {
  __shared__ uint4 smem[Z6_SLOTS * Z6_CH];            // the ring (96 KB)
  __shared__ float zst[256 * 32];                     // one staged 32-column slice (32 KB)
  __shared__ float carry[WSUM_CARRY];                 // partial sums of the part continuing past the sub-tile (16 KB)
  __shared__ float alst[256 * 8];                     // alpha of the sub-tile's rows (H <= 8)
  __shared__ int plo[256], pseg[256], pr0[256], pr1[256];   // the sub-tile's segment parts: first local row, segment, rows
  __shared__ int sh[12];
  const int tid = threadIdx.x;
  const int HHd = H * Hd, HHg = ncb * 128, cg0 = (int)blockIdx.y * HHg;   // all columns; this group's: [cg0, cg0 + HHg)
  const int quads = HHd / 4, tpr = quads < 256 ? quads : 256, Glong = 1024 / tpr;   // seg_wsum_long_kernel's row groups
  if (tid == 0) {
    auto lb = [&](long v) {   // first s in [0, N] with rowptr[s] >= v
      int lo = 0, hi = N;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rowptr[mid] >= v) hi = mid; else lo = mid + 1;
      }
      return lo;
    };
    const int s0 = lb((long)blockIdx.x * R);
    const int s1 = blockIdx.x + 1 == gridDim.x ? N : lb((long)(blockIdx.x + 1) * R);
    sh[0] = s0; sh[1] = s1; sh[2] = rowptr[s0]; sh[3] = rowptr[s1];
  }
  __syncthreads();
  const int s_begin = sh[0], s_end = sh[1], R0 = sh[2], R1 = sh[3];
  // segments without rows
  for (long i = tid; i < (long)(s_end - s_begin) * (HHg / 4); i += 512) {
    const int s = s_begin + (int)(i / (HHg / 4)), q = (int)(i % (HHg / 4));
    if (rowptr[s] == rowptr[s + 1])
      *reinterpret_cast<float4*>(S + (long)s * HHd + cg0 + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int c = tid & 31, slot = tid >> 5;
  for (int t0 = R0; t0 < R1; t0 += 256) {
    const int t1 = t0 + 256 < R1 ? t0 + 256 : R1;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                     // the previous sub-tile's reductions are done
    // parts: a row starts one where its segment differs from the previous row's (or at the sub-tile's first row)
    const int r = t0 + tid;
    const int sg = tid < 256 && r < t1 ? dsti[r] : -1;
    const bool start = sg >= 0 && (tid == 0 || dsti[r - 1] != sg);
    const unsigned long long bal = __ballot(start);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) sh[4 + w] = __popcll(bal);
    for (int i = tid; i < (t1 - t0) * H; i += 512) alst[i] = alpha[(long)t0 * H + i];
    __syncthreads();
    if (start) {
      int idx = __popcll(bal & ((1ull << lane) - 1));
      for (int k = 0; k < w; ++k) idx += sh[4 + k];
      plo[idx] = tid; pseg[idx] = sg; pr0[idx] = rowptr[sg]; pr1[idx] = rowptr[sg + 1];
    }
    const int nparts = sh[4] + sh[5] + sh[6] + sh[7];
    __syncthreads();
    __syncthreads();
    // one part of one segment for column col of the slice (a, ch) (cl: the group's own): rows of group g are r0 + g + k G
    auto part = [&](int i, int a, int ch) {
      const int cl = a * 128 + (ch >> 1) * 64 + (ch & 1) * 32 + c, col = cg0 + cl, h = col / Hd;
      const int r0 = pr0[i], r1 = pr1[i], lo = t0 + plo[i], hi = i + 1 < nparts ? t0 + plo[i + 1] : t1;
      const int G = r1 - r0 > SEG_LONG ? Glong : 1;
      const bool cin = r0 < t0, cout = r1 > t1;
      float tot = 0.f;
      for (int g = 0; g < G; ++g) {
        float acc = cin ? carry[g * HHg + cl] : 0.f;
        int r = lo + (((g - (lo - r0)) % G) + G) % G;
        for (; r < hi; r += G) acc = __builtin_fmaf(zst[(r - t0) * 32 + c], alst[(r - t0) * H + h], acc);
        if (cout) carry[g * HHg + cl] = acc;
        else tot = g == 0 ? acc : tot + acc;
      }
      if (!cout) S[(long)pseg[i] * HHd + col] = tot;
    };
    // slot 0 runs part 0 (the one that may continue a carry) first and the last part (the one that may leave one) last
    auto red = [&](int a, int ch) {
      for (int i = slot; i < nparts - 1; i += 16) part(i, a, ch);
      if (slot == 0) part(nparts - 1, a, ch);
    };
    z6w_tile<2, ZB>(smem, zst, e, lde, perm, Wq + (long)blockIdx.y * ncb * 6144, ncb, Pi + cg0, dsti, Pj + cg0, srci,
                    ld_add, nullptr, 0, t0, t1, nullptr, nullptr, H, Hd / 128, nullptr, H, CGAT_ACT_NONE, nullptr, red);
  }
}

// ---------------------------------------------------------------------------------------
// The per-edge launch with the x_j projection folded in (f16x3 arithmetic):
//     Z[t, :] = [W_e | W_j] [e[perm[t]] ; x[src[t]]] + Pi[dst[t], :]
// Why, and what bounds these kernels: timing-only ablations (tools/edgez_ablation.sh; E = 1 000 080)
//                                   edge_z (K = 128, Pi and Pj gathered)     this kernel (K = 256, Pi gathered)
//     as is                                      3.15 ms                     3.2 -> 2.76 ms (see below)
//     without the Z stores                       (-17 %)                     2.1 -> 1.92
//     without the epilogue's loads               (-55 %)                     2.7 -> 2.27
//     MFMA + LDS-ring skeleton only              ~0.95                       1.7
// Neither form hid its epilogue behind the other workgroup of the CU; pointing the old kernel's Pj gather at cached
// rows (3.0 ms) or sharing the weight stream between 256 rows (3.6 ms) changed nothing.  The reason is the in-order
// vmcnt: stores count in it, so the first ring wait after an epilogue that needs a load issued AFTER the stores
// drains them, and inside the epilogue every load issued after a store does the same.  Two changes took this kernel
// from 3.2 to 2.76 ms: an 8-slot ring (the first load younger than the stores is needed five k-steps later instead of
// two; waits of vmcnt(18)/(10), derivation at the wait) and all Pi loads of a slice issued before its first store.
// Folding the x_j projection into the product (K = 256) is what makes room for that: it removes the Pj gather (6 KB
// per edge, a third of the epilogue's requests, 16 VGPRs of addresses) at the price of matrix work the kernel has
// room for, and the per-node projection Pj = x W_j^T is no longer computed.  Still exposed: ~0.85 ms of store
// latency (five k-steps = 1.3 us is not enough under load) and the Pi loads' L2 latency (0.2 ms); a ring on a
// producer wave, whose vmcnt never sees a store, is the next step.
// Operand: prepare_W2_f16 planes, chunk (a, half, s) = 8 KB at Wq + ((a*2 + half)*8 + s) * 512 uint4, s < 4 the W_e
// k-steps, s >= 4 the W_j ones, one scale per column block a over both (wmax behind the planes); the row scale is the
// maximum over the concatenated 256-value row.
// ZB: Z is stored as bf16 (the "bf16" edge-storage mode: half the bytes of the store that bounds this kernel; the
// logits are still taken from the fp32 values in registers)
template <bool ZB>
__global__ __launch_bounds__(256, 2) void edge_zx_kernel(const float* __restrict__ e, long lde,
                                                         const int* __restrict__ perm, const float* __restrict__ xn,
                                                         long ldx, const uint4* __restrict__ Wq, int ncb,
                                                         const float* __restrict__ Pi, const int* __restrict__ dsti,
                                                         const int* __restrict__ srci, long ld_add,
                                                         float* __restrict__ Z, long ldz, int E,
                                                         const float* __restrict__ wA, const float* __restrict__ bA,
                                                         int H, int cb_per_head, float* __restrict__ a_out) {
  constexpr int CH16 = 2 * 4 * 64;              // 16-byte pieces per chunk = 8 KB
  constexpr int RING = 8;                       // ring slots (see the vmcnt note at the loop's wait)
  __shared__ uint4 smem[RING * CH16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int row_w = blockIdx.x * 128 + wave * 32;
  const int row_a = row_w + n16, row_b = row_a + 16;
  const int rca = row_a < E ? row_a : E - 1, rcb = row_b < E ? row_b : E - 1;
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + lane;
  const unsigned t_off = (unsigned)tid * 16;
  const long last_chunk = (long)ncb * 16 - 1;
  const float* wmax = reinterpret_cast<const float*>(Wq + (long)ncb * 16 * CH16);

  // q[plane][2 s + nb]: s < 4 from e[perm[row]], s >= 4 from x[src[row]]
  bf16x8 q1[16], q2[16];
  float rs_a, rs_b;
  {
    const float* ra[2] = {e + (perm ? (long)perm[rca] : (long)rca) * lde, e + (perm ? (long)perm[rcb] : (long)rcb) * lde};
    const float* rx[2] = {xn + (long)srci[rca] * ldx, xn + (long)srci[rcb] * ldx};
    float qv[2][64];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float4* qp = reinterpret_cast<const float4*>((s < 4 ? ra[nb] : rx[nb]) + 32 * (s & 3) + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
        qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
      }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 64; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      float sq, iq;
      pow2_scale(m, sq, iq);
      if (nb) rs_b = iq; else rs_a = iq;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = qv[nb][8 * s + j] * sq;
        split2_x8_f16(v, q1[2 * s + nb], q2[2 * s + nb]);
      }
    }
  }
  const float* pia = Pi + (long)dsti[rca] * ld_add;
  const float* pib = Pi + (long)dsti[rcb] * ld_add;
  float* za = Z + (long)rca * ldz;
  float* zb = Z + (long)rcb * ldz;
  __bf16* za16 = reinterpret_cast<__bf16*>(Z) + (long)rca * ldz;
  __bf16* zb16 = reinterpret_cast<__bf16*>(Z) + (long)rcb * ldz;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#define EX_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const uint4* tb = Wq + gi * CH16;                                                          \
    const unsigned dst = wave_t + (unsigned)((gi_) & (RING - 1)) * (CH16 * 16);                \
    glds_b128(tb, t_off, dst);                                                                 \
    glds_b128(tb + 256, t_off, dst + 4096);                                                    \
  }
  EX_TLOAD(0l);
  EX_TLOAD(1l);
  EX_TLOAD(2l);
  EX_TLOAD(3l);
  EX_TLOAD(4l);
  EX_TLOAD(5l);
  EX_TLOAD(6l);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fb1, fb2;
#define EX_READ(F1_, F2_, slot_, cb_)                                                          \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * (CH16) + (cb_) * 64;                                   \
    F1_ = fp[0];                                                                               \
    F2_ = fp[4 * 64];                                                                          \
  }
#define EX_MFMA1(F1_, F2_, qi_, P_)                                                            \
  {                                                                                            \
    P_ = mma16<true>(F2_, q1[qi_], P_);                                                        \
    P_ = mma16<true>(F1_, q2[qi_], P_);                                                        \
    P_ = mma16<true>(F1_, q1[qi_], P_);                                                        \
  }
#define EX_MFMA(F1_, F2_, s_, cb_)                                                             \
  {                                                                                            \
    EX_MFMA1(F1_, F2_, 2 * (s_) + 0, part[2 * (cb_) + 0])                                      \
    EX_MFMA1(F1_, F2_, 2 * (s_) + 1, part[2 * (cb_) + 1])                                      \
  }
  EX_READ(fa1, fa2, 0, 0);
  f32x4 part[8];
  float dot_a = 0.f, dot_b = 0.f;
  const int ncbA = a_out ? H * cb_per_head : 0;
  for (int cb = 0; cb < ncb; ++cb) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
      for (int i = 0; i < 8; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {                  // chunk (cb, half, s) sits in ring slot s
        EX_TLOAD((long)cb * 16 + half * 8 + s + 7);
#pragma unroll
        for (int cbp = 0; cbp < 2; ++cbp) {
          EX_READ(fb1, fb2, s, 2 * cbp + 1);
          __builtin_amdgcn_sched_barrier(0);
          EX_MFMA(fa1, fa2, s, 2 * cbp);
          if (cbp == 0) EX_READ(fa1, fa2, s, 2)
          else EX_READ(fa1, fa2, (s + 1) & 7, 0);
          __builtin_amdgcn_sched_barrier(0);
          EX_MFMA(fb1, fb2, s, 2 * cbp + 1);
        }
        // At the end of k-step s chunk s + 2 must have landed (its fragments are read ahead during s + 1); it was
        // issued five k-steps ago.  vmcnt retires IN ORDER and counts stores: everything younger than that chunk may
        // stay in flight -- the five later chunks (10 loads) and, for s < 5, the eight Z stores of the previous
        // slice's epilogue, which were issued after it.  With a 4-slot ring the first wait after an epilogue already
        // had to drain the stores (a load issued after them was needed two k-steps later): the epilogue's write
        // latency was paid in full on every slice.
        if (s < 5) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      {
        float sw, iw;
        pow2_scale(wmax[cb], sw, iw);
        const float ma = rs_a * iw, mb = rs_b * iw;
#pragma unroll
        for (int i = 0; i < 4; ++i) { part[2 * i + 0] = part[2 * i + 0] * ma; part[2 * i + 1] = part[2 * i + 1] * mb; }
      }
      // ---- epilogue of the 64-column slice: z = part + Pi[dst]; store; logits ----
      const int col0 = cb * 128 + half * 64 + 4 * kg;
      const bool isA = cb < ncbA;
      // all Pi loads of the slice before its first store: a load issued after a store cannot be waited for without
      // draining that store (in-order vmcnt)
      float4 pia4[4], pib4[4];
#pragma unroll
      for (int c16 = 0; c16 < 4; ++c16) {
        pia4[c16] = *reinterpret_cast<const float4*>(pia + col0 + 16 * c16);
        pib4[c16] = *reinterpret_cast<const float4*>(pib + col0 + 16 * c16);
      }
      asm volatile("" ::: "memory");
#pragma unroll
      for (int c16 = 0; c16 < 4; ++c16) {
        const int col = col0 + 16 * c16;
        const float4 ia = pia4[c16], ib = pib4[c16];
        const f32x4 pa = part[2 * c16 + 0], pb = part[2 * c16 + 1];
        const float4 va = make_float4(pa[0] + ia.x, pa[1] + ia.y, pa[2] + ia.z, pa[3] + ia.w);
        const float4 vb = make_float4(pb[0] + ib.x, pb[1] + ib.y, pb[2] + ib.z, pb[3] + ib.w);
        // (non-temporal stores of Z were tried at the end of round 2: 2.77 -> 3.27 ms -- the 64-byte pieces of a row that
        // four consecutive store instructions write are merged into full lines by L2 only when they allocate there)
        // no `row < E` guard: the ring's vmcnt allowances count exactly eight stores per epilogue, and a wave whose
        // second row block lies past the end would skip four of them (lanes past the end hold the clamped row E - 1
        // and rewrite it with identical values)
        if constexpr (ZB) {
          store4_bf16(za16 + col, va);
          store4_bf16(zb16 + col, vb);
        } else {
          *reinterpret_cast<float4*>(za + col) = va;
          *reinterpret_cast<float4*>(zb + col) = vb;
        }
        if (isA) {
          const float4 w = *reinterpret_cast<const float4*>(wA + col);
          dot_a += (va.x > 0.f ? va.x : 0.01f * va.x) * w.x + (va.y > 0.f ? va.y : 0.01f * va.y) * w.y +
                   (va.z > 0.f ? va.z : 0.01f * va.z) * w.z + (va.w > 0.f ? va.w : 0.01f * va.w) * w.w;
          asm volatile("" : "+v"(dot_a));   // keep the two accumulations apart: see the note on packed math above
          dot_b += (vb.x > 0.f ? vb.x : 0.01f * vb.x) * w.x + (vb.y > 0.f ? vb.y : 0.01f * vb.y) * w.y +
                   (vb.z > 0.f ? vb.z : 0.01f * vb.z) * w.z + (vb.w > 0.f ? vb.w : 0.01f * vb.w) * w.w;
          asm volatile("" : "+v"(dot_b));
        }
      }
      if (isA && half == 1 && (cb + 1) % cb_per_head == 0) {
        const int h = cb / cb_per_head;
        float da = dot_a, db = dot_b;
        da += __shfl_xor(da, 16, 64); da += __shfl_xor(da, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        if (kg == 0) {
          const float bh = bA ? bA[h] : 0.f;
          if (row_a < E) a_out[(long)row_a * H + h] = da + bh;
          if (row_b < E) a_out[(long)row_b * H + h] = db + bh;
        }
        dot_a = 0.f; dot_b = 0.f;
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef EX_TLOAD
#undef EX_READ
#undef EX_MFMA1
#undef EX_MFMA
}

// planes of the two 128 x 128 blocks W_e[a], W_j[a] (element (k, c) = W[(128 a + c) * ldw + k]) under one scale
__global__ __launch_bounds__(256) void prepare_W2_f16_kernel(const float* __restrict__ We, const float* __restrict__ Wj,
                                                             long ldw, _Float16* __restrict__ dst,
                                                             float* __restrict__ wmax) {
  __shared__ float wm[4];
  const int a = blockIdx.x, tid = threadIdx.x;
  float v[2][64];
  float m = 0.f;
#pragma unroll
  for (int src = 0; src < 2; ++src)
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      const int i = r * 256 + tid, c = i >> 7, b = i & 127;      // k is the contiguous index of the source
      v[src][r] = (src ? Wj : We)[((long)a * 128 + c) * ldw + b];
      m = fmaxf(m, fabsf(v[src][r]));
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  if ((tid & 63) == 0) wm[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
  if (tid == 0) wmax[a] = m;
  float st, it;
  pow2_scale(m, st, it);
#pragma unroll
  for (int src = 0; src < 2; ++src)
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      const int i = r * 256 + tid, c = i >> 7, b = i & 127;
      plane_image_put<2, 256>(dst, a, 128 * src + b, c, v[src][r] * st);   // k = 128 src + b: W_e then W_j
    }
}

// =======================================================================================
// Launchers.  Every launch takes its operands as one record (kernels.h), asks edge_z_form ONCE which kernel runs in which
// shape, and hands record and form to the one function that expands them into that kernel's argument list.
// =======================================================================================
// Every kernel instantiation of this file.  First use decides the order in which the device code is emitted; naming them
// here, in the order they have always had, keeps the code object byte-identical whatever order the launchers below take.
[[maybe_unused]] static const void* const k_instantiations[] = {
    (const void*)edge_zx_kernel<true>, (const void*)edge_zx_kernel<false>,
    (const void*)edge_z6w_kernel<false, 3>, (const void*)edge_z6w_kernel<true, 0>, (const void*)edge_z6w_kernel<false, 0>,
    (const void*)edge_z_kernel<2, true>, (const void*)edge_z_kernel<2, false>, (const void*)edge_z_kernel<6, true, true>,
    (const void*)edge_z_kernel<6, true>, (const void*)edge_z_kernel<6, false>, (const void*)edge_z_kernel<3, true>,
    (const void*)edge_z_kernel<3, false>, (const void*)edge_z6w_kernel<false, 1>,
    (const void*)edge_msg_wsum_kernel<true>, (const void*)edge_msg_wsum_kernel<false>};
size_t edge_zx_wq_floats(int W2) { return (size_t)W2 * 256 + W2 / 128 + 64; }
bool edge_zx_dims(int C, int Ce, int W2, long ld_add, long ldz) {
  return mode_f16() && C == 128 && Ce == 128 && W2 % 128 == 0 && (ld_add % 4) == 0 && (ldz % 4) == 0;
}
// We / Wj: the edge_attr and x_j slices of the stacked first-layer weight (row stride ldw); Wq: edge_zx_wq_floats(W2)
int edge_zx_launch(const EdgeZParams& p, hipStream_t stream) {
  if (p.rows <= 0) return CGAT_OK;
  const int ncb = p.W2 / 128;
  hipLaunchKernelGGL(prepare_W2_f16_kernel, dim3(ncb), dim3(256), 0, stream, p.We, p.Wj, p.ldw, (_Float16*)p.Wq,
                     p.Wq + (size_t)ncb * 32768);
  CGAT_LAUNCH_CHECK();
  CGAT_PROF("edge_z", stream);
#define EZX_GO(ZB_)                                                                                                   \
  hipLaunchKernelGGL((edge_zx_kernel<ZB_>), dim3(cdiv(p.rows, 128)), dim3(256), 0, stream, p.e, p.lde, p.perm, p.x, p.ldx, \
                     (const uint4*)p.Wq, ncb, p.Pi, p.dsti, p.srci, p.ld_add, p.Z, p.ldz, p.rows, p.wA, p.bA, p.H,    \
                     p.Hd / 128, p.a_out)
  if (p.store == Z_BF16) EZX_GO(true);
  else EZX_GO(false);
#undef EZX_GO
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

bool edge_z_dims(int K, int W2, long lde, long ld_add, long ldz) {
  return mode_split() && K == 128 && W2 % 128 == 0 && (lde % 4) == 0 && (ld_add % 4) == 0 && (ldz % 4) == 0;
}

// floats of workspace for the pre-split weight
// three bf16 planes (the fp16 form: two), then room for the per-head column sums of edge_ge's bit-plane form
// (edgebwd.hip: H * 128 <= W2 / 2 floats at edge_ge_cs_offset)
size_t edge_ge_cs_offset(int W2) { return (((size_t)W2 * 128 * 3 + 1) / 2 + 3) / 4 * 4; }
size_t edge_z_wq_floats(int W2) { return edge_ge_cs_offset(W2) + (size_t)W2; }

// ---- which kernel runs: the parts of the decision, then the decision ----
// CGAT_EDGE_Z6W=0: the 128-row form of the six-pass per-edge launch (A/B switch); with it off there is no fused inference
static bool z6w_on() {
  static const bool on = [] { const char* e = getenv("CGAT_EDGE_Z6W"); return !(e && e[0] == '0'); }();
  return mode_24bit() && on;
}
// CGAT_Z_COL_GROUPS=0: no column groups over grid.y at few row tiles (A/B switch of the bit-identity test, like CGAT_EDGE_Z6W)
static int z_groups(int row_tiles, int ncb, int unit = 1) {
  static const bool on = [] { const char* e = getenv("CGAT_Z_COL_GROUPS"); return !(e && e[0] == '0'); }();
  return on ? z_col_groups(row_tiles, ncb, unit) : 1;
}
// Below 128 row tiles of 256 (the harness' shipped 64-crystal batch: 60 - 120 tiles) the 256-row kernels leave CUs idle:
// the training forward takes the 128-row kernel with column groups instead, the forward without grad deals the column
// blocks of its own two launches to grid.y groups; CGAT_Z_COL_GROUPS=0 turns both off.
static bool few_row_tiles(int rows) { return cdiv(rows, 256) < 128; }
// edge_z6w_kernel's operand limits: fc_out_A's weight within its LDS (hhd_logits: H * Hd of a launch that forms logits,
// else 0) and 32-bit gather offsets into n_add_rows known rows -- N * 4 * 2 H Hd < 2^32 bytes, kept as a guard rather than
// widened (100 000 atoms at H * Hd = 2048 use 1.6 GB of it)
static bool z6w_operands(long hhd_logits, int n_add_rows, long ld_add) {
  return hhd_logits <= 2048 && n_add_rows > 0 && (long)n_add_rows * 4 * ld_add < (1l << 32);
}
// Does the per-edge launch of these dims run edge_z6w_kernel (given gathered addends, a slot permutation and an activation
// it has): the 24-bit modes, not the few-row form (the harness' shipped batch: 60 workgroups walking 12 blocks, 119 us --
// the 128-row kernel with its column blocks dealt to grid.y groups fills the chip instead), and the operand limits.
static bool z6w_shape(int E, int ncb, int unit_z, bool z_bf16, long hhd_logits, int n_add_rows, long ld_add) {
  const bool few_rows = !z_bf16 && few_row_tiles(E) && z_groups(cdiv(E, 128), ncb, unit_z) > 1;
  return z6w_on() && !few_rows && z6w_operands(hhd_logits, n_add_rows, ld_add);
}

// edge_z_launch, edge_logits_launch (p.Z == null) and, as the plain product of linear128_rows below, the dense layer.
//   * edge_z6w_kernel: the six-pass per-edge launch on 256-row workgroups (same arithmetic, bit-identical results), where
//     z6w_shape holds and the launch has what that kernel is written for; the running maximum shares a register with the
//     logits, so not both.
//   * edge_z_kernel otherwise.  Few rows beside many column blocks -- at the harness' shipped batch the per-node
//     projections are 10 workgroups and the per-edge first layer of a vector-attention layer 240, each walking 20 blocks
//     (149 / 180 us per launch, 2.4 ms of an 18-ms step) -- : the column blocks are dealt to grid.y groups (round 6).  A
//     workgroup then splits its rows once per group (64 KB, L2-resident) and walks ncb / G blocks; every block is computed
//     as before: bit-identical.  The 24-bit modes only (the fp16 image keeps its scale behind the LAST block), fp32 storage.
//     With logits a group holds whole heads: a head's logit is the sum over ITS column blocks only, and the group carries
//     the number of blocks in front of it (head index, fc_out_A's weight row).
EdgeZForm edge_z_form(const EdgeZParams& p) {
  EdgeZForm f = {};
  if (p.rows <= 0) return f;
  const int ncb = p.W2 / 128;
  const bool logits = p.a_out != nullptr;
  const int unit = logits ? p.Hd / 128 : 1;   // column blocks that stay in one group
  f.passes = mode_f16() ? 2 : mode_bf16x3() ? 3 : 6;
  f.adds = p.Pj != nullptr;
  f.zb = p.store == Z_BF16;
  f.G = 1;
  f.ncb_g = ncb;
  if (!p.Z) {   // logits only: the attention column blocks, in groups of whole heads at few row tiles
    f.kernel = EZK_ROWS256; f.z6w_mode = 1; f.tile_rows = 256;
    f.grid_x = cdiv(p.rows, 256);
    if (few_row_tiles(p.rows)) f.G = z_groups(f.grid_x, p.H * p.Hd / 128, unit);
    f.ncb_g = p.H * p.Hd / 128 / f.G;
  } else if (z6w_shape(p.rows, ncb, unit, f.zb, logits ? (long)p.H * p.Hd : 0, p.n_add_rows, p.ld_add) && p.Pj && p.perm &&
             (p.act == CGAT_ACT_NONE || p.act == CGAT_ACT_LEAKY) && !(p.omax && logits)) {
    f.kernel = EZK_ROWS256; f.z6w_mode = p.store == Z_BITS ? 3 : 0; f.tile_rows = 256;
    f.grid_x = cdiv(p.rows, 256);
  } else {
    f.kernel = EZK_ROWS128; f.tile_rows = 128;
    f.grid_x = cdiv(p.rows, 128);
    if (mode_24bit() && !f.zb) f.G = z_groups(f.grid_x, ncb, unit);
    f.ncb_g = ncb / f.G;
  }
  return f;
}
// what edge_z_launch refuses, given the form it would run
static int edge_z_check(const EdgeZParams& p, const EdgeZForm& f) {
  CGAT_CHECK_ARG(p.store != Z_BF16 || (p.Pj != nullptr && mode_24bit() && p.act == CGAT_ACT_NONE && !p.omax),
                 "edge_z: bf16 storage is the per-edge launch of the six-pass form only");
  CGAT_CHECK_ARG(p.store != Z_BITS || (f.kernel == EZK_ROWS256 && p.Pj && p.perm && p.a_out && p.wA && p.act == CGAT_ACT_NONE &&
                                       !p.omax && p.ld_add == p.ldz && 2l * p.n_add_rows + cdiv(p.rows, 32) <= (long)p.rows &&
                                       (long)p.H * p.Hd == p.W2 / 2),
                 "edge_z: the bit form of the training forward is edge_z6w_kernel's, with logits (edge_z6w_takes)");
  return CGAT_OK;
}

// A record of what edge_z_form reads and no more -- dims, storage and which optional operands are PRESENT -- for the
// questions asked before there are operands (edge_z6w_takes, the debug query).  Never launched.
static EdgeZParams edge_z_shape(int rows, int W2, int H, int Hd, int n_add_rows, long ld_add, ZStore store, bool adds,
                                bool logits, bool omax, int act, bool z = true) {
  alignas(16) static float present_f;
  static int present_i;
  EdgeZParams p = {};
  p.rows = rows; p.W2 = W2; p.H = H; p.Hd = Hd; p.n_add_rows = n_add_rows; p.ld_add = p.ldz = ld_add; p.store = store;
  p.act = act;
  p.e = &present_f;
  if (z) p.Z = &present_f;
  if (adds) { p.Pi = p.Pj = &present_f; p.perm = p.dsti = p.srci = &present_i; }
  if (logits) { p.wA = &present_f; p.a_out = &present_f; }
  if (omax) p.omax = &present_f;
  return p;
}
// ... the fp32 training forward of a scalar-attention layer [E, 2 H Hd] over N nodes, at 128 row tiles or more -- where no
// switch (CGAT_Z_COL_GROUPS) decides between this kernel and the few-row form (layers.hip: the bit form's predicate)
bool edge_z6w_takes(int N, int E, int H, int Hd) {
  const int W2 = 2 * H * Hd;
  return Hd % 128 == 0 && !few_row_tiles(E) &&
         edge_z_form(edge_z_shape(E, W2, H, Hd, N, W2, Z_F32, true, true, false, CGAT_ACT_NONE)).kernel == EZK_ROWS256;
}

// ---- the kernels' argument lists, each expanded here and nowhere else ----
// per-group offsets of a launch whose grid.y runs over the form's column groups (HeadBatch: w in 16-byte pieces)
static HeadBatch col_groups(const EdgeZForm& f) {
  if (f.G == 1) return HeadBatch{};
  const long c = (long)f.ncb_g * 128;
  return HeadBatch{0, (long)f.ncb_g * 6144, c, c, c, c, (long)f.ncb_g};
}
// grid.y = f.G groups (or heads) whose operands lie hb apart; accumulate / dact / ld_dact: the dense layer's extras
static void edge_z_rows128(const EdgeZForm& f, const EdgeZParams& p, const HeadBatch& hb, hipStream_t stream,
                           int accumulate = 0, const float* dact = nullptr, long ld_dact = 0) {
#define EZ_GO(P_, A_, ZB_)                                                                                            \
  hipLaunchKernelGGL((edge_z_kernel<P_, A_, ZB_>), dim3(f.grid_x, f.G), dim3(256), 0, stream, p.e, p.lde, p.perm,     \
                     (const uint4*)p.Wq, f.ncb_g, p.Pi, p.dsti, p.Pj, p.srci, p.ld_add, p.Z, p.ldz, p.rows, p.wA, p.bA, p.H, \
                     p.Hd / 128, p.a_out, p.act, accumulate, p.omax, dact, ld_dact, hb)
  if (f.passes == 2) { if (f.adds) EZ_GO(2, true, false); else EZ_GO(2, false, false); }
  else if (f.passes == 6 && f.zb) EZ_GO(6, true, true);
  else if (f.passes == 6) { if (f.adds) EZ_GO(6, true, false); else EZ_GO(6, false, false); }
  else { if (f.adds) EZ_GO(3, true, false); else EZ_GO(3, false, false); }
#undef EZ_GO
}
static void edge_z_rows256(const EdgeZForm& f, const EdgeZParams& p, hipStream_t stream) {
  // the bit form's holes behind the two half projections: rows 2 N + g of Z
  unsigned* zbits = f.z6w_mode == 3 ? reinterpret_cast<unsigned*>(p.Z + 2l * p.n_add_rows * p.ldz) : nullptr;
#define Z6_GO(ZB_, M_)                                                                                                \
  hipLaunchKernelGGL((edge_z6w_kernel<ZB_, M_>), dim3(f.grid_x, f.G), dim3(512), 0, stream, p.e, p.lde, p.perm,       \
                     (const uint4*)p.Wq, f.ncb_g, p.Pi, p.dsti, p.Pj, p.srci, p.ld_add, p.Z, p.ldz, p.rows, p.wA, p.bA, p.H, \
                     p.Hd / 128, p.a_out, p.act, p.omax, zbits)
  if (f.z6w_mode == 3) Z6_GO(false, 3);
  else if (f.z6w_mode == 0 && f.zb) Z6_GO(true, 0);
  else if (f.z6w_mode == 0) Z6_GO(false, 0);
  else Z6_GO(false, 1);
#undef Z6_GO
}

int edge_z_launch(const EdgeZParams& p, hipStream_t stream) {
  if (p.rows <= 0) return CGAT_OK;
  const int ncb = p.W2 / 128;
  const EdgeZForm f = edge_z_form(p);
  CGAT_TRY(edge_z_check(p, f));
  // operand (a = column block, b = k, c = column in block) = We[(128 a + c) * ldw + b]
  // (We == nullptr: the caller has prepared that image in Wq already, e.g. several slices in one launch)
  if (!p.We) {}
  else if (mode_f16()) CGAT_TRY(prepare_W_f16_launch(p.We, p.Wq, ncb, 128 * p.ldw, 1, p.ldw, stream));
  else CGAT_TRY(prepare_T_planes_launch(p.We, p.Wq, ncb, 128 * p.ldw, 1, p.ldw, 0, stream));
  CGAT_PROF(p.Pj ? "edge_z" : "edge_proj", stream);   // the per-edge launch / the per-node projections
  if (f.kernel == EZK_ROWS256) edge_z_rows256(f, p, stream);
  else edge_z_rows128(f, p, col_groups(f), stream);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- the forward without grad (edge_z6w_kernel<., 1> and edge_msg_wsum_kernel above) ----
// The shapes at which edge_z_launch runs the per-edge launch of the 24-bit modes with the six-pass arithmetic (C = Ce =
// 128, Hd % 128 == 0; as edge_z6w_kernel or, below 128 row tiles of 256, as the 128-row kernel with column groups: the
// same Z and logits), with
//   * edge_z6w_kernel's operand limits at W2 = 2 H Hd (the carry of edge_msg_wsum_kernel stays within its 16 KB by column
//     groups) and at most 8 heads (its alpha staging);
//   * E * H % 4 == 0.
bool edge_infer_fused(int N, int E, int C, int Ce, int H, int Hd) {
  const long HHd = (long)H * Hd;
  return z6w_on() && C == 128 && Ce == 128 && Hd % 128 == 0 && H <= 8 && E > 0 &&
         // the training forward's S sits behind Z and alpha in the saved buffer and is 16-byte aligned only when
         // E * H % 4 == 0; otherwise seg_wsum_launch takes its scalar kernel, whose order is not the one built here
         ((long)E * H) % 4 == 0 && z6w_operands(HHd, N, 2 * HHd);
}
int edge_logits_launch(const EdgeZParams& p, hipStream_t stream) {
  CGAT_CHECK_ARG(p.W2 == 2 * p.H * p.Hd && p.Hd % 128 == 0 && p.H * p.Hd <= 2048 && (p.lde % 4) == 0 && p.wA && p.a_out &&
                 p.perm && !p.Z && aligned16(p.e, p.Pi, p.Pj, p.wA),
                 "edge_logits: needs Hd %% 128 == 0, H * Hd <= 2048, 16-byte aligned rows and fc_out_A's weight");
  if (p.rows <= 0) return CGAT_OK;
  CGAT_TRY(prepare_T_planes_launch(p.We, p.Wq, p.W2 / 128, 128 * p.ldw, 1, p.ldw, 0, stream));   // (the whole W2 image: edge_msg_wsum's too)
  CGAT_PROF("edge_logits", stream);
  edge_z_rows256(edge_z_form(p), p, stream);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
// rows per workgroup: a range that starts and ends at segment boundaries is at most R + (longest segment - 1) rows, so
// 256 minus the mean in-degree (rounded up to 16) keeps ordinary ranges in one 256-row sub-tile.
// column groups: to fill the chip at few rows, and at least as many as keep the carry of a long segment's Glong row
// groups within WSUM_CARRY floats
static EdgeZForm edge_msg_wsum_form(const EdgeZParams& p) {
  EdgeZForm f = {};
  if (p.rows <= 0) return f;
  const int HHd = p.H * p.Hd, ncb = HHd / 128;
  const long deg = cdiv(p.rows, p.N);
  f.kernel = EZK_MSG_WSUM; f.passes = 6; f.adds = true; f.zb = p.store == Z_BF16;
  f.tile_rows = (int)(deg >= 128 ? 128 : 256 - 16 * cdiv(deg, 16));
  f.grid_x = cdiv(p.rows, f.tile_rows);
  const int Glong = 1024 / (HHd / 4 < 256 ? HHd / 4 : 256);
  f.G = few_row_tiles(p.rows) ? z_groups(f.grid_x, ncb) : 1;
  while (ncb % f.G != 0 || (long)Glong * (ncb / f.G) * 128 > WSUM_CARRY) ++f.G;
  f.ncb_g = ncb / f.G;
  return f;
}
static int edge_msg_wsum_check(const EdgeZParams& p) {
  CGAT_CHECK_ARG(p.W2 == 2 * p.H * p.Hd && p.Hd % 128 == 0 && p.H * p.Hd <= 2048 && p.H <= 8 && (p.lde % 4) == 0 && p.perm &&
                 p.N > 0 && aligned16(p.e, p.Pi, p.Pj, p.S),
                 "edge_msg_wsum: needs Hd %% 128 == 0, H * Hd <= 2048, H <= 8 and 16-byte aligned rows");
  return CGAT_OK;
}
// Wq: the image edge_logits_launch made; Pi / Pj: [N, W2] (the message columns are the second half)
int edge_msg_wsum_launch(const EdgeZParams& p, hipStream_t stream) {
  CGAT_TRY(edge_msg_wsum_check(p));
  if (p.rows <= 0) return CGAT_OK;
  const int HHd = p.H * p.Hd;
  const EdgeZForm f = edge_msg_wsum_form(p);
  const uint4* Wm = reinterpret_cast<const uint4*>(p.Wq) + (long)(HHd / 128) * 6144;   // the message column blocks' image
  CGAT_PROF("edge_msg_wsum", stream);
#define WSUM_GO(ZB_)                                                                                                  \
  hipLaunchKernelGGL(edge_msg_wsum_kernel<ZB_>, dim3(f.grid_x, f.G), dim3(512), 0, stream, p.e, p.lde, p.perm, Wm, f.ncb_g, \
                     p.Pi + HHd, p.dsti, p.Pj + HHd, p.srci, (long)p.W2, p.H, p.Hd, p.alpha, p.rowptr, p.N, f.tile_rows, p.S)
  if (f.zb) WSUM_GO(true);
  else WSUM_GO(false);
#undef WSUM_GO
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- dense layer at width 128: out[n, :] = act(in[n, :] W^T + bias) + beta * out[n, :],  W(o, k) = W[o*so + k*sk] ----
// The hypernetwork trunks (Linear + Tanh, reference Hypernetworksmp.py:24-60) and the linear terms of the predicted
// layers are [rows,128] x [128,128] products; on the generic 128x128x32 GEMM tile they are all prologue and epilogue.
// Here they run as the one-column-block case of the kernel above (rows split once into registers, 96 KB of weight
// planes through the LDS-DMA ring).
bool linear128_fast(int K, int N, long ldi, long ldo, const void* in, const void* out) {
  return mode_split() && K == 128 && N >= 128 && N % 128 == 0 && (ldi % 4) == 0 && (ldo % 4) == 0 && aligned16(in, out);
}
size_t linear128_ws_bytes(int n_out) { return ws_round((size_t)n_out * 128 * 3 / 2 + 4, 4); }
// the layer as the per-edge kernel's plain product: e = in, Pi = the bias vector, Z = out, no logits
static EdgeZParams linear128_rows(const Linear128Params& p, void* image) {
  EdgeZParams r = {};
  r.e = p.in; r.lde = p.ldi; r.rows = p.rows;
  r.Wq = (float*)image; r.W2 = p.n_out;
  r.Pi = p.bias;
  r.Z = p.out; r.ldz = p.ldo;
  r.H = 1; r.Hd = 128;
  r.act = p.act; r.omax = p.omax;
  return r;
}
int linear128_launch(const Linear128Params& p, void* ws, hipStream_t stream) {
  if (p.rows <= 0) return CGAT_OK;
  const int ncb = p.n_out / 128;
  // operand (a = output block, b = k, c = output in block) = W[(128 a + c) * so + b * sk]
  // prepared: the mode's image of this weight made ahead of time (f16x3: prepare_W_f16_batch_launch; the bf16 forms:
  // prepare_T_bf16_batch_launch), n_out == 128 only
  if (p.prepared && p.n_out == 128) ws = const_cast<void*>(p.prepared);
  else if (mode_f16()) CGAT_TRY(prepare_W_f16_launch(p.W, ws, ncb, 128 * p.so, p.sk, p.so, stream));
  else CGAT_TRY(prepare_T_planes_launch(p.W, ws, ncb, 128 * p.so, p.sk, p.so, 0, stream));
  CGAT_PROF("linear128", stream);
  const EdgeZParams r = linear128_rows(p, ws);
  const EdgeZForm f = edge_z_form(r);   // (column blocks over grid.y when the row tiles leave CUs idle)
  edge_z_rows128(f, r, col_groups(f), stream, p.accumulate, p.dact, p.ld_dact);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// The same product for `heads` independent (input, weight, output) triples in ONE launch pair: head h reads
// in + h * s_in, W + h * s_w (the same (so, sk) element strides), bias + h * s_bias, dact + h * s_dact and writes
// out + h * s_out.  The per-head second layers of a vector-attention layer at the harness' shipped batch are 2 H chains
// of [prepare, product] launches of 20-40 us each that fill a fraction of the chip; as grid.y they are one.
// ws: heads * linear128_heads_image_floats(n_out) floats.
// (sized for the six-pass image: three bf16 planes per 128 x 128 block)
size_t linear128_heads_image_floats(int n_out) { return (size_t)(n_out / 128) * 24576 + ((n_out / 128 + 3) & ~3); }
int linear128_heads_launch(const Linear128Params& p, void* ws, hipStream_t stream) {
  if (p.rows <= 0 || p.heads <= 0) return CGAT_OK;
  CGAT_CHECK_ARG((mode_f16() || mode_24bit()) && p.n_out % 128 == 0,
                 "linear128_heads: split arithmetic modes and 128-wide output blocks only");
  const int ncb = p.n_out / 128;
  const long img = (long)linear128_heads_image_floats(p.n_out);
  // one image launch for all heads (the 24-bit modes, round 6: the six-pass image), one product launch
  if (mode_f16()) CGAT_TRY(prepare_W_f16_launch(p.W, ws, ncb, 128 * p.so, p.sk, p.so, stream, p.heads, p.s_w, img));
  else CGAT_TRY(prepare_T_planes_launch(p.W, ws, ncb, 128 * p.so, p.sk, p.so, 0, stream, nullptr, p.heads, p.s_w, img));
  CGAT_PROF("linear128", stream);
  const EdgeZParams r = linear128_rows(p, ws);
  EdgeZForm f = edge_z_form(r);
  f.G = p.heads; f.ncb_g = ncb;         // grid.y runs over the heads, each over all its column blocks: no column groups
  edge_z_rows128(f, r, HeadBatch{p.s_in, img / 4, p.s_bias, p.s_out, p.s_dact}, stream, p.accumulate, p.dact, p.ld_dact);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// debug (include/cgat_hip.h): the form of a launch of these dims, storage and present operands in the current mode
extern "C" int cgat_debug_edge_z_form(int32_t launch, int32_t rows, int32_t W2, int32_t H, int32_t Hd, int32_t n_add_rows,
                                      int64_t ld_add, int32_t store, int32_t adds, int32_t logits, int32_t omax,
                                      int32_t act, cgat_edge_z_form* out) {
  CGAT_CHECK_ARG(out && launch >= 0 && launch <= 2 && store >= Z_F32 && store <= Z_BITS && rows >= 0 && W2 > 0 &&
                 W2 % 128 == 0 && H > 0 && Hd > 0, "debug_edge_z_form: bad arguments");
  EdgeZParams p = edge_z_shape(rows, W2, H, Hd, n_add_rows, ld_add, (ZStore)store, adds != 0 || launch != 0,
                               logits != 0 || launch == 1, omax != 0, act, launch == 0);
  p.N = n_add_rows;
  EdgeZForm f;
  if (launch == 2) { CGAT_TRY(edge_msg_wsum_check(p)); f = edge_msg_wsum_form(p); }
  else { f = edge_z_form(p); if (launch == 0) CGAT_TRY(edge_z_check(p, f)); }
  *out = {f.kernel, f.passes, f.adds, f.zb, f.z6w_mode, f.G, f.ncb_g, f.grid_x, f.tile_rows};
  return CGAT_OK;
}

