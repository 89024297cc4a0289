// Backward products of the per-edge first-layer weight W_e over the 1536-wide pre-activation gradient gZ
// (the `edge_attr` slice of MultiHeadNetwork.fc_in for both message networks, reference CGAT.py:96):
//     g_edge_attr[perm[t], :] = gZ[t, :] @ W_e               (edge_ge_kernel,  K = 1536, 128 outputs per edge)
// gZ is produced once per step by edge_seg_bwd_kernel in 128-column blocks [W2/128][E][128] and read here
// straight from HBM: every element is used for only 128 multiply-adds, so the split into three bf16 planes
// (bilinear.hip: six v_mfma_f32_16x16x32_bf16 passes, fp32 accumulation, fp32-equivalent) happens in the loop
// -- ~64 VALU instructions per 96 MFMAs and wave, overlapped by the second wave of the SIMD -- while W_e
// arrives pre-split in fragment order through a double-buffered LDS tile shared by the 8 waves.
#include <string.h>
#include "../../include/cgat_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

// Wq: prepare_T_bf16 planes of the operand (a = 128-column block of gZ, b = column in block, c = output) =
// W_e[128 a + b][c]; chunk (a, half, s) = 12 KB at Wq + ((a*2 + half)*4 + s) * 768 uint4.
// RC: the operand is not read but rebuilt from its ingredients (struct EdgeRC, kernels.h): per k-step and row one mask
// word, one coefficient and 8 floats of a per-node row (or of the constant wA) instead of 8 floats of gZ
// LeakyReLU'(z) from the sign bit: 1.0f or 0.01f chosen by a bitwise select of the two bit patterns (v_bfe_i32 +
// v_bfi_b32: two instructions instead of the and / compare / cndmask a `?:` compiles to)
__device__ __forceinline__ float rc_d(unsigned m, int bit) {
  const unsigned s = (unsigned)((int)(m << (31 - bit)) >> 31);
  return __uint_as_float((s & 0x3F800000u) | (~s & 0x3C23D70Au));
}
// eight mask bits -> the bf16 fragment of their values 0 / 1 (0x3F80 = 1.0): one plane, exact
__device__ __forceinline__ bf16x8 bits8_bf16(unsigned m) {
  uint4 w;
#define GE_BITPAIR(i_) ((((unsigned)((int)(m << (31 - 2 * (i_))) >> 31)) & 0x3F80u) |                     \
                        (((unsigned)((int)(m << (30 - 2 * (i_))) >> 31)) & 0x3F800000u))
  w.x = GE_BITPAIR(0); w.y = GE_BITPAIR(1); w.z = GE_BITPAIR(2); w.w = GE_BITPAIR(3);
#undef GE_BITPAIR
  return __builtin_bit_cast(bf16x8, w);
}
// BP (with RC, six passes: scalar attention in the 24-bit modes; edge_ge_bitplane below): the k-steps of the ATTENTION
// half run on the stored bit alone.  There gZ[t, (h, c)] = ga[t, h] wA[h, c] d, d = 1 or 0.01 by the bit m, so with
// W'[(h, c), :] = wA[h, c] W_e[(h, c), :] (prepare_T_bf16_attn_launch: the image's attention blocks hold W')
//     sum_c gZ[t, (h, c)] W_e[(h, c), :] = ga[t, h] * (P + 0.01 (cs_h - P)),   P = sum_c m[t, h, c] W'[(h, c), :],
// cs_h = sum_c W'[(h, c), :].  m is exact in ONE bf16 plane: P takes three passes (the planes of W') instead of six and
// its row operand is eight shifted bits -- no coefficient, no wA, no multiply, no split.  P is summed per head in a
// second accumulator set and folded into the first at the head's last block (GA_FLUSH: the arithmetic is pinned there).
template <int PASSES, bool RC = false, bool BP = false>
__global__ __launch_bounds__(512, 2) void edge_ge_kernel(const float* __restrict__ gZ, long ldg, long gzb,
                                                         const uint4* __restrict__ Wq, int ncb,
                                                         float* __restrict__ out, long ldo,
                                                         const int* __restrict__ scatter, int E, int accumulate,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ amax, const EdgeRC rc, HeadBatch hb) {
  // grid.y = head of a multi-head second layer (edge_ge_heads_launch): per-head operand offsets
  gZ += (long)blockIdx.y * hb.in;
  Wq += (long)blockIdx.y * hb.w;
  out += (long)blockIdx.y * hb.out;
  if (bias) bias += (long)blockIdx.y * hb.bias;
  // PASSES == 2: two fp16 planes, three passes (mfma_bf16.h).  The rows of gZ are consumed k-step by k-step, so their
  // scale is per tensor: amax[0] = max |gZ| from the kernel that produced it; the weight's max sits behind its planes.
  // PASSES == 1 (edge storage "bf16-mma", BASELINE configs[4]'s "bf16 activations with MFMA edge-MLP"): ONE bf16 pass on
  // the leading planes of both operands -- bf16 operands, fp32 accumulation; the three-plane weight image is read as
  // it is (its first plane is the round-to-nearest bf16 of the weight), only that plane is staged
  constexpr bool F16 = PASSES == 2;
  constexpr bool ONE = PASSES == 1;
  constexpr int NP = F16 ? 2 : 3;
  constexpr int HP = NP * 256;                   // 16-byte pieces of one (a, half, k-step) block
  __shared__ uint4 Bs[2][2 * HP];                // [buffer][half][plane][cb][lane]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int row_w = blockIdx.x * 256 + wave * 32;
  const int row_a = row_w + n16, row_b = row_a + 16;
  const long rca = row_a < E ? row_a : E - 1, rcb = row_b < E ? row_b : E - 1;
  // element (t, 128 a + j) of the operand lives at gZ[t * ldg + a * gzb + j]: (ldg, gzb) = (128, E * 128) for the
  // column-blocked gZ, (W2, 128) for a plain row-major matrix
  const float* ga = gZ + rca * ldg + 8 * kg;     // + a * gzb + 32 s
  const float* gb = gZ + rcb * ldg + 8 * kg;
  const int nk = ncb * 4;
  const int ks0 = RC ? (int)((long)blockIdx.y * hb.ks0) : 0;
  // RC: per-row bases of the ingredients
  const unsigned* mka = nullptr; const unsigned* mkb = nullptr;
  const float *gsa = nullptr, *gsb = nullptr, *caA = nullptr, *cbA = nullptr, *caM = nullptr, *cbM = nullptr;
  if constexpr (RC) {
    mka = rc.mask + rca * rc.nw; mkb = rc.mask + rcb * rc.nw;
    gsa = rc.gS + (long)rc.dst[rca] * rc.HHd + 8 * kg; gsb = rc.gS + (long)rc.dst[rcb] * rc.HHd + 8 * kg;
    caA = rc.ga + rca * rc.H; cbA = rc.ga + rcb * rc.H;
    caM = rc.alpha + rca * rc.H; cbM = rc.alpha + rcb * rc.H;
  }

  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sA = 1.f, inv_all = 1.f;
  if constexpr (F16) {
    float iA, sW, iW;
    pow2_scale(amax[0], sA, iA);
    pow2_scale(reinterpret_cast<const float*>(Wq + (long)ncb * 8 * HP)[0], sW, iW);
    inv_all = iA * iW;
  }

  // B staging: thread tid moves 16-byte pieces tid, tid + 512 (, tid + 1024) of the k-step's [half0 | half1] image
  // (sb*: the tile stored at the end of this iteration, loaded during the previous one; tb*: the tile after it, loaded
  // during this iteration -- a tile loaded and stored within one iteration left every wave waiting for its L2 latency
  // in front of the barrier)
  uint4 sb0, sb1, sb2, tb0, tb1, tb2;
  const int p1 = tid + 512, p2 = tid + 1024;
  const int p0 = tid < 256 ? tid : HP + tid - 256;      // ONE: where the thread's plane-0 piece lives in the tile
#define GE_BLOAD(ks_, B0_, B1_, B2_)                                                                     \
  {                                                                                                      \
    const long a_ = (ks_) >> 2, s_ = (ks_) & 3;                                                          \
    const uint4* h0 = Wq + ((a_ * 2 + 0) * 4 + s_) * HP;                                                 \
    const uint4* h1 = Wq + ((a_ * 2 + 1) * 4 + s_) * HP;                                                 \
    if (ONE) {                       /* plane 0 of each half: 256 + 256 pieces, one per thread */          \
      B0_ = tid < 256 ? h0[tid] : h1[tid - 256];                                                         \
    } else {                                                                                             \
      B0_ = h0[tid];                                                                                     \
      B1_ = p1 < HP ? h0[p1] : h1[p1 - HP];                                                              \
      if (NP == 3) B2_ = h1[p2 - HP];                                                                    \
    }                                                                                                    \
  }
#define GE_BSTORE(buf_)                                                                                  \
  {                                                                                                      \
    if (ONE) {                                                                                           \
      Bs[buf_][p0] = sb0;                                                                                \
    } else {                                                                                             \
      Bs[buf_][tid] = sb0; Bs[buf_][p1] = sb1;                                                           \
      if (NP == 3) Bs[buf_][p2] = sb2;                                                                   \
    }                                                                                                    \
  }
  // raw gZ (rows a/b, 8 columns each) of the next k-step (ra*, rb*) and of the one after (sa*, sb*): loads are
  // issued two k-steps (~3 us) before their values are split, enough bytes in flight per CU to cover HBM latency
  float4 ra0, ra1, rb0, rb1, sa0, sa1, sb0_, sb1_;
  // RC: coefficient and mask word of rows a / b for the k-step in r* (rc*) and in s* (sc*)
  float rca_c = 0.f, rcb_c = 0.f, sca_c = 0.f, scb_c = 0.f;
  unsigned rca_m = 0, rcb_m = 0, sca_m = 0, scb_m = 0;
#define GE_ALOAD(ks_, A0_, A1_, B0_, B1_, CA_, CB_, MA_, MB_)                                            \
  {                                                                                                      \
    if constexpr (RC) {                                                                                  \
      const int kk_ = (ks_) + ks0;                     /* k-step within the whole row (K groups, grid.y) */  \
      const int c0_ = 32 * kk_;                        /* first column of the k-step (uniform) */           \
      const bool isA_ = c0_ < rc.HHd;                                                                    \
      const int cc_ = isA_ ? c0_ : c0_ - rc.HHd, h_ = cc_ / rc.Hd;                                       \
      const float4* pa = reinterpret_cast<const float4*>(isA_ ? rc.wA + cc_ + 8 * kg : gsa + cc_);      \
      const float4* pb = reinterpret_cast<const float4*>(isA_ ? rc.wA + cc_ + 8 * kg : gsb + cc_);      \
      A0_ = pa[0]; A1_ = pa[1]; B0_ = pb[0]; B1_ = pb[1];                                                \
      CA_ = (isA_ ? caA : caM)[h_]; CB_ = (isA_ ? cbA : cbM)[h_];                                        \
      MA_ = mka[kk_]; MB_ = mkb[kk_];                                                                    \
    } else {                                                                                             \
      const long off = (long)((ks_) >> 2) * gzb + 32 * ((ks_) & 3);                                      \
      const float4* pa = reinterpret_cast<const float4*>(ga + off);                                      \
      const float4* pb = reinterpret_cast<const float4*>(gb + off);                                      \
      A0_ = pa[0]; A1_ = pa[1]; B0_ = pb[0]; B1_ = pb[1];                                                \
    }                                                                                                    \
  }
  // RC: the stored value was (coefficient * vector) * d, rebuilt in the same order
#define GE_SPLIT(R0_, R1_, C_, M_, Q1_, Q2_, Q3_)                                                        \
  {                                                                                                      \
    float g_[8] = {R0_.x, R0_.y, R0_.z, R0_.w, R1_.x, R1_.y, R1_.z, R1_.w};                              \
    if constexpr (RC) {           /* the power-of-two scale of the fp16 form rides on the coefficient: exact */ \
      const unsigned mb_ = (M_) >> (8 * kg);                                                             \
      const float cs_ = F16 ? (C_) * sA : (C_);                                                          \
      /* __fmul_rn: the stored value was ROUNDED; contracted into the split's v - hi it would not be */   \
      _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) g_[i_] = __fmul_rn(cs_ * g_[i_], rc_d(mb_, i_));  \
    }                                                                                                    \
    if constexpr (F16 && !RC) {                                                                          \
      const float v[8] = {g_[0] * sA, g_[1] * sA, g_[2] * sA, g_[3] * sA,                                \
                          g_[4] * sA, g_[5] * sA, g_[6] * sA, g_[7] * sA};                               \
      split2_x8_f16(v, Q1_, Q2_);                                                                        \
    } else if constexpr (F16) {                                                                          \
      split2_x8_f16(g_, Q1_, Q2_);                                                                       \
    } else {                                                                                             \
      split3_x8(g_, Q1_, Q2_, Q3_);                                                                      \
    }                                                                                                    \
  }
  // BP: the attention k-steps of this launch group come first (whole column blocks: HHd % 128 == 0, groups are whole
  // blocks), the loop below then starts at block aA.  The accumulators keep the sign convention of that loop -- at the
  // start of block a they hold (-1)^a times the sum so far -- and so does the per-head set.
  int aA = 0;
  if constexpr (BP) {
    static_assert(RC && PASSES == 6, "the bit-plane body belongs to the six-pass rebuilt form");
    __shared__ float Cs[8 * 128];                  // cs of every head (H <= 8), signed as the flush meets it
    const int nA = min(nk, max(0, rc.HHd / 32 - ks0));
    aA = nA >> 2;
    if (aA > 0) {
      for (int i = tid; i < rc.H * 128; i += 512) Cs[i] = rc.cs[i];
      const int hsteps = rc.Hd >> 5;               // k-steps per head (a multiple of 4)
      f32x4 part[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      unsigned ma[4], mb[4], xa[4], xb[4];         // mask words of rows a / b: this block's, the next block's
#pragma unroll
      for (int s = 0; s < 4; ++s) { ma[s] = mka[ks0 + s]; mb[s] = mkb[ks0 + s]; }
      GE_BLOAD(0, sb0, sb1, sb2);
      GE_BSTORE(0);
      GE_BLOAD(1, sb0, sb1, sb2);
      __syncthreads();
      // k-step ks: its tile is in Bs[ks & 1], the tile of ks + 1 in flight in one register set; the tile of ks + 2 is
      // requested into the other set, the MFMAs run, the first set is stored into the other buffer
#define GA_STEP(ks_, buf_, MA_, MB_, UB0, UB1, UB2, TB0, TB1, TB2)                                         \
      {                                                                                                  \
        const int kl_ = (ks_) + 2 < nA ? (ks_) + 2 : nA - 1;                                             \
        GE_BLOAD(kl_, TB0, TB1, TB2);                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        const bf16x8* bs = reinterpret_cast<const bf16x8*>(&Bs[buf_][lane]);                             \
        const bf16x8 qa = bits8_bf16((MA_) >> (8 * kg)), qb = bits8_bf16((MB_) >> (8 * kg));             \
        bf16x8 f1 = bs[0], f2 = bs[256], f3 = bs[512];                                                   \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                  \
          bf16x8 n1, n2, n3;                                                                             \
          if (g < 7) {                                                                                   \
            const int o = ((g + 1) >> 2) * HP + ((g + 1) & 3) * 64;                                      \
            n1 = bs[o]; n2 = bs[o + 256]; n3 = bs[o + 512];                                              \
          }                                                                                              \
          /* smallest plane first; rows a and b alternate so that no pass waits for the one before it */   \
          part[2 * g + 0] = mma16<false>(f3, qa, part[2 * g + 0]);                                       \
          part[2 * g + 1] = mma16<false>(f3, qb, part[2 * g + 1]);                                       \
          part[2 * g + 0] = mma16<false>(f2, qa, part[2 * g + 0]);                                       \
          part[2 * g + 1] = mma16<false>(f2, qb, part[2 * g + 1]);                                       \
          part[2 * g + 0] = mma16<false>(f1, qa, part[2 * g + 0]);                                       \
          part[2 * g + 1] = mma16<false>(f1, qb, part[2 * g + 1]);                                       \
          if (g < 7) { f1 = n1; f2 = n2; f3 = n3; }                                                      \
        }                                                                                                \
        Bs[(buf_) ^ 1][tid] = UB0; Bs[(buf_) ^ 1][p1] = UB1; Bs[(buf_) ^ 1][p2] = UB2;                   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                               \
        __builtin_amdgcn_s_barrier();                                                                    \
        asm volatile("" ::: "memory");                                                                   \
      }
      for (int a = 0; a < aA; ++a) {
        const int ks = 4 * a, an = a + 1 < aA ? a + 1 : a;
        const int h = (ks0 + ks) / hsteps;
        const float cha = caA[h], chb = cbA[h];      // ga[t, h] of rows a / b: used at the head's last block only
#pragma unroll
        for (int s = 0; s < 4; ++s) { xa[s] = mka[ks0 + 4 * an + s]; xb[s] = mkb[ks0 + 4 * an + s]; }
        GA_STEP(ks, 0, ma[0], mb[0], sb0, sb1, sb2, tb0, tb1, tb2)
        GA_STEP(ks + 1, 1, ma[1], mb[1], tb0, tb1, tb2, sb0, sb1, sb2)
        GA_STEP(ks + 2, 0, ma[2], mb[2], sb0, sb1, sb2, tb0, tb1, tb2)
        GA_STEP(ks + 3, 1, ma[3], mb[3], tb0, tb1, tb2, sb0, sb1, sb2)
        if ((ks0 + ks + 4) % hsteps == 0) {
          // GA_FLUSH: acc += ga * (P + 0.01 (cs - P)) as  d = cs - P;  u = fma(0.01, d, P);  acc = fma(ga, u, acc),
          // each one rounding, in this order (P, cs and acc all carry this block's sign; 0.01f is LeakyReLU's slope)
          const float* cs = Cs + h * 128 + 4 * kg;
#pragma unroll
          for (int g = 0; g < 8; ++g) {
            const float4 c4 = *reinterpret_cast<const float4*>(cs + 16 * g);
            const float cv[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float pv = part[2 * g + nb][j];
                const float u = __fmaf_rn(0.01f, __fsub_rn(cv[j], pv), pv);
                acc[2 * g + nb][j] = __fmaf_rn(nb ? chb : cha, u, acc[2 * g + nb][j]);
              }
              part[2 * g + nb] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[i] = -acc[i]; part[i] = -part[i]; }
#pragma unroll
        for (int s = 0; s < 4; ++s) { ma[s] = xa[s]; mb[s] = xb[s]; }
      }
#undef GA_STEP
    }
  }
  const int kbeg = 4 * aA;                       // first k-step of the loop below (0 unless BP)
  bf16x8 qa1, qa2, qa3, qb1, qb2, qb3;           // current k-step's gZ fragments (rows a, b)
  bf16x8 na1, na2, na3, nb1, nb2, nb3;           // next k-step's
  if (!BP || kbeg < nk) {
    GE_ALOAD(kbeg, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m);
    GE_BLOAD(kbeg, sb0, sb1, sb2);
    GE_SPLIT(ra0, ra1, rca_c, rca_m, qa1, qa2, qa3);
    GE_SPLIT(rb0, rb1, rcb_c, rcb_m, qb1, qb2, qb3);
    GE_BSTORE(0);
    ra0 = ra1 = rb0 = rb1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (PASSES < 6) GE_BLOAD(kbeg + 1, sb0, sb1, sb2);   // nk >= 4
    GE_ALOAD(kbeg + 1, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m);
    __syncthreads();
  }

#define GE_MFMA1(F1_, F2_, F3_, Q1_, Q2_, Q3_, P_)                                                       \
  {                                                                                                      \
    if (PASSES >= 6) {                                                                                   \
      P_ = mma16<F16>(F3_, Q1_, P_);                                                                     \
      P_ = mma16<F16>(F1_, Q3_, P_);                                                                     \
      P_ = mma16<F16>(F2_, Q2_, P_);                                                                     \
    }                                                                                                    \
    if (!ONE) {                                                                                          \
      P_ = mma16<F16>(F2_, Q1_, P_);                                                                     \
      P_ = mma16<F16>(F1_, Q2_, P_);                                                                     \
    }                                                                                                    \
    P_ = mma16<F16>(F1_, Q1_, P_);                                                                       \
  }
  // One iteration: loads for k-step ks + 2 go into the (S, T) register sets, the (R, SB) sets -- loaded one iteration
  // ago -- are consumed.  The loop is unrolled by two with the sets swapped instead of copied: a register copy of an
  // in-flight load is a wait for it, and such copies at the loop end drained vmcnt every k-step.
#define GE_ITER(ks_, buf_, RA0, RA1, RB0, RB1, RCA, RCB, RMA, RMB, SA0, SA1, SB0, SB1, SCA, SCB, SMA, SMB,           \
                UB0, UB1, UB2, TB0, TB1, TB2)                                                            \
  {                                                                                                      \
    const bf16x8* bs = reinterpret_cast<const bf16x8*>(&Bs[buf_][lane]);                                 \
    /* no branches in the body (loads past the end re-fetch the last k-step, splits and stores of such tiles are */ \
    /* harmless): with conditional loads the compiler's wait-count bookkeeping turns conservative at every merge */ \
    const int kl_ = (ks_) + 2 < nk ? (ks_) + 2 : nk - 1;                                                 \
    if constexpr (PASSES >= 6) {   /* six-pass form: its three-plane tile one k-step ahead only (12 VGPRs less; */ \
      const int kb_ = (ks_) + 1 < nk ? (ks_) + 1 : nk - 1;   /* the loads sit in front of the operand loads, so the */ \
      GE_BLOAD(kb_, UB0, UB1, UB2);                          /* store's wait leaves those in flight) */     \
    } else {                                                                                             \
      GE_BLOAD(kl_, TB0, TB1, TB2);                                                                      \
    }                                                                                                    \
    GE_ALOAD(kl_, SA0, SA1, SB0, SB1, SCA, SCB, SMA, SMB);                                               \
    __builtin_amdgcn_sched_barrier(0);     /* the loads are ISSUED here, not where the scheduler likes them */ \
    /* the raw values in the R set belong to k-step ks + 1: split them while this step's MFMAs run */      \
    bf16x8 f1 = bs[0], f2, f3;                                                                           \
    if (!ONE) f2 = bs[256];                                                                              \
    if (PASSES >= 6) f3 = bs[512];                                                                       \
    _Pragma("unroll") for (int g = 0; g < 8; ++g) {      /* 16-column output block g = (half, cb) */        \
      bf16x8 n1, n2, n3;                                                                                 \
      if (g < 7) {                                                                                       \
        const int o = ((g + 1) >> 2) * HP + ((g + 1) & 3) * 64;                                          \
        n1 = bs[o];                                                                                      \
        if (!ONE) n2 = bs[o + 256];                                                                      \
        if (PASSES >= 6) n3 = bs[o + 512];                                                               \
      }                                                                                                  \
      GE_MFMA1(f1, f2, f3, qa1, qa2, qa3, acc[2 * g + 0]);                                               \
      if (g == 1) GE_SPLIT(RA0, RA1, RCA, RMA, na1, na2, na3);                                           \
      GE_MFMA1(f1, f2, f3, qb1, qb2, qb3, acc[2 * g + 1]);                                               \
      if (g == 4) GE_SPLIT(RB0, RB1, RCB, RMB, nb1, nb2, nb3);                                           \
      if (g < 7) { f1 = n1; f2 = n2; f3 = n3; }                                                          \
    }                                                                                                    \
    if (ONE) { Bs[(buf_) ^ 1][p0] = UB0; }                                                               \
    else { Bs[(buf_) ^ 1][tid] = UB0; Bs[(buf_) ^ 1][p1] = UB1; if (NP == 3) Bs[(buf_) ^ 1][p2] = UB2; } \
    /* LDS writes of this wave done, then the barrier -- NOT __syncthreads(): its fence also drains vmcnt, i.e. the */ \
    /* operand loads just issued two k-steps ahead */                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                   \
    __builtin_amdgcn_s_barrier();                                                                        \
    asm volatile("" ::: "memory");                                                                       \
    qa1 = na1; qa2 = na2; qa3 = na3; qb1 = nb1; qb2 = nb2; qb3 = nb3;                                    \
  }
  // One 128-column block of the operand (four k-steps) per trip.  The matrix instruction's accumulator rounds with a
  // sign-independent bias (-0.9e-9 ... -1.5e-9 of sum |g||w| on every output when all k-steps accumulated
  // with one sign, tools/f16_bias_probe.py): the weight planes of odd blocks are prepared NEGATED (edge_ge_launch) and
  // the accumulators change sign between blocks (exact), so a block's bias enters the result with the sign (-1)^a and
  // consecutive blocks cancel; after the last block the accumulators hold (-1)^ncb times the sum.
  for (int a = aA; a < ncb; ++a) {
    const int ks = 4 * a;
    GE_ITER(ks, 0, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m, sa0, sa1, sb0_, sb1_, sca_c, scb_c, sca_m, scb_m,
            sb0, sb1, sb2, tb0, tb1, tb2)
    GE_ITER(ks + 1, 1, sa0, sa1, sb0_, sb1_, sca_c, scb_c, sca_m, scb_m, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m,
            tb0, tb1, tb2, sb0, sb1, sb2)
    GE_ITER(ks + 2, 0, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m, sa0, sa1, sb0_, sb1_, sca_c, scb_c, sca_m, scb_m,
            sb0, sb1, sb2, tb0, tb1, tb2)
    GE_ITER(ks + 3, 1, sa0, sa1, sb0_, sb1_, sca_c, scb_c, sca_m, scb_m, ra0, ra1, rb0, rb1, rca_c, rcb_c, rca_m, rcb_m,
            tb0, tb1, tb2, sb0, sb1, sb2)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = -acc[i];
  }
#undef GE_ITER
#undef GE_BLOAD
#undef GE_BSTORE
#undef GE_ALOAD
#undef GE_SPLIT
#undef GE_MFMA1
  // acc[2 g + nb][j] = out[row(nb)][16 g + 4 kg + j]
  const long oa = scatter ? (long)scatter[rca] : rca, ob = scatter ? (long)scatter[rcb] : rcb;
  {
    const float fin = (F16 ? inv_all : 1.f) * ((ncb & 1) ? -1.f : 1.f);   // undo the scales (fp16 form) and the last sign
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = acc[i] * fin;
  }
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bias) bv = *reinterpret_cast<const float4*>(bias + 16 * g + 4 * kg);
    if (row_a < E) {
      const f32x4 v = acc[2 * g + 0];
      float4* o = reinterpret_cast<float4*>(out + oa * ldo + 16 * g + 4 * kg);
      float4 w = make_float4(v[0] + bv.x, v[1] + bv.y, v[2] + bv.z, v[3] + bv.w);
      if (accumulate) { const float4 u = *o; w.x += u.x; w.y += u.y; w.z += u.z; w.w += u.w; }
      *o = w;
    }
    if (row_b < E) {
      const f32x4 v = acc[2 * g + 1];
      float4* o = reinterpret_cast<float4*>(out + ob * ldo + 16 * g + 4 * kg);
      float4 w = make_float4(v[0] + bv.x, v[1] + bv.y, v[2] + bv.z, v[3] + bv.w);
      if (accumulate) { const float4 u = *o; w.x += u.x; w.y += u.y; w.z += u.z; w.w += u.w; }
      *o = w;
    }
  }
}

// ---------------------------------------------------------------------------------------
//     g_W_e[col, :] = sum_t gZ[t, col] * e[perm[t], :]           (edge_gw_kernel,  K = E, 1536 x 128 outputs)
// Both operands of this product are needed with t (the edge slot) as the MFMA's k index, i.e. transposed with
// respect to their [t][feature] storage:
//   * e[perm[t]] is pre-split ONCE per step into fragment-ordered planes (prepare_T_bf16 with a row gather:
//     operand (a = t/128, b = t%128, c = k) -- 0.77 GB at E = 1M, zero-padded past E) and streamed through a
//     double-buffered LDS tile shared by all waves of the workgroup;
//   * gZ tiles (32 slots x 128 columns = 16 KB contiguous in the blocked layout) are loaded coalesced, split in
//     registers, written as bf16 planes into an XOR-swizzled [32][128] LDS image and read back transposed with
//     ds_read_b64_tr_b16 (image (b) of cdna_hip_programming.md T10: conflict-free writes and transposed reads).
// A workgroup owns two 128-column blocks (8 waves x 32 columns, all 128 outputs k per wave: 64 accumulator
// VGPRs) and a contiguous range of k-steps; the workgroups of one range (one per column-block pair) are adjacent
// in the grid so that the e planes they share are fetched from HBM once and hit the Infinity Cache afterwards.
// Two-level summation through memory: every FLUSH k-steps (2048 slots) the accumulators are added into the
// workgroup's private slab tile and cleared; consecutive groups accumulate products of opposite sign (the split
// multiplies the raw gZ values by +-1), which cancels the bf16 MFMA's floor bias (bilinear.hip).  The slabs of
// all ranges are then summed in fixed order by splitk_reduce.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// BP (with RC, six passes: scalar attention in the 24-bit modes at Hd = 256; edge_gw_bitplane below): the ATTENTION half
// of the columns runs on the stored bit alone.  There gZ[t, (h, c)] = ga[t, h] wA[h, c] d, d = 1 or 0.01 by the bit m, so
// with the coefficient moved onto the OTHER operand, e'_h[t, :] = fl(ga[t, h] e[perm[t], :]),
//     g_W_e[(h, c), :] = wA[h, c] (P + 0.01 (cs_h - P)),   P[(h, c), :] = sum_t m[t, (h, c)] e'_h[t, :],   cs_h = sum_t e'_h[t, :].
// m is exact in ONE bf16 plane: P takes three passes (the planes of e') instead of six, the Gs image holds one plane of
// shifted bits -- no coefficient, no wA, no multiply, no split --, and wA and the 0.01 fold are applied once per output by
// the reducer (edge_gw_bit_reduce_kernel).  A head's 256 columns are one column-block pair, so an attention workgroup
// needs e' of ONE head: it builds the planes itself from 32 gathered fp32 rows of e per k-step (8 elements per thread)
// and writes them to Es in the order the MFMA loop reads; it does not read Eq.  cs_h: per-thread partial sums of the
// rounded e' (one per wave's slot quad and output), added to the workgroup's cs rows at every flush.
// One launch holds both halves: workgroups [0, S * message pairs) are the message pairs on S ranges (the body below,
// XCD-aware order as before), the SA * H behind them the attention pairs on SA longer ranges (same order: the H
// workgroups of a range share the gathered e rows from one L2).  SA : S follows the measured cost per k-step.
template <int PASSES, bool RC = false, bool BP = false>   // RC: the gZ tile is rebuilt from its ingredients (struct EdgeRC)
__global__ __launch_bounds__(512, 2) void edge_gw_kernel(const float* __restrict__ gZ, long ldg, long gzb,
                                                         const uint4* __restrict__ Eq, float* __restrict__ slab,
                                                         int E, int ncb, int nsteps, int S,
                                                         const float* __restrict__ gmax, const float* __restrict__ emax,
                                                         const EdgeRC rc, const float* __restrict__ erows, long lde,
                                                         const int* __restrict__ perm, int SA,
                                                         float* __restrict__ slabA, float* __restrict__ csl) {
  static_assert(!BP || (RC && PASSES == 6), "the bit-plane body belongs to the six-pass rebuilt form");
  // PASSES == 2: two fp16 planes, three passes; both operands are indexed by the reduction index (the edge slot), so
  // both scales are per tensor: gmax[0] = max |gZ| (from its producer), emax[0] = max |e| (the planes carry 2^k e)
  // PASSES == 1 (edge storage "bf16-mma"): one bf16 pass on the leading planes of both operands (see edge_ge_kernel)
  constexpr bool F16 = PASSES == 2;
  constexpr bool ONE = PASSES == 1;
  constexpr int NP = F16 ? 2 : 3;
  constexpr int HP = NP * 256;
  constexpr int FLUSH = 64;
  __shared__ uint4 Es[2][2 * HP];                        // e planes of one k-step: [half][plane][cb][lane]
  __shared__ __attribute__((aligned(16))) unsigned char Gs[2][2][NP][8192];   // [buffer][column block][plane][32 x 256 B]
  float sG = 1.f, inv_all = 1.f;
  if constexpr (F16) {
    float iG, sE, iE;
    pow2_scale(gmax[0], sG, iG);
    pow2_scale(emax[0], sE, iE);
    inv_all = iG * iE;
  }
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int grp = wave >> 2, wq = wave & 3;              // column block of the pair, 32-column slice in it
  const int cbA = BP ? rc.HHd / 128 : 0;                // BP: the attention half's column blocks are not this body's
  const int npair = (ncb - cbA) / 2;
  // XCD-aware order: consecutive workgroup ids go to different XCDs (own L2 each), and the npair workgroups of one range
  // read the same e planes.  The first 8 * floor(S / 8) ranges are dealt out so that a range's workgroups sit on ONE XCD,
  // next to each other in its dispatch order (the planes then come from HBM once and from that L2 afterwards; in plain
  // order every column-block pair fetched them into its own XCD: 6.5 GB of FETCH_SIZE for 0.77 GB of planes at
  // W2 = 1536); the remaining S % 8 ranges keep the plain order.  Same number of workgroups either way.
  int pair, split;
  const bool attn = BP && (int)blockIdx.x >= S * npair;  // (workgroup-uniform)
  {
    const int wg = attn ? blockIdx.x - S * npair : blockIdx.x;   // (a multiple of 8 apart or not: equal wg & 7 = one XCD)
    const int Sx = attn ? SA : S, np = attn ? rc.H : npair;
    const int s8 = Sx >> 3, body = 8 * s8 * np;
    if (wg < body) {
      const int xcd = wg & 7, j = wg >> 3;
      pair = j % np;
      split = xcd * s8 + j / np;
    } else {
      const int r = wg - body;
      pair = r % np;
      split = 8 * s8 + r / np;
    }
  }
  const int Sr = attn ? SA : S;                          // ranges this workgroup's half is dealt over
  // ranges in units of two k-steps (the loop is unrolled by two without a tail); a k-step past nsteps holds slots >= E,
  // which contribute zeros, and its e planes are the zero padding of the last 128-slot block
  const int npairs = (nsteps + 1) / 2;
  const int ks0 = 2 * (int)((long)npairs * split / Sr), ks1 = 2 * (int)((long)npairs * (split + 1) / Sr);
  const int cb128 = (attn ? 0 : cbA) + pair * 2 + grp;
  const float* gblk = gZ + (long)cb128 * gzb;
  const int gt = tid & 255;                              // thread within the column block's group
  // RC: this thread's four columns 128 cb128 + 4 (gt & 31) never change: head, half, mask word and bit offset are fixed
  const int rc_col = 128 * cb128 + 4 * (gt & 31);
  const bool rc_isA = RC && rc_col < rc.HHd;
  const int rc_cc = rc_isA ? rc_col : rc_col - rc.HHd;
  const int rc_h = RC ? rc_cc / rc.Hd : 0;
  const int rc_word = rc_col >> 5, rc_bit = rc_col & 31;
  const float* rc_coef = RC ? (rc_isA ? rc.ga : rc.alpha) + rc_h : nullptr;
  // (attention half: the "row" is the constant wA, fetched through the same load as a gS row -- selecting between a
  // register copy and a global pointer makes the compiler spill the copy and load it back through flat memory)
  const int last_row = E - 1;

  f32x4 acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  // (se*: the tile stored at the end of this iteration, loaded during the previous one; te*: the one after it)
  uint4 se0, se1, se2, te0, te1, te2;
  const int p1 = tid + 512, p2 = tid + 1024;
  const int p0 = tid < 256 ? tid : HP + tid - 256;      // ONE: where the thread's plane-0 piece lives in the tile
#define GW_ELOAD(ks_, E0_, E1_, E2_)                                                                     \
  {                                                                                                      \
    const long a_ = (ks_) >> 2, s_ = (ks_) & 3;                                                          \
    const uint4* h0 = Eq + ((a_ * 2 + 0) * 4 + s_) * HP;                                                 \
    const uint4* h1 = Eq + ((a_ * 2 + 1) * 4 + s_) * HP;                                                 \
    if (ONE) {                       /* plane 0 of each half: one piece per thread */                      \
      E0_ = tid < 256 ? h0[tid] : h1[tid - 256];                                                         \
    } else {                                                                                             \
      E0_ = h0[tid];                                                                                     \
      E1_ = p1 < HP ? h0[p1] : h1[p1 - HP];                                                              \
      if (NP == 3) E2_ = h1[p2 - HP];                                                                    \
    }                                                                                                    \
  }
  // raw gZ tile pieces: float4 number gt + 256 i of the k-step's contiguous [32][128] tile, i < 4
  float4 r0, r1, r2, r3, s0, s1, s2, s3;
  // RC: (coefficient, mask word) of the four rows in r* / s*, and the destination nodes of the rows one k-step further
  // (the row of gS is a dependent load: its index is fetched a k-step before the row itself)
  float rk0 = 0.f, rk1 = 0.f, rk2 = 0.f, rk3 = 0.f, sk0 = 0.f, sk1 = 0.f, sk2 = 0.f, sk3 = 0.f;
  unsigned rm0 = 0, rm1 = 0, rm2 = 0, rm3 = 0, sm0 = 0, sm1 = 0, sm2 = 0, sm3 = 0;
  int dn0 = 0, dn1 = 0, dn2 = 0, dn3 = 0;
#define GW_D1(ks_, i_, D_)                                                                               \
  {                                                                                                      \
    const long t = (long)(ks_) * 32 + ((gt + 256 * (i_)) >> 5);                                          \
    D_ = rc.dst[t < E ? t : last_row];                                                                   \
  }
  // (also in the attention half, where they are not used: no branches inside the loop body, see GW_ITER)
#define GW_DLOAD(ks_) { if constexpr (RC) { GW_D1(ks_, 0, dn0) GW_D1(ks_, 1, dn1) GW_D1(ks_, 2, dn2) GW_D1(ks_, 3, dn3) } }
  // row pointers of k-step ks_ from the dn* loaded for it (attention half: the constant wA -- through the same load,
  // because selecting between a register copy and a pointer makes the compiler keep the copy in scratch)
  const float *gp0 = nullptr, *gp1 = nullptr, *gp2 = nullptr, *gp3 = nullptr;
#define GW_PTRS()                                                                                        \
  {                                                                                                      \
    if constexpr (RC) {                                                                                  \
      gp0 = rc_isA ? rc.wA + rc_cc : rc.gS + (long)dn0 * rc.HHd + rc_cc;                                 \
      gp1 = rc_isA ? rc.wA + rc_cc : rc.gS + (long)dn1 * rc.HHd + rc_cc;                                 \
      gp2 = rc_isA ? rc.wA + rc_cc : rc.gS + (long)dn2 * rc.HHd + rc_cc;                                 \
      gp3 = rc_isA ? rc.wA + rc_cc : rc.gS + (long)dn3 * rc.HHd + rc_cc;                                 \
    }                                                                                                    \
  }
#define GW_G1(ks_, i_, R_, K_, M_, P_)                                                                   \
  {                                                                                                      \
    const int idx = gt + 256 * (i_);                                                                     \
    const long t = (long)(ks_) * 32 + (idx >> 5);                                                        \
    if constexpr (RC) {                                                                                  \
      const long tc = t < E ? t : last_row;                                                              \
      R_ = *reinterpret_cast<const float4*>(P_);                                                         \
      const float kk_ = rc_coef[tc * rc.H];              /* unconditional load, then the select */        \
      K_ = t < E ? kk_ : 0.f;                                                                            \
      M_ = rc.mask[tc * rc.nw + rc_word];                                                                \
    } else {                                                                                             \
      R_ = t < E ? *reinterpret_cast<const float4*>(gblk + t * ldg + 4 * (idx & 31))                     \
                 : make_float4(0.f, 0.f, 0.f, 0.f);                                                      \
    }                                                                                                    \
  }
  // Order inside one group of loads (vmcnt retires in order): the row indices of the k-step AFTER this one first --
  // they are needed (as addresses) at the top of the next iteration, and being the oldest of their group they can be
  // waited for with everything behind them still in flight --, then the e tile, then the rows themselves.
#define GW_LOADS(ks_, E0_, E1_, E2_, A_, B_, C_, D_, KA_, KB_, KC_, KD_, MA_, MB_, MC_, MD_)              \
  {                                                                                                      \
    GW_PTRS()                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    GW_DLOAD((ks_) + 1)                                                                                  \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
    GW_ELOAD(ks_, E0_, E1_, E2_);                                                                        \
    GW_G1(ks_, 0, A_, KA_, MA_, gp0) GW_G1(ks_, 1, B_, KB_, MB_, gp1)                                    \
    GW_G1(ks_, 2, C_, KC_, MC_, gp2) GW_G1(ks_, 3, D_, KD_, MD_, gp3)                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                   \
  }
  // split one float4 (row idx >> 5, columns 4 (idx & 31) ...) and store 8 bytes per plane into image (b)
#define GW_S1(i_, R_, K_, M_, buf_, sg_)                                                                 \
  {                                                                                                      \
    const int idx = gt + 256 * (i_);                                                                     \
    const int row = idx >> 5, c4 = idx & 31;                                                             \
    const int off = 256 * row + 16 * ((c4 >> 1) ^ (((row & 3) << 2) | ((row >> 2) & 3))) + 8 * (c4 & 1); \
    uint2 x1, x2, x3;                                                                                    \
    float4 g_ = R_;                                                                                      \
    if constexpr (RC) {   /* the stored value was (coefficient * vector) * d; the sign and the power-of-two scale */ \
      const unsigned mb_ = (M_) >> rc_bit;     /* of the split ride on the coefficient (exact) */           \
      const float ks_ = (K_) * (F16 ? (sg_) * sG : (sg_));                                                \
      /* __fmul_rn: the stored value was ROUNDED; contracted into the split's v - hi it would not be */   \
      g_.x = __fmul_rn(ks_ * g_.x, rc_d(mb_, 0)); g_.y = __fmul_rn(ks_ * g_.y, rc_d(mb_, 1));            \
      g_.z = __fmul_rn(ks_ * g_.z, rc_d(mb_, 2)); g_.w = __fmul_rn(ks_ * g_.w, rc_d(mb_, 3));            \
    }                                                                                                    \
    if constexpr (RC && F16) {                                                                           \
      split2_pair_f16(g_.x, g_.y, x1.x, x2.x);                                                           \
      split2_pair_f16(g_.z, g_.w, x1.y, x2.y);                                                           \
    } else if constexpr (RC) {                                                                           \
      split3_pair(g_.x, g_.y, x1.x, x2.x, x3.x);                                                         \
      split3_pair(g_.z, g_.w, x1.y, x2.y, x3.y);                                                         \
    } else if constexpr (F16) {                                                                          \
      const float m_ = (sg_) * sG;                                                                       \
      split2_pair_f16(g_.x * m_, g_.y * m_, x1.x, x2.x);                                                 \
      split2_pair_f16(g_.z * m_, g_.w * m_, x1.y, x2.y);                                                 \
    } else {                                                                                             \
      split3_pair(g_.x * sg_, g_.y * sg_, x1.x, x2.x, x3.x);                                             \
      split3_pair(g_.z * sg_, g_.w * sg_, x1.y, x2.y, x3.y);                                             \
    }                                                                                                    \
    *reinterpret_cast<uint2*>(&Gs[buf_][grp][0][off]) = x1;                                              \
    if (!ONE) *reinterpret_cast<uint2*>(&Gs[buf_][grp][1][off]) = x2;                                    \
    if (PASSES >= 6) *reinterpret_cast<uint2*>(&Gs[buf_][grp][NP - 1][off]) = x3;                        \
  }
  // transposed fragment of plane pl_, column block nb_ of this wave: k = 8 kg + j  <->  slot 8 kg + j
  const int l16q = n16 >> 2, l16p = n16 & 3;
#define GW_TRADDR(nb_, h_)                                                                               \
  ({                                                                                                     \
    const int row = 8 * kg + 4 * (h_) + l16q;                                                            \
    const int ch = 4 * wq + 2 * (nb_) + (l16p >> 1);                                                     \
    256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3))) + 8 * (l16p & 1);                      \
  })
  const int tr00 = GW_TRADDR(0, 0), tr01 = GW_TRADDR(0, 1), tr10 = GW_TRADDR(1, 0), tr11 = GW_TRADDR(1, 1);
#define GW_TRREAD(buf_, pl_, o0_, o1_)                                                                   \
  ({                                                                                                     \
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(&Gs[buf_][grp][pl_][o0_]));   \
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(&Gs[buf_][grp][pl_][o1_]));   \
    typedef short s16x8 __attribute__((ext_vector_type(8)));                                             \
    const s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                         \
    __builtin_bit_cast(bf16x8, both);                                                                    \
  })
#define GW_MFMA1(F1_, F2_, F3_, Q1_, Q2_, Q3_, P_)                                                       \
  {                                                                                                      \
    if (PASSES >= 6) {                                                                                   \
      P_ = mma16<F16>(F3_, Q1_, P_);                                                                     \
      P_ = mma16<F16>(F1_, Q3_, P_);                                                                     \
      P_ = mma16<F16>(F2_, Q2_, P_);                                                                     \
    }                                                                                                    \
    if (!ONE) {                                                                                          \
      P_ = mma16<F16>(F2_, Q1_, P_);                                                                     \
      P_ = mma16<F16>(F1_, Q2_, P_);                                                                     \
    }                                                                                                    \
    P_ = mma16<F16>(F1_, Q1_, P_);                                                                       \
  }
  // the workgroup's slab tile: rows = its 256 columns of gZ, 128 outputs each
  // (BP: message slabs hold the message columns only, [S][W2 - HHd][128]; attention slabs [SA][HHd][128] at slabA)
  float* tile = attn ? slabA + ((long)split * cbA * 128 + (long)cb128 * 128 + 32 * wq) * 128
                     : slab + ((long)split * (ncb - cbA) * 128 + (long)(cb128 - cbA) * 128 + 32 * wq) * 128;
#define GW_FLUSH(first_, sg_)                                                                            \
  {                                                                                                      \
    _Pragma("unroll") for (int g = 0; g < 8; ++g)                                                        \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                                   \
      float4* o = reinterpret_cast<float4*>(tile + (long)(16 * nb + n16) * 128 + 16 * g + 4 * kg);       \
      const f32x4 v = acc[2 * g + nb];                                                                   \
      const float fs_ = F16 ? (sg_) * inv_all : (sg_);                                                   \
      float4 w = make_float4(v[0] * fs_, v[1] * fs_, v[2] * fs_, v[3] * fs_);                            \
      if (!(first_)) { const float4 u = *o; w.x += u.x; w.y += u.y; w.z += u.z; w.w += u.w; }            \
      *o = w;                                                                                            \
      acc[2 * g + nb] = f32x4{0.f, 0.f, 0.f, 0.f};                                                       \
    }                                                                                                    \
  }
  if constexpr (BP) {
    if (attn) {
      // e' role: thread (op, sq) holds outputs op and op + 64 of the k-step's slots 4 sq ... 4 sq + 3 (a wave's loads
      // cover 256 contiguous bytes of one gathered row; its coefficient and row index are wave-uniform)
      const int op = tid & 63, sq = wave, head = pair;
      unsigned char* const esb = reinterpret_cast<unsigned char*>(&Es[0][0]) +
                                 16 * ((op >> 4) * 64 + (sq >> 1) * 16 + (op & 15)) + 8 * (sq & 1);
      // bit role: thread (slot, word, half) expands 16 bits of the head's eight mask words of one slot
      const int gslot = tid >> 4, gw = (tid >> 1) & 7, ghs = tid & 1, ggrp = gw >> 2;
      const int gch = 4 * (gw & 3) + 2 * ghs, gsw = ((gslot & 3) << 2) | ((gslot >> 2) & 3);
      const int goff0 = 256 * gslot + 16 * (gch ^ gsw), goff1 = 256 * gslot + 16 * ((gch + 1) ^ gsw);
      const unsigned* mbase = rc.mask + head * 8 + gw;
      const float* kbase = rc.ga + head;
      float* csrow = csl + (((long)split * rc.H + head) * 8 + sq) * 128 + op;
      // (pe*: the sums of the k-step split LAST -- it is multiplied one iteration later and may open the next flush group)
      float cs0 = 0.f, cs1 = 0.f, pe0 = 0.f, pe1 = 0.f;
      if (ks1 <= ks0) {   // empty range: the reducer still sums this slab and these cs rows
        GW_FLUSH(true, 1.f);
        csrow[0] = 0.f; csrow[64] = 0.f;
        return;
      }
      int pn0 = 0, pn1 = 0, pn2 = 0, pn3 = 0;            // rows of e for the k-step after the one being loaded
      float rv[8], sv[8], rk[4], sk[4];                  // raw e values / coefficients: next k-step's, the one after
      unsigned rm = 0, sm = 0;
#define AT_D1(ks_, j_, D_)                                                                               \
      {                                                                                                  \
        const long t = (long)(ks_) * 32 + 4 * sq + (j_);                                                 \
        D_ = perm[t < E ? t : last_row];                                                                 \
      }
#define AT_DLOAD(ks_) { AT_D1(ks_, 0, pn0) AT_D1(ks_, 1, pn1) AT_D1(ks_, 2, pn2) AT_D1(ks_, 3, pn3) }
#define AT_K1(ks_, j_, K_)                                                                               \
      {                                                                                                  \
        const long t = (long)(ks_) * 32 + 4 * sq + (j_);                                                 \
        const float kk_ = kbase[(t < E ? t : last_row) * rc.H];   /* unconditional load, then the select */ \
        K_[j_] = t < E ? kk_ : 0.f;                                                                      \
      }
      // same order inside one group of loads as GW_LOADS below: the row indices of the k-step AFTER this one first
#define AT_LOADS(ks_, V_, K_, M_)                                                                        \
      {                                                                                                  \
        const float* q0 = erows + (long)pn0 * lde + op;                                                  \
        const float* q1 = erows + (long)pn1 * lde + op;                                                  \
        const float* q2 = erows + (long)pn2 * lde + op;                                                  \
        const float* q3 = erows + (long)pn3 * lde + op;                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        AT_DLOAD((ks_) + 1)                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                                               \
        V_[0] = q0[0]; V_[1] = q0[64]; V_[2] = q1[0]; V_[3] = q1[64];                                    \
        V_[4] = q2[0]; V_[5] = q2[64]; V_[6] = q3[0]; V_[7] = q3[64];                                    \
        AT_K1(ks_, 0, K_) AT_K1(ks_, 1, K_) AT_K1(ks_, 2, K_) AT_K1(ks_, 3, K_)                          \
        {                                                                                                \
          const long t = (long)(ks_) * 32 + gslot;                                                       \
          M_ = mbase[(t < E ? t : last_row) * rc.nw];                                                    \
        }                                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                               \
      }
      // e' = fl(+-ga e) (the flush group's sign rides on the coefficient: exact), its column sum, its three planes:
      // 8 bytes (four slots) per plane and output into the fragment-ordered tile
#define AT_SPLIT_E(V_, K_, buf_, sg_)                                                                    \
      {                                                                                                  \
        float v_[8];                                                                                     \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_) {                                               \
          const float k_ = K_[j_] * (sg_);                                                               \
          v_[2 * j_] = __fmul_rn(k_, V_[2 * j_]); v_[2 * j_ + 1] = __fmul_rn(k_, V_[2 * j_ + 1]);        \
        }                                                                                                \
        pe0 = __fadd_rn(__fadd_rn(v_[0], v_[2]), __fadd_rn(v_[4], v_[6]));                               \
        pe1 = __fadd_rn(__fadd_rn(v_[1], v_[3]), __fadd_rn(v_[5], v_[7]));                               \
        uint2 a1, a2, a3, b1, b2, b3;                                                                    \
        split3_pair(v_[0], v_[2], a1.x, a2.x, a3.x); split3_pair(v_[4], v_[6], a1.y, a2.y, a3.y);        \
        split3_pair(v_[1], v_[3], b1.x, b2.x, b3.x); split3_pair(v_[5], v_[7], b1.y, b2.y, b3.y);        \
        unsigned char* d_ = esb + (buf_) * (2 * HP * 16);                                                \
        *reinterpret_cast<uint2*>(d_) = a1;                                                              \
        *reinterpret_cast<uint2*>(d_ + 4096) = a2;                                                       \
        *reinterpret_cast<uint2*>(d_ + 8192) = a3;                                                       \
        *reinterpret_cast<uint2*>(d_ + HP * 16) = b1;                                                    \
        *reinterpret_cast<uint2*>(d_ + HP * 16 + 4096) = b2;                                             \
        *reinterpret_cast<uint2*>(d_ + HP * 16 + 8192) = b3;                                             \
      }
#define AT_SPLIT_G(M_, buf_)                                                                             \
      {                                                                                                  \
        const unsigned mb_ = (M_) >> (16 * ghs);                                                         \
        *reinterpret_cast<uint4*>(&Gs[buf_][ggrp][0][goff0]) = __builtin_bit_cast(uint4, bits8_bf16(mb_));      \
        *reinterpret_cast<uint4*>(&Gs[buf_][ggrp][0][goff1]) = __builtin_bit_cast(uint4, bits8_bf16(mb_ >> 8)); \
      }
      AT_DLOAD(ks0);
      AT_LOADS(ks0, rv, rk, rm);
      AT_SPLIT_E(rv, rk, 0, 1.f)
      AT_SPLIT_G(rm, 0)
      AT_LOADS(ks0 + 1, rv, rk, rm);                     // ranges are even
      __syncthreads();
      bool firstA = true;
      // the pipeline of GW_ITER below: loads of k-step ks + 2 into the S set, the R set split into the other buffer
#define AT_ITER(ks_, buf_, RV, RK, RM, SV, SK, SM)                                                       \
      {                                                                                                  \
        const int rel = (ks_) - ks0;                                                                     \
        const float sgn_next = (((rel + 1) / FLUSH) & 1) ? -1.f : 1.f;                                   \
        const int kl_ = (ks_) + 2 < ks1 ? (ks_) + 2 : ks1 - 1;                                           \
        AT_LOADS(kl_, SV, SK, SM);                                                                       \
        cs0 = __fadd_rn(cs0, pe0); cs1 = __fadd_rn(cs1, pe1);        /* this k-step's e' */                \
        const bf16x8* es = reinterpret_cast<const bf16x8*>(&Es[buf_][lane]);                             \
        const bf16x8 qa = GW_TRREAD(buf_, 0, tr00, tr01), qb = GW_TRREAD(buf_, 0, tr10, tr11);           \
        bf16x8 f1 = es[0], f2 = es[256], f3 = es[512];                                                   \
        _Pragma("unroll") for (int g = 0; g < 8; ++g) {                                                  \
          bf16x8 n1, n2, n3;                                                                             \
          if (g < 7) {                                                                                   \
            const int o = ((g + 1) >> 2) * HP + ((g + 1) & 3) * 64;                                      \
            n1 = es[o]; n2 = es[o + 256]; n3 = es[o + 512];                                              \
          }                                                                                              \
          /* smallest plane first; columns a and b alternate so that no pass waits for the one before it */ \
          acc[2 * g + 0] = mma16<false>(f3, qa, acc[2 * g + 0]);                                         \
          acc[2 * g + 1] = mma16<false>(f3, qb, acc[2 * g + 1]);                                         \
          acc[2 * g + 0] = mma16<false>(f2, qa, acc[2 * g + 0]);                                         \
          acc[2 * g + 1] = mma16<false>(f2, qb, acc[2 * g + 1]);                                         \
          acc[2 * g + 0] = mma16<false>(f1, qa, acc[2 * g + 0]);                                         \
          acc[2 * g + 1] = mma16<false>(f1, qb, acc[2 * g + 1]);                                         \
          if (g == 1) AT_SPLIT_E(RV, RK, (buf_) ^ 1, sgn_next)                                           \
          if (g == 4) AT_SPLIT_G(RM, (buf_) ^ 1)                                                         \
          if (g < 7) { f1 = n1; f2 = n2; f3 = n3; }                                                      \
        }                                                                                                \
        if ((rel + 1) % FLUSH == 0 || (ks_) + 1 == ks1) {                                                \
          const float sg = ((rel / FLUSH) & 1) ? -1.f : 1.f;                                             \
          GW_FLUSH(firstA, sg);                                                                          \
          float c0 = cs0 * sg, c1 = cs1 * sg;                                                            \
          if (!firstA) { c0 = __fadd_rn(c0, csrow[0]); c1 = __fadd_rn(c1, csrow[64]); }                  \
          csrow[0] = c0; csrow[64] = c1;                                                                 \
          cs0 = cs1 = 0.f;                                                                               \
          firstA = false;                                                                                \
        }                                                                                                \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                               \
        __builtin_amdgcn_s_barrier();                                                                    \
        asm volatile("" ::: "memory");                                                                   \
      }
      for (int ks = ks0; ks < ks1; ks += 2) {
        AT_ITER(ks, 0, rv, rk, rm, sv, sk, sm)
        AT_ITER(ks + 1, 1, sv, sk, sm, rv, rk, rm)
      }
#undef AT_ITER
#undef AT_SPLIT_G
#undef AT_SPLIT_E
#undef AT_LOADS
#undef AT_K1
#undef AT_DLOAD
#undef AT_D1
      return;
    }
  }
  if (ks1 <= ks0) {   // empty range: the reducer still sums this slab
    GW_FLUSH(true, 1.f);
    return;
  }
  GW_DLOAD(ks0);
  GW_LOADS(ks0, se0, se1, se2, r0, r1, r2, r3, rk0, rk1, rk2, rk3, rm0, rm1, rm2, rm3);
  if (ONE) { Es[0][p0] = se0; }
  else {
    Es[0][tid] = se0; Es[0][p1] = se1;
    if (NP == 3) Es[0][p2] = se2;
  }
  GW_S1(0, r0, rk0, rm0, 0, 1.f) GW_S1(1, r1, rk1, rm1, 0, 1.f) GW_S1(2, r2, rk2, rm2, 0, 1.f) GW_S1(3, r3, rk3, rm3, 0, 1.f)
  r0 = r1 = r2 = r3 = make_float4(0.f, 0.f, 0.f, 0.f);
  rk0 = rk1 = rk2 = rk3 = 0.f;
  GW_LOADS(ks0 + 1, se0, se1, se2, r0, r1, r2, r3, rk0, rk1, rk2, rk3, rm0, rm1, rm2, rm3);   // ranges are even
  __syncthreads();
  bool first = true;
  // One iteration: the loads of k-step ks + 2 go into the (S, TE) register sets, the (R, UE) sets -- loaded one iteration
  // ago -- are consumed.  Unrolled by two with the sets swapped instead of copied: a register copy of an in-flight load
  // is a wait for it, and such copies at the loop end drained vmcnt every k-step.
#define GW_ITER(ks_, buf_, R0, R1, R2, R3, RK0, RK1, RK2, RK3, RM0, RM1, RM2, RM3,                           \
                S0, S1, S2, S3, SK0, SK1, SK2, SK3, SM0, SM1, SM2, SM3, UE0, UE1, UE2, TE0, TE1, TE2)    \
  {                                                                                                      \
    const int rel = (ks_) - ks0;                                                                         \
    /* sign of the flush group the NEXT k-step belongs to (its tile is split during this iteration) */     \
    const float sgn_next = (((rel + 1) / FLUSH) & 1) ? -1.f : 1.f;                                       \
    /* no branches around the loads (past the range: the last k-step again, never used): with conditional loads */ \
    /* the compiler's wait-count bookkeeping turns conservative at every merge */                         \
    const int kl_ = (ks_) + 2 < ks1 ? (ks_) + 2 : ks1 - 1;                                               \
    GW_LOADS(kl_, TE0, TE1, TE2, S0, S1, S2, S3, SK0, SK1, SK2, SK3, SM0, SM1, SM2, SM3);                \
    const bf16x8* es = reinterpret_cast<const bf16x8*>(&Es[buf_][lane]);                                 \
    /* this wave's two transposed gZ fragments (32 columns x 32 slots), three planes each */               \
    bf16x8 qa1 = GW_TRREAD(buf_, 0, tr00, tr01), qa2, qa3;                                               \
    bf16x8 qb1 = GW_TRREAD(buf_, 0, tr10, tr11), qb2, qb3;                                               \
    if (!ONE) { qa2 = GW_TRREAD(buf_, 1, tr00, tr01); qb2 = GW_TRREAD(buf_, 1, tr10, tr11); }            \
    if (PASSES >= 6) { qa3 = GW_TRREAD(buf_, 2, tr00, tr01); qb3 = GW_TRREAD(buf_, 2, tr10, tr11); }     \
    bf16x8 f1 = es[0], f2, f3;                                                                           \
    if (!ONE) f2 = es[256];                                                                              \
    if (PASSES >= 6) f3 = es[512];                                                                       \
    _Pragma("unroll") for (int g = 0; g < 8; ++g) {      /* 16 outputs k = 16 g ...: e fragment g = (half, cb) */ \
      bf16x8 n1, n2, n3;                                                                                 \
      if (g < 7) {                                                                                       \
        const int o = ((g + 1) >> 2) * HP + ((g + 1) & 3) * 64;                                          \
        n1 = es[o];                                                                                      \
        if (!ONE) n2 = es[o + 256];                                                                      \
        if (PASSES >= 6) n3 = es[o + 512];                                                               \
      }                                                                                                  \
      GW_MFMA1(f1, f2, f3, qa1, qa2, qa3, acc[2 * g + 0]);                                               \
      if (g == 0) GW_S1(0, R0, RK0, RM0, (buf_) ^ 1, sgn_next)                                           \
      if (g == 2) GW_S1(1, R1, RK1, RM1, (buf_) ^ 1, sgn_next)                                           \
      if (g == 4) GW_S1(2, R2, RK2, RM2, (buf_) ^ 1, sgn_next)                                           \
      if (g == 6) GW_S1(3, R3, RK3, RM3, (buf_) ^ 1, sgn_next)                                           \
      GW_MFMA1(f1, f2, f3, qb1, qb2, qb3, acc[2 * g + 1]);                                               \
      if (g < 7) { f1 = n1; f2 = n2; f3 = n3; }                                                          \
    }                                                                                                    \
    if (ONE) { Es[(buf_) ^ 1][p0] = UE0; }                                                               \
    else { Es[(buf_) ^ 1][tid] = UE0; Es[(buf_) ^ 1][p1] = UE1; if (NP == 3) Es[(buf_) ^ 1][p2] = UE2; } \
    if ((rel + 1) % FLUSH == 0 || (ks_) + 1 == ks1) {                                                    \
      const float sg = ((rel / FLUSH) & 1) ? -1.f : 1.f;                                                 \
      GW_FLUSH(first, sg);                                                                               \
      first = false;                                                                                     \
    }                                                                                                    \
    /* LDS writes of this wave done, then the barrier -- NOT __syncthreads(): its fence also drains vmcnt, i.e. the */ \
    /* operand loads just issued two k-steps ahead */                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                   \
    __builtin_amdgcn_s_barrier();                                                                        \
    asm volatile("" ::: "memory");                                                                       \
  }
  for (int ks = ks0; ks < ks1; ks += 2) {
    GW_ITER(ks, 0, r0, r1, r2, r3, rk0, rk1, rk2, rk3, rm0, rm1, rm2, rm3,
            s0, s1, s2, s3, sk0, sk1, sk2, sk3, sm0, sm1, sm2, sm3, se0, se1, se2, te0, te1, te2)
    GW_ITER(ks + 1, 1, s0, s1, s2, s3, sk0, sk1, sk2, sk3, sm0, sm1, sm2, sm3,
            r0, r1, r2, r3, rk0, rk1, rk2, rk3, rm0, rm1, rm2, rm3, te0, te1, te2, se0, se1, se2)
  }
#undef GW_ITER
#undef GW_LOADS
#undef GW_PTRS
#undef GW_ELOAD
#undef GW_G1
#undef GW_D1
#undef GW_DLOAD
#undef GW_S1
#undef GW_TRADDR
#undef GW_TRREAD
#undef GW_MFMA1
#undef GW_FLUSH
}

// =======================================================================================
// Launchers.  Every launch takes its operands as one record (kernels.h), asks edge_ge_form / edge_gw_form ONCE which kernel
// runs on which image, grid and workspace carve, and hands record and form to the one function that expands them into that
// kernel's argument list.
// =======================================================================================
// Every instantiation of the two kernels.  First use decides the order in which the device code is emitted; naming them
// here, in the order they have always had, keeps the code object byte-identical whatever order the launchers below take.
[[maybe_unused]] static const void* const k_instantiations[] = {
    (const void*)edge_ge_kernel<6, true, true>, (const void*)edge_ge_kernel<1, true>, (const void*)edge_ge_kernel<2, true>,
    (const void*)edge_ge_kernel<6, true>, (const void*)edge_ge_kernel<3, true>, (const void*)edge_ge_kernel<2, false>,
    (const void*)edge_ge_kernel<6, false>, (const void*)edge_ge_kernel<3, false>,
    (const void*)edge_gw_kernel<6, true, true>, (const void*)edge_gw_kernel<1, true>, (const void*)edge_gw_kernel<2, true>,
    (const void*)edge_gw_kernel<6, true>, (const void*)edge_gw_kernel<3, true>, (const void*)edge_gw_kernel<2, false>,
    (const void*)edge_gw_kernel<6, false>, (const void*)edge_gw_kernel<3, false>};

// ---- edge_ge: the parts of the decision, then the decision ----
// The rebuilt rows take the bit-plane body (edge_ge_kernel<6, true, true>) in the 24-bit modes when the attention half is
// whole heads of whole 128-column blocks (at most 8: the kernel's LDS copy of cs) and a launch group of ncb_g column
// blocks starts at a head's first block (a group that is the whole row always does).
static bool edge_ge_bitplane(const EdgeRC* rc, int W2, int ncb_g) {
  return rc && mode_24bit() && !edge_mma_bf16() && rc->H >= 1 && rc->H <= 8 && rc->Hd % 128 == 0 &&
         rc->HHd == rc->H * rc->Hd && rc->HHd <= W2 && rc->nw * 32 == W2 && (ncb_g * 128) % rc->Hd == 0;
}
bool edge_ge_dims(int Ce, int W2, long ldg, long gzb, long ldo) {
  return mode_split() && Ce == 128 && W2 % 128 == 0 && gzb != 0 && (gzb % 4) == 0 && (ldg % 4) == 0 && (ldo % 4) == 0;
}
// (the six-pass image is the larger one: three bf16 planes per 128 x 128 block)
size_t edge_ge_heads_image_floats(int W2) { return (size_t)(W2 / 128) * 24576 + 4; }
bool edge_ge_heads_dims(int heads, int W2, long ldx, long ldy, long ldw, bool have_amax) {
  const bool f16 = mode_f16() && have_amax;
  const bool six = mode_24bit();      // round 6: the 24-bit modes batch their heads too
  return (f16 || six) && heads >= 1 && heads <= TPREP_MAX && W2 % 128 == 0 && ldw == W2 && edge_ge_dims(128, W2, ldx, 128, ldy);
}
// K-split form for FEW row tiles beside a long K (round 6; the harness' shipped batch: g_edge_attr at 30 720 edges is 120
// workgroups walking 20 column blocks, the node-side input gradients at 1 280 atoms 5 workgroups -- or, as small-row
// programs, 0.84 GFLOP on the fp64 matrix instruction: 100-160 us a launch).  The column blocks are dealt to S groups
// (grid.y), group s multiplies its blocks into slab s; the caller adds the slabs in group order (sum_slabs_launch).  A group
// holds an EVEN number of blocks, so that a block's position in its group has the parity of its position in the row (the
// sign alternation above).  The groups have six-pass bodies only: none for rebuilt rows under "bf16-mma", which run one pass.
// Returns the number of groups a launch of this shape takes; 1 = not worth it / not available (then the plain launch).
int edge_ge_ksplit_groups(int E, int W2, bool rebuilt) {
  if (!mode_24bit() || (rebuilt && edge_mma_bf16())) return 1;
  const int ncb = W2 / 128, tiles = cdiv(E, 256);
  if (W2 % 128 != 0 || E < 1024 || tiles >= 192) return 1;     // (the reference's fixtures stay on the unsplit forms)
  int best = 1;
  for (int S = 2; S <= ncb; ++S)
    if (ncb % S == 0 && ((ncb / S) & 1) == 0) { best = S; if (tiles * S >= 192) break; }
  return best;
}

// The form of an edge_ge_launch, by the kind of its record:
//   * the heads launch (heads > 0): grid.y = head; two fp16 planes in the f16x3 mode (max |x| known: edge_ge_heads_dims),
//     the six-pass image otherwise, either prepared for all heads at once;
//   * a prepared image (We == null): the six-pass kernel on the caller's image -- the per-node second layer of the message
//     network, whose H per-head weights are not one affine operand (layers.hip);
//   * else the f16x3 form with max |rows| known, for a weight whose 128 outputs are contiguous (s_out == 1: the backward
//     products) or whose W2 inputs are (s_col == 1: a forward nn.Linear weight [128, W2], round 3); the bit-plane body
//     where edge_ge_bitplane holds for the launch's K groups (groups that start inside a head keep the six-pass body); ONE
//     bf16 pass for the per-EDGE launch under "bf16-mma" (rc: the rebuilt rows -- and never in the fp16 mode, which has its
//     own bf16 storage form); else six passes, three in the bf16x3 mode.
EdgeGeForm edge_ge_form(const EdgeGeParams& p) {
  EdgeGeForm f = {};
  if (p.rows <= 0) return f;
  const int ncb = p.W2 / 128;
  f.grid_x = cdiv(p.rows, 256);
  f.groups = 1; f.ncb_g = ncb;
  if (p.heads > 0) {
    f.heads = p.heads;
    f.passes = mode_f16() ? 2 : 6;
    f.prep = mode_f16() ? GE_PREP_HEADS_F16 : GE_PREP_PLANES;
    return f;
  }
  if (!p.We) { f.passes = 6; f.prep = GE_PREP_NONE; return f; }
  if (p.slabs) { f.groups = p.S; f.ncb_g = p.S >= 1 ? ncb / p.S : 0; }
  const bool out_contig = p.s_out == 1 && (p.s_col % 4) == 0, in_contig = p.s_col == 1 && (p.s_out % 4) == 0 && p.W2 % 128 == 0;
  const bool f16 = mode_f16() && p.amax && (out_contig || in_contig) && aligned16(p.We);
  f.rc = p.rc != nullptr;
  f.bitplane = !f16 && edge_ge_bitplane(p.rc, p.W2, f.ncb_g);
  const bool one = f.rc && !f16 && edge_mma_bf16() && !mode_bf16x3();
  f.passes = f.bitplane ? 6 : one ? 1 : f16 ? 2 : mode_bf16x3() ? 3 : 6;
  f.prep = f16 ? GE_PREP_F16_TMAX : f.bitplane ? GE_PREP_ATTN : GE_PREP_PLANES;
  return f;
}
// what edge_ge_launch refuses, given the form it would run
static int edge_ge_check(const EdgeGeParams& p, const EdgeGeForm& f) {
  CGAT_CHECK_ARG(!p.slabs || (f.groups >= 1 && f.groups * f.ncb_g == p.W2 / 128 && (f.groups == 1 || (f.ncb_g & 1) == 0) &&
                              mode_24bit()),
                 "edge_ge_ksplit: %d groups of %d column blocks", p.S, p.W2 / 128);
  return CGAT_OK;
}

// ---- edge_ge_kernel's argument list, expanded here and nowhere else ----
// grid.y = the form's K groups or heads, whose operands lie hb apart
static void edge_ge_go(const EdgeGeForm& f, const EdgeGeParams& p, const HeadBatch& hb, hipStream_t stream) {
  EdgeRC rcv = {};
  if (f.rc) { rcv = *p.rc; rcv.cs = p.Wq + edge_ge_cs_offset(p.W2); }   // (cs: where GE_PREP_ATTN leaves the column sums)
  const dim3 grid(f.grid_x, f.heads > 0 ? f.heads : f.groups);
#define GE_GO(P_, R_, B_)                                                                                             \
  hipLaunchKernelGGL((edge_ge_kernel<P_, R_, B_>), grid, dim3(512), 0, stream, p.gZ, p.ldg, p.gzb, (const uint4*)p.Wq,  \
                     f.ncb_g, p.out, p.ldo, p.scatter, p.rows, p.accumulate, p.bias, p.amax, rcv, hb)
  if (f.bitplane) GE_GO(6, true, true);
  else if (f.passes == 1) GE_GO(1, true, false);
  else if (f.rc) { if (f.passes == 2) GE_GO(2, true, false); else if (f.passes == 6) GE_GO(6, true, false); else GE_GO(3, true, false); }
  else { if (f.passes == 2) GE_GO(2, false, false); else if (f.passes == 6) GE_GO(6, false, false); else GE_GO(3, false, false); }
#undef GE_GO
}

int edge_ge_launch(const EdgeGeParams& p0, hipStream_t stream) {
  if (p0.rows <= 0) return CGAT_OK;
  const EdgeGeForm f = edge_ge_form(p0);
  CGAT_TRY(edge_ge_check(p0, f));
  EdgeGeParams p = p0;
  const int ncb = p.W2 / 128;
  const long img = (long)edge_ge_heads_image_floats(p.W2);
  HeadBatch hb = {};
  if (f.heads > 0) hb = {p.s_x, img / 4, p.s_bias, p.s_y, 0};
  if (p.slabs) {   // the slabs are the output: group s walks its ncb_g blocks from k-step ks0 into slab s
    p.out = p.slabs; p.ldo = 128; p.accumulate = 0; p.bias = nullptr; p.amax = nullptr;
    hb = {(long)f.ncb_g * p.gzb, (long)f.ncb_g * 6144, 0, (long)p.rows * 128, 0, 0, (long)f.ncb_g * 4};
  }
  // operand (a = column block, b = column in block, c = output k) = We[(128 a + b) * s_col + c * s_out]
  switch (f.prep) {
    case GE_PREP_NONE: break;
    case GE_PREP_PLANES:
      CGAT_TRY(prepare_T_planes_launch(p.We, p.Wq, ncb, 128 * p.s_col, p.s_col, p.s_out, /*alternate=*/1, stream, nullptr,
                                       f.heads > 0 ? f.heads : 1, p.s_w, f.heads > 0 ? img : 0));
      break;
    case GE_PREP_F16_TMAX: {   // per-tensor weight scale: max |We| behind the two planes
      float* wmax = p.Wq + (size_t)ncb * 16384;
      CGAT_TRY(fill_launch(wmax, 0.f, 1, stream));
      if (p.s_out == 1) CGAT_TRY(absmax_rows128_launch(p.We, p.s_col, p.W2, wmax, stream));
      else
        for (int j = 0; j < ncb; ++j) CGAT_TRY(absmax_rows128_launch(p.We + 128 * j, p.s_out, 128, wmax, stream));
      CGAT_TRY(prepare_T_planes_launch(p.We, p.Wq, ncb, 128 * p.s_col, p.s_col, p.s_out, /*alternate=*/1, stream, wmax));
      break;
    }
    case GE_PREP_ATTN:
      CGAT_TRY(prepare_T_bf16_attn_launch(p.We, p.Wq, ncb, 128 * p.s_col, p.s_col, p.s_out, p.rc->wA, p.rc->H, p.rc->Hd,
                                          p.Wq + edge_ge_cs_offset(p.W2), stream));
      break;
    case GE_PREP_HEADS_F16: {   // source dims (k, a, b) of W_h[c * W2 + 128 a + b]; the partial maxima behind the images
      const float* src[TPREP_MAX];
      float* dst[TPREP_MAX];
      for (int h = 0; h < f.heads; ++h) { src[h] = p.We + (long)h * p.s_w; dst[h] = p.Wq + (size_t)h * img; }
      CGAT_TRY(bilinear_prepare_T_batch(f.heads, src, dst, 128, ncb, 128, 1, 2, 0, p.Wq + (size_t)f.heads * img, stream,
                                        /*alternate=*/1));
      break;
    }
  }
  CGAT_PROF(p.scatter ? "edge_ge" : "rows_ge", stream);   // the per-edge launch / node-side and dense-layer uses
  edge_ge_go(f, p, hb, stream);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// ---- edge_gw: the parts of the decision, then the decision ----
bool edge_gw_dims(int Ce, int W2, long ldg, long gzb) {
  return mode_split() && Ce == 128 && W2 % 256 == 0 && gzb != 0 && (gzb % 4) == 0 && (ldg % 4) == 0;
}
static int edge_gw_splits(int W2) {   // ranges x column-block pairs ~ one workgroup per CU
  const int npair = W2 / 256;
  if (npair <= 0) return 1;
  return 256 / npair > 0 ? 256 / npair : 1;
}
// Bit-plane form (edge_gw_kernel<6, true, true>): the per-edge launch over rebuilt rows in the 24-bit modes, scalar
// attention with heads of exactly one column-block pair.  Both halves share one wave of workgroups and the launch lasts
// as long as its slowest one, so the k-ranges are dealt per half: H * SA + (message pairs) * SM <= 256 with
// SA : SM = (cost of an attention k-step) : (cost of a message k-step) = GW_BIT_COST_A : GW_BIT_COST_M, measured on an
// MI355X.
#define GW_BIT_COST_A 3
#define GW_BIT_COST_M 4
static bool g_gw_force_six = false;    // debug, process-wide: keep the six-pass form (cgat_debug_edge_gw_force_six)
bool edge_gw_force_six(bool on) { const bool was = g_gw_force_six; g_gw_force_six = on; return was; }
// (mode and shape alone: what the debug switches cannot change)
static bool gw_bitplane_shape(int H, int Hd, int HHd, int W2, int* SA, int* SM) {
  if (!mode_24bit() || edge_mma_bf16() || mode_bf16x3()) return false;
  if (Hd != 256 || H < 1 || HHd != H * Hd || W2 <= HHd || (W2 - HHd) % 256 != 0) return false;
  const int npm = (W2 - HHd) / 256;
  // SA (H + npm * COST_M / COST_A) <= 256
  const int sa = 256 * GW_BIT_COST_A / (H * GW_BIT_COST_A + npm * GW_BIT_COST_M);
  if (sa < 1 || 256 - H * sa < npm) return false;
  *SA = sa;
  *SM = (256 - H * sa) / npm;
  return true;
}
// The plain form: S k-ranges per column-block pair, slabs summed by splitk_reduce; fp16 planes with both maxima known in the
// f16x3 mode, ONE bf16 pass for rebuilt rows under "bf16-mma" (as edge_ge_form), else six passes, three in the bf16x3 mode.
// The bit-plane form replaces it for rebuilt rows with a slot permutation where gw_bitplane_shape holds (bit_shape), unless a
// debug switch keeps the six-pass form.  te -- the edge part of grad fc_out_A -- comes from the bit-plane form's column
// sums.  With that form switched off for this launch it still runs first, for that sum alone (te_only), and the six-pass
// form writes `out`: on that debug route the whole bit-plane launch and its reducer are paid on top of the six-pass launch
// (about twice the work of either), and the six-pass launch then reuses the same slab workspace, behind them on the same
// stream.  It keeps grad fc_out_A's bits independent of the switch (tests/test_edge_gw_bitplane.py compares a layer step
// with the switch on and off bit for bit in everything but the two W_e blocks).
EdgeGwForm edge_gw_form(const EdgeGwParams& p) {
  EdgeGwForm f = {};
  if (p.E <= 0) return f;
  const bool f16 = mode_f16() && p.gmax && p.emax;
  f.rc = p.rc != nullptr;
  const bool one = f.rc && !f16 && edge_mma_bf16() && !mode_bf16x3();
  f.passes = one ? 1 : f16 ? 2 : mode_bf16x3() ? 3 : 6;
  f.S = edge_gw_splits(p.W2);
  f.grid_x = f.S * (p.W2 / 256);
  f.slab = (((size_t)cdiv(p.E, 128) * 128 * 128 * 3 + 1) / 2 + 15) / 16 * 16;
  f.ws_end = f.slab + (size_t)f.S * p.W2 * 128;
  f.bit_shape = !f16 && p.rc && p.perm && p.rc->nw * 32 == p.W2 &&
                gw_bitplane_shape(p.rc->H, p.rc->Hd, p.rc->HHd, p.W2, &f.SA, &f.SM);
  f.bitplane = f.bit_shape && !p.force_six && !g_gw_force_six;
  f.te_only = p.te && !f.bitplane;
  if (f.bit_shape) {
    const int H = p.rc->H, HHd = p.rc->HHd;
    f.npm = (p.W2 - HHd) / 256;
    f.bit_grid_x = f.SM * f.npm + f.SA * H;
    f.slabA = f.slab + (size_t)f.SM * (p.W2 - HHd) * 128;
    f.csl = f.slabA + (size_t)f.SA * HHd * 128;
    const size_t end = f.csl + (size_t)f.SA * H * 8 * 128;
    if (end > f.ws_end) f.ws_end = end;
  }
  return f;
}
// what edge_gw_launch refuses, given the form it would run
static int edge_gw_check(const EdgeGwParams&, const EdgeGwForm& f) {
  CGAT_CHECK_ARG(!f.te_only || f.bit_shape, "edge_gw: the edge part of grad fc_out_A needs the shape of the bit-plane form");
  return CGAT_OK;
}
// A record of what edge_gw_form reads and no more -- dims and which optional operands are PRESENT -- for the questions
// asked before there are operands (edge_gw_bitplane_layer, the debug queries).  Never launched.
static EdgeGwParams edge_gw_shape(int E, int W2, const EdgeRC* rc, bool maxima, bool perm, bool force_six, bool te) {
  alignas(16) static float present_f;
  static int present_i;
  static GwTe present_te;
  EdgeGwParams p = edge_gw_params(&present_f, 128, (long)E * 128, &present_f, 128, perm ? &present_i : nullptr, E, W2, nullptr,
                                  nullptr, 128);
  p.rc = rc;
  if (maxima) p.gmax = p.emax = &present_f;
  p.force_six = force_six;
  if (te) p.te = &present_te;
  return p;
}
static EdgeRC edge_rc_shape_only(int H, int Hd, int W2) {
  EdgeRC rc = {};
  rc.H = H; rc.Hd = Hd; rc.HHd = H * Hd; rc.nw = W2 / 32;
  return rc;
}
// (bit_shape, not bitplane: independent of the debug switches -- the bit form of the layer's saved buffer rests on that)
bool edge_gw_bitplane_layer(int H, int Hd) {
  const EdgeRC rc = edge_rc_shape_only(H, Hd, 2 * H * Hd);
  return edge_gw_form(edge_gw_shape(1, 2 * H * Hd, &rc, false, true, false, false)).bit_shape;
}
// workspace floats: e planes (zero-padded to a multiple of 128 slots) + slabs.  The slab part is the MAXIMUM over both
// forms on purpose (the bit-plane form: at most 256 workgroup tiles of 256 x 128 and 256 x 8 rows of column sums, 35 MB;
// the plain form needs 33 MB at W2 = 1536), also for launches that never take the bit-plane route: the size then does not
// depend on the route or on the debug switch, and the dry and the real pass of a layer agree whatever either decides.
size_t edge_gw_ws_floats(int E, int W2) {
  const size_t planes = ((size_t)cdiv(E, 128) * 128 * 128 * 3 + 1) / 2;
  const size_t plain = (size_t)edge_gw_splits(W2) * W2 * 128, bit = (size_t)256 * 256 * 128 + (size_t)256 * 8 * 128;
  return planes + (plain > bit ? plain : bit) + 64;
}

// The reducer of the bit-plane form: one workgroup per 32 outputs of one column, eight threads per output.
// The slabs are added in fp64 and rounded once (the ranges are shorter than the six-pass form's: more slabs per output,
// and their fp32 sum was most of the product's error at few edges) -- fixed order, deterministic.
//   message column:   out = sum over the SM slabs (eight contiguous groups summed in order, then the groups in order)
//   attention column: P likewise over the SA slabs; cs_h[j] = the SA x 8 partial rows, thread q the rows of slot quad q
//                     in range order, then q in order;  out = wA (P + 0.01 (cs - P)) on the rounded P and cs as
//                     d = cs - P;  u = fma(0.01, d, P);  out = wA * u, each one fp32 rounding, in this order
// te (the bit form of the layer's saved buffer): an attention workgroup also leaves
//   te.part[4 col + quarter] = sum over its 32 outputs j of We[col, j] * u[col, j]     (fp64, a fixed tree over the lanes)
// the edge part of grad fc_out_A; gw_te_add_kernel adds the four quarters to te.out[col].  out == nullptr: nothing else.
__global__ __launch_bounds__(256) void edge_gw_bit_reduce_kernel(const float* __restrict__ slabM, int SM,
                                                                 const float* __restrict__ slabA, int SA,
                                                                 const float* __restrict__ csl, const float* __restrict__ wA,
                                                                 int H, int HHd, int W2, float* __restrict__ out, long ldo,
                                                                 const GwTe te) {
  __shared__ double part[8][32], cpart[8][32];
  const int o = threadIdx.x & 31, zg = threadIdx.x >> 5;
  const int col = blockIdx.x >> 2, j = 32 * (blockIdx.x & 3) + o;
  const bool isA = col < HHd;
  const int splits = isA ? SA : SM, per = (splits + 7) / 8;
  const int z0 = zg * per, z1 = min(splits, z0 + per);
  const long rows = isA ? HHd : W2 - HHd;
  const float* src = (isA ? slabA : slabM) + (long)(isA ? col : col - HHd) * 128 + j;
  double sd = 0., cd = 0.;
  for (int z = z0; z < z1; ++z) sd += (double)src[(long)z * rows * 128];
  if (isA) {
    const float* cr = csl + ((long)(col / 256) * 8 + zg) * 128 + j;
    for (int z = 0; z < SA; ++z) cd += (double)cr[(long)z * H * 8 * 128];
  }
  part[zg][o] = sd; cpart[zg][o] = cd;
  __syncthreads();
  if (zg != 0) return;
#pragma unroll
  for (int g = 1; g < 8; ++g) { sd += part[g][o]; cd += cpart[g][o]; }
  float s = (float)sd;
  if (isA) {
    const float u = __fmaf_rn(0.01f, __fsub_rn((float)cd, s), s);
    s = __fmul_rn(wA[col], u);
    if (te.part) {   // (uniform per workgroup; lanes 0..31 of wave 0 are the only threads left)
      double p = (double)te.We[(long)col * te.ldw + j] * (double)u;
#pragma unroll
      for (int w = 16; w > 0; w >>= 1) p += __shfl_xor(p, w, 64);
      if (o == 0) te.part[(long)col * 4 + (blockIdx.x & 3)] = p;
    }
  }
  if (out) out[(long)col * ldo + j] = s;
}
__global__ void gw_te_add_kernel(const double* __restrict__ part, int HHd, float* __restrict__ out) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= HHd) return;
  const double* p = part + (long)col * 4;
  out[col] = (float)(((p[0] + p[1]) + (p[2] + p[3])) + (double)out[col]);
}

// ---- edge_gw_kernel's argument list, expanded here and nowhere else: the bit-plane form (bit) or the plain form ----
static void edge_gw_go(const EdgeGwForm& f, const EdgeGwParams& p, bool bit, hipStream_t stream) {
  const EdgeRC rcv = f.rc ? *p.rc : EdgeRC{};
#define GW_GO(P_, R_, B_)                                                                                             \
  hipLaunchKernelGGL((edge_gw_kernel<P_, R_, B_>), dim3(B_ ? f.bit_grid_x : f.grid_x), dim3(512), 0, stream, p.gZ, p.ldg,  \
                     p.gzb, (const uint4*)p.ws, p.ws + f.slab, p.E, p.W2 / 128, cdiv(p.E, 32), B_ ? f.SM : f.S, p.gmax,  \
                     p.emax, rcv, B_ ? p.e : nullptr, B_ ? p.lde : 0l, B_ ? p.perm : nullptr, B_ ? f.SA : 0,           \
                     B_ ? p.ws + f.slabA : nullptr, B_ ? p.ws + f.csl : nullptr)
  if (bit) GW_GO(6, true, true);
  else if (f.passes == 1) GW_GO(1, true, false);
  else if (f.rc) { if (f.passes == 2) GW_GO(2, true, false); else if (f.passes == 6) GW_GO(6, true, false); else GW_GO(3, true, false); }
  else { if (f.passes == 2) GW_GO(2, false, false); else if (f.passes == 6) GW_GO(6, false, false); else GW_GO(3, false, false); }
#undef GW_GO
}

// out[col * ldo + k] = sum_t G[t, col] * e[perm[t] * lde + k],   G[t, 128 a + j] at gZ[t * ldg + a * gzb + j]
int edge_gw_launch(const EdgeGwParams& p, hipStream_t stream) {
  if (p.E <= 0) {
    GemmParams z = gemm_params(p.W2, 128, 0, nullptr, 1, nullptr, 1, p.out, p.ldo);
    return gemm_launch(z, nullptr, 0, stream);   // K = 0: zero fill
  }
  const EdgeGwForm f = edge_gw_form(p);
  CGAT_TRY(edge_gw_check(p, f));
  // operand (a = slot block, b = slot in block, c = k) = e[perm[128 a + b] * lde + c], zero past E
  CGAT_TRY(prepare_T_bf16_rows_launch(p.e, p.lde, p.perm, p.E, p.ws, cdiv(p.E, 128), stream, f.passes == 2 ? p.emax : nullptr));
  if (f.bitplane || f.te_only) {
    {
      CGAT_PROF("edge_gw", stream);
      edge_gw_go(f, p, true, stream);
      CGAT_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(edge_gw_bit_reduce_kernel, dim3(p.W2 * 4), dim3(256), 0, stream, p.ws + f.slab, f.SM, p.ws + f.slabA, f.SA,
                       p.ws + f.csl, p.rc->wA, p.rc->H, p.rc->HHd, p.W2, f.te_only ? nullptr : p.out, p.ldo, p.te ? *p.te : GwTe{});
    CGAT_LAUNCH_CHECK();
    if (p.te) {
      hipLaunchKernelGGL(gw_te_add_kernel, dim3(cdiv(p.rc->HHd, 256)), dim3(256), 0, stream, p.te->part, p.rc->HHd, p.te->out);
      CGAT_LAUNCH_CHECK();
    }
    if (!f.te_only) return CGAT_OK;
  }
  {
    CGAT_PROF(p.perm ? "edge_gw" : "rows_gw", stream);
    edge_gw_go(f, p, false, stream);
    CGAT_LAUNCH_CHECK();
  }
  return splitk_reduce_launch(p.ws + f.slab, f.S, p.W2, 128, p.out, p.ldo, stream);
}

// ---------------------------------------------------------------------------------------
//     Gj[n, :] = sum_{edges leaving n} gZ[t, :]          (edge_gj_kernel: the x_j-side segment sum of the rebuilt rows)
// One workgroup per GJ_NODES source nodes, a thread per four columns (256 threads walk the W2 / 4 quads); per edge a thread fetches its
// mask word, its coefficient and -- message half -- four floats of the destination's gS row (the destinations of a
// node's edges are its neighbours in the same crystal: those rows stay in L2), instead of 16 bytes of a 6-KB gZ row
// gathered from HBM.  Edges four at a time so that the dependent chain slot -> destination -> row overlaps.
// ---------------------------------------------------------------------------------------
#define GJ_NODES 4
__global__ __launch_bounds__(256) void edge_gj_kernel(const EdgeRC rc, const int* __restrict__ src_rowptr,
                                                      const int* __restrict__ src_pos, int N, int W2,
                                                      float* __restrict__ Gj, long ldo, float* __restrict__ gjmax) {
  float gmax = 0.f;
  // XCD-aware order: consecutive workgroup ids go to different XCDs (own L2 each), but the gS rows a node gathers are
  // those of its neighbours, i.e. of nearby nodes: give every XCD one contiguous range of nodes, so that a crystal's rows
  // are fetched into one L2 instead of into five to eight (PMC: 3.1 GB of HBM traffic per launch for a 0.26-GB table)
  const int per_xcd = gridDim.x / 8;                       // the grid is a multiple of 8
  const int blk = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  const int n0 = blk * GJ_NODES, n1 = min(N, n0 + GJ_NODES);
  for (int q = threadIdx.x; 4 * q < W2; q += 256) {      // four columns per thread (W2 = 1536: 1.5 rounds)
    const int col = 4 * q;
    const bool isA = col < rc.HHd;
    const int cc = isA ? col : col - rc.HHd, h = cc / rc.Hd;
    const int word = col >> 5, bit = col & 31;
    const float* coef = (isA ? rc.ga : rc.alpha) + h;
    for (int n = n0; n < n1; ++n) {
      const int r0 = src_rowptr[n], r1 = src_rowptr[n + 1];
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int rb = r0; rb < r1; rb += 4) {
        long t[4];
        float k[4];
        unsigned m[4];
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = src_pos[rb + u < r1 ? rb + u : r1 - 1];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          k[u] = rb + u < r1 ? coef[t[u] * rc.H] : 0.f;
          m[u] = rc.mask[t[u] * rc.nw + word];
          // (attention half: the constant wA through the same load -- see edge_gw_kernel)
          v[u] = *reinterpret_cast<const float4*>(isA ? rc.wA + cc : rc.gS + (long)rc.dst[t[u]] * rc.HHd + cc);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned mb = m[u] >> bit;
          acc.x += (k[u] * v[u].x) * rc_d(mb, 0); acc.y += (k[u] * v[u].y) * rc_d(mb, 1);
          acc.z += (k[u] * v[u].z) * rc_d(mb, 2); acc.w += (k[u] * v[u].w) * rc_d(mb, 3);
        }
      }
      *reinterpret_cast<float4*>(Gj + (long)n * ldo + col) = acc;
      gmax = fmaxf(fmaxf(gmax, fmaxf(fabsf(acc.x), fabsf(acc.y))), fmaxf(fabsf(acc.z), fabsf(acc.w)));
    }
  }
  if (gjmax) block_absmax_commit(gmax, gjmax);
}
int edge_gj_launch(const EdgeRC& rc, const int* src_rowptr, const int* src_pos, int N, int W2, float* Gj, long ldo,
                   hipStream_t stream, float* gjmax) {
  if (N <= 0) return CGAT_OK;
  CGAT_CHECK_ARG(W2 % 4 == 0 && (ldo % 4) == 0 && (((uintptr_t)Gj) & 15) == 0,
                 "edge_gj: W2 = %d must be a multiple of 4 with a 16-byte aligned output", W2);
  CGAT_PROF("edge_gj", stream);
  hipLaunchKernelGGL(edge_gj_kernel, dim3(cdiv(cdiv(N, GJ_NODES), 8) * 8), dim3(256), 0, stream, rc, src_rowptr, src_pos,
                     N, W2, Gj, ldo, gjmax);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// debug (include/cgat_hip.h): the form of a launch of these dims and present operands in the current arithmetic and
// edge-storage modes, on records that are never launched.  The weight lies as the backward products' (128 contiguous
// outputs per input column; the heads launch: [128, W2] row-major); the K-split launch takes edge_ge_ksplit_groups' groups.
extern "C" int cgat_debug_edge_bwd_form(int32_t product, int32_t launch, int32_t rows, int32_t W2, int32_t H, int32_t Hd,
                                        int32_t rebuilt, int32_t maxima, int32_t perm, int32_t force_six, int32_t te,
                                        cgat_edge_bwd_form* out) {
  CGAT_CHECK_ARG(out && (product == 0 || product == 1) && launch >= 0 && launch <= (product == 0 ? 3 : 0) && rows >= 0 &&
                 W2 > 0 && W2 % 128 == 0 && H > 0 && Hd > 0, "debug_edge_bwd_form: bad arguments");
  alignas(16) static float present_f;
  static int present_i;
  const EdgeRC rc = edge_rc_shape_only(H, Hd, W2);
  memset(out, 0, sizeof(*out));
  if (product == 1) {
    const EdgeGwParams p = edge_gw_shape(rows, W2, rebuilt ? &rc : nullptr, maxima != 0, perm != 0, force_six != 0, te != 0);
    const EdgeGwForm f = edge_gw_form(p);
    CGAT_TRY(edge_gw_check(p, f));
    out->passes = f.passes; out->rc = f.rc; out->bitplane = f.bitplane; out->grid_x = f.grid_x;
    out->bit_shape = f.bit_shape; out->te_only = f.te_only; out->ranges = f.S; out->SA = f.SA; out->SM = f.SM;
    out->message_pairs = f.npm; out->bit_grid_x = f.bit_grid_x;
    out->ws_end = (int64_t)f.ws_end; out->ws_floats = (int64_t)edge_gw_ws_floats(rows, W2);
    return CGAT_OK;
  }
  EdgeGeParams p = edge_ge_params(&present_f, 128, (long)rows * 128, launch == 2 ? nullptr : &present_f, launch == 3 ? 1 : 128,
                                  launch == 3 ? W2 : 1, &present_f, W2, &present_f, 128, rows);
  if (rebuilt) p.rc = &rc;
  if (maxima) p.amax = &present_f;
  if (perm) p.scatter = &present_i;
  if (launch == 1) { p.slabs = &present_f; p.S = edge_ge_ksplit_groups(rows, W2, rebuilt != 0); }
  if (launch == 3) p.heads = H;
  const EdgeGeForm f = edge_ge_form(p);
  CGAT_TRY(edge_ge_check(p, f));
  out->passes = f.passes; out->rc = f.rc; out->bitplane = f.bitplane; out->prep = f.prep; out->grid_x = f.grid_x;
  out->groups = f.groups; out->blocks_per_group = f.ncb_g; out->heads = f.heads;
  return CGAT_OK;
}
