// The hypernetwork contraction without ever materialising the predicted weights.
//
// Reference (CGAT/Hypernetworksmp.py:236-254, 205-209): per row n a Linear(C -> C*C + C) emits
// a C x C matrix W_n and bias b_n (66 KB per row at C = 128), then y_n = W_n v_n + b_n.
// With T[o,i,k] = weight[(o*C + i), k] this is the trilinear form
//        y[n,o] = sum_{i,k} T[o,i,k] v[n,i] z[n,k]  (+ bias-row terms handled by plain GEMMs)
// which is a GEMM whose A operand is the row-wise outer product v (x) z, generated on the fly
// in registers: one v_mul per MFMA.  The three backward products have the same shape under a
// permutation of T's indices, so one kernel serves forward, d/dv and d/dz:
//
//   bilinear_rows :  out[n,c]   = init[n,c] + sum_{a,b} p[n,a] q[n,b] T[a,b,c]             (this file)
//   bilinear_wgrad:  out[a,b,c] = sum_n p[n,a] q[n,b] r[n,c]                               (bilwgrad.hip)
// T is read as an operand image made by bilinear_prepare_T (opimage.hip).
//
// Fast path (NB = NC = 128): 128 rows per workgroup, wave w owns rows 32w..32w+31 and all 128
// output columns (4 accumulator blocks); q lives in 64 VGPRs per lane for the whole kernel, p
// is fetched one scalar per 256 MFMAs, T streams through LDS in 16 KB chunks (contiguous
// 512-byte rows, double-buffered).  MFMA-bound by construction: 32 768 v_mfma_f32_32x32x2_f32
// per wave per 128 rows, 2*C^3 flop per row.
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// T is expected in the "interleaved" layout made by bilinear_prepare_T: row (a,b) holds its 128
// output columns as [r = c % 32][cb = c / 32], so that lane r fetches the B operands of its four
// accumulator blocks with ONE ds_read_b128.
// grid = asplit * tiles: workgroup (s, tile) covers a in [s*NA/asplit, (s+1)*NA/asplit) and writes
// a partial slab when asplit > 1 (summed in fixed order by sum_slabs_batch_launch, rowops.hip).
// JS = j-steps per LDS chunk (a chunk is 2*JS rows of T = JS KB), FLUSH = number of consecutive
// `a` whose products share one partial accumulator (two-level summation, see below).
template <int JS, int FLUSH>
__global__ __launch_bounds__(256, 1) void bilinear_rows128_kernel(const float* __restrict__ p, long ldp,
                                                                  const float* __restrict__ q, long ldq,
                                                                  const float* __restrict__ T,
                                                                  const float* __restrict__ init, long ldi,
                                                                  float* __restrict__ out, long ldo, int nrows,
                                                                  int NA, int tiles, int asplit, long slab_stride) {
  constexpr int NCH = 64 / JS;          // chunks per `a`
  constexpr int NP = JS / 4;            // 16-byte pieces per thread per chunk (2*JS rows * 32 pieces / 256 threads)
  __shared__ __attribute__((aligned(16))) float Bs[2][2 * JS * 128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hi = lane >> 5;
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int a_beg = (int)((long)NA * split / asplit), a_end = (int)((long)NA * (split + 1) / asplit);
  const int row0 = tile * 128 + wave * 32;
  const int myrow = row0 + r;
  const long rowc = myrow < nrows ? myrow : nrows - 1;
  if (asplit > 1) {
    out += (long)split * slab_stride;
    if (split > 0) init = nullptr;
  }

  // q[row, 64*hi .. 64*hi+63] stays in registers
  float qreg[64];
  {
    const float4* qp = reinterpret_cast<const float4*>(q + rowc * ldq + 64 * hi);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float4 t = qp[j];
      qreg[4 * j] = t.x; qreg[4 * j + 1] = t.y; qreg[4 * j + 2] = t.z; qreg[4 * j + 3] = t.w;
    }
  }
  f32x16 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      float v = 0.f;
      if (init) {
        int orow = row0 + (t & 3) + 8 * (t >> 2) + 4 * hi;
        if (orow < nrows) v = init[(long)orow * ldi + cb * 32 + r];
      }
      acc[cb][t] = v;
    }

  // chunk (a, jc): T rows  a*128 + 64*kk + JS*jc + jj,  kk in {0,1}, jj < JS  -> LDS row kk*JS + jj.
  // Thread piece i (< NP) covers LDS row f_row + 8*i: kk = (f_row + 8 i) / JS, jj = (f_row + 8 i) % JS.
  const int f_row = tid >> 5, f_cq = tid & 31;
  // named staging registers (an array captured by a lambda is demoted to scratch by hipcc)
  float4 pre0, pre1, pre2, pre3, pre4, pre5, pre6, pre7;
#define BIL_G1(i_, reg_)                                                                                   \
  if constexpr ((i_) < NP) {                                                                               \
    constexpr int kk = (8 * (i_)) / JS;                                                                    \
    reg_ = *reinterpret_cast<const float4*>(tb + ((long)(64 * kk + 8 * (i_) - kk * JS)) * 128);            \
  }
#define BIL_GLOAD(a_, jc_)                                                                                 \
  {                                                                                                        \
    const float* tb = T + ((long)(a_) * 128 + JS * (jc_) + f_row) * 128 + 4 * f_cq;                        \
    BIL_G1(0, pre0) BIL_G1(1, pre1) BIL_G1(2, pre2) BIL_G1(3, pre3)                                        \
    BIL_G1(4, pre4) BIL_G1(5, pre5) BIL_G1(6, pre6) BIL_G1(7, pre7)                                        \
  }
#define BIL_S1(i_, reg_) \
  if constexpr ((i_) < NP) *reinterpret_cast<float4*>(lb + 8 * (i_) * 128) = reg_;
#define BIL_LSTORE(buf_)                                                                                   \
  {                                                                                                        \
    float* lb = &Bs[buf_][f_row * 128 + 4 * f_cq];                                                         \
    BIL_S1(0, pre0) BIL_S1(1, pre1) BIL_S1(2, pre2) BIL_S1(3, pre3)                                        \
    BIL_S1(4, pre4) BIL_S1(5, pre5) BIL_S1(6, pre6) BIL_S1(7, pre7)                                        \
  }
  BIL_GLOAD(a_beg, 0);
  BIL_LSTORE(0);
  float pa = p[rowc * ldp + a_beg];
  __syncthreads();
  // Two-level summation: the 128*FLUSH products of FLUSH consecutive `a` go into fresh accumulators
  // that are then added to the totals -- the error growth of the reference's blocked order
  // (W_n = T z ; y = W_n v), instead of one 16 384-term fp32 chain.
  int buf = 0;
  for (int a2 = a_beg; a2 < a_end; a2 += FLUSH) {
    f32x16 part[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int t = 0; t < 16; ++t) part[cb][t] = 0.f;
    for (int a = a2; a < a2 + FLUSH && a < a_end; ++a) {
      const int an = (a + 1 < a_end) ? a + 1 : a;  // the prefetch after the last chunk re-reads a valid chunk, unused
      float pa_next = p[rowc * ldp + an];
#pragma unroll
      for (int jc = 0; jc < NCH; ++jc) {
        if (jc + 1 < NCH) BIL_GLOAD(a, jc + 1) else BIL_GLOAD(an, 0);
        // B operands of step jj for this lane's four blocks: one 16-byte LDS read, fetched ahead
        const float4* bs = reinterpret_cast<const float4*>(&Bs[buf][(hi * JS) * 128 + 4 * r]);
        float4 bv = bs[0];
#pragma unroll
        for (int jj = 0; jj < JS; ++jj) {
          float4 bn = bv;
          if (jj + 1 < JS) bn = bs[(jj + 1) * 32];
          __builtin_amdgcn_sched_barrier(0);  // keep the next step's LDS read ahead of this step's MFMAs
          const float av = pa * qreg[JS * jc + jj];
          part[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv.x, part[0], 0, 0, 0);
          part[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv.y, part[1], 0, 0, 0);
          part[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv.z, part[2], 0, 0, 0);
          part[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv.w, part[3], 0, 0, 0);
          bv = bn;
        }
        BIL_LSTORE(buf ^ 1);
        __syncthreads();
        buf ^= 1;
      }
      pa = pa_next;
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) acc[cb] += part[cb];
  }
#undef BIL_G1
#undef BIL_GLOAD
#undef BIL_S1
#undef BIL_LSTORE
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      int orow = row0 + (t & 3) + 8 * (t >> 2) + 4 * hi;
      if (orow < nrows) out[(long)orow * ldo + cb * 32 + r] = acc[cb][t];
    }
}

// ---------------------------------------------------------------------------------------
// Split-bf16 form of the same contraction (the default arithmetic, "bf16x6").  Every fp32 operand x is
// written x = x1 + x2 + x3 with bf16 pieces (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2):
// 24 significant bits in all) and a product a*b is accumulated in fp32 as
//     a3b1 + a1b3 + a2b2 + a2b1 + a1b2 + a1b1        (six bf16 MFMA passes, smallest terms first);
// products of bf16 pairs are exact in fp32 and the dropped terms are <= 2^-24 relative.  Measured on
// MI355X (tools/bf16x3_probe.hip): max-norm relative error vs fp64 4.0e-7 / 9.4e-7 / 3.2e-6 at K = 128 /
// 2048 / 16384, against 4.5e-7 / 1.2e-6 / 4.2e-6 for the f32-input MFMA chain -- the same accuracy, at
// a matrix-core ceiling of 2500/6 = 417 TFLOP/s of fp32-equivalent work instead of 157.  PASSES = 3
// keeps only a2b1 + a1b2 + a1b1 (~3e-6; mode "bf16x3", never the default).
//
// The bf16 MFMA's accumulator alignment drops low bits floor-wise (measured: a sign-independent bias of
// about -5e-11 of the running sum per accumulation step; the f32-input MFMA rounds to nearest), which
// over 16 384-term sums is coherent across rows.  Consecutive partial sums are therefore accumulated
// with opposite product signs ((-1)^a folded into the prepared T and into p) so the biases cancel.
//
// "Scale-after" evaluation order:
//     out[n,c] = init[n,c] + sum_a p[n,a] * ( sum_b q[n,b] T[a,b,c] )
// The inner sum is a K = 128 GEMM whose row operand q never changes: its three bf16 planes are split
// ONCE and stay in 96 VGPRs for the whole kernel, T arrives pre-split, so the loop holds no operand
// arithmetic at all -- LDS fragment reads and MFMAs only.  The 128*6 exact products of one `a` go into
// fresh fp32 accumulators (the inner level of the two-level summation), which are then scaled by
// p[n,a] and added to the totals (one v_fma per 3 MFMAs).  The product is computed transposed
// (D[c,n]: T fragment = the MFMA's A operand, q fragment = B) so that every accumulator register of a
// lane belongs to one of its two rows and p[n,a] is a per-lane scalar.
//
// T reaches LDS by LDS-DMA (global_load_lds: no staging VGPRs, no ds_write) into a 4-slot ring of 24-KB
// chunks with the loads of chunk i+3 in flight while chunk i is consumed; one raw s_barrier per chunk
// behind a counted vmcnt.  The p column of each `a` is staged the same way two `a` ahead.  Fragments
// are read one 12-MFMA group ahead -- across the barrier too, because chunk i+1 was already retired
// and published by the barrier that ended chunk i-1 -- so a wave never waits on LDS latency with an
// empty matrix pipe.
//   RAW: chunk j is issued in iteration j-3, retired by this wave's `vmcnt(3)` at the end of iteration
//        j-2, published by the barrier that follows; first read in iteration j-1 (group-0 prefetch).
//   WAR: chunk j+3 overwrites the slot of chunk j-1, all of whose reads were consumed by MFMAs issued
//        before the barrier that ended iteration j-1; the glds is issued after that barrier.
// The LDS-DMA is issued from inline asm: hipcc would otherwise wait vmcnt(0) before every ds_read that
// follows a glds builtin (it cannot tell ring slots apart).  No other vector-memory instruction may
// appear in the loop, so the counts are exact: per iteration 3 T loads, preceded (chunk 0 of each `a`)
// by one p load.
//
// MFMA shape: v_mfma_f32_16x16x32_bf16.  Same flop per cycle as 32x32x16, but under the chip's power
// management it sustains a higher clock (MI355X_MICROARCH.md "DVFS give-back" item 7); measured here
// on the same kernel structure: 1.39 ms vs 1.54 ms per 83 340-row launch.
// Wave tile 32 rows x 128 columns = 2 row blocks x 8 column blocks of 16; a lane owns rows
// n = (lane & 15) and 16 + (lane & 15) and, per column block, columns 4 (lane >> 4) + 0..3.
// T layout (prepare_T_bf16_kernel), holding (-1)^a T[a]:
//   Tq[a][half = c/64][kh = b/64][s2 = (b/32)%2][piece][cb = (c%64)/16][kg = (b%32)/8][i = c%16][j = b%8]
// one chunk = (a, half, kh) = 2 k-steps x 3 planes x 4 column blocks x 1 KB; a fragment is one ds_read_b128.

// Timing-only ablations of the fp16 form at 83 340 rows (the ablation build and its driver are in the history at
// 43b4fa4): 754 us as is, 729 without the barrier, 682 without the LDS-DMA loads, 673 without both, against 520 us of
// pure MFMA issue at the 1.9 GHz the chip holds here.  Tried and dropped (round 1): 4 waves x 64 rows per workgroup
// (one wave per SIMD on the 512-register budget, every T fragment feeding four row blocks instead of two, i.e. half
// the LDS fragment traffic): 777 us -- what it saves in LDS reads it loses by having no second wave to cover the
// flush, the barrier wait and the accumulator-register copies.
template <int PASSES>
__global__ __launch_bounds__(512, 2) void bilinear_rows128_ring16_kernel(
    const float* __restrict__ p, long ldp, const float* __restrict__ q, long ldq, const uint4* __restrict__ Tq,
    const float* __restrict__ init, long ldi, float* __restrict__ out, long ldo, int nrows, int NA, int tiles, int asplit,
    long slab_stride, int vec_io, const float* __restrict__ tmax) {
  constexpr bool F16 = PASSES == 2;             // two fp16 planes, three passes (mfma_bf16.h); tmax = max |T|
  constexpr int NP = F16 ? 2 : 3;               // planes per operand
  constexpr int CH16 = 2 * NP * 4 * 64;         // 16-byte pieces per chunk = 24 KB (16 KB)
  constexpr int PST = 8 * 64;
  __shared__ uint4 smem[4 * CH16 + 4 * PST / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int a_beg = (int)((long)NA * split / asplit), a_end = (int)((long)NA * (split + 1) / asplit);
  const int row_w = tile * 256 + wave * 32;
  const int row_a = row_w + n16, row_b = row_w + 16 + n16;           // the lane's two output rows
  const long rowc_a = row_a < nrows ? row_a : nrows - 1, rowc_b = row_b < nrows ? row_b : nrows - 1;
  const int row_st = row_w + (lane & 31);                            // the row whose p this lane stages
  const long rowc_st = row_st < nrows ? row_st : nrows - 1;
  if (asplit > 1) {
    out += (long)split * slab_stride;
    if (split > 0) init = nullptr;
  }
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const unsigned wave_p = __builtin_amdgcn_readfirstlane(sbase + 4 * CH16 * 16 + wave * 256);
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + lane;
  const float* pst = reinterpret_cast<const float*>(smem + 4 * CH16) + wave * 64 + n16;
  p += (long)tile * 256 * ldp;                                       // scalar tile base + 32-bit lane offsets
  const unsigned prow_off = (unsigned)((rowc_st - (long)tile * 256) * ldp * 4);
  const unsigned t_off = (unsigned)tid * 16;
  const long last_chunk = (long)a_end * 4 - 1;

  // q[row, 32 s + 8 kg + j] for both row blocks as three bf16 (two fp16) planes: qf[plane][2 s + nb]
  bf16x8 q1[8], q2[8], q3[F16 ? 1 : 8];
  float rs_a = 1.f, rs_b = 1.f;                 // F16: 1 / (scale of the lane's q row * scale of T)
  if constexpr (F16) {
    float qv[2][32];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
        qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
      }
    float st, it;
    pow2_scale(tmax[0], st, it);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
      m = fmaxf(m, __shfl_xor(m, 16));          // the row's 128 values live in the four lanes n16 + 16 kg
      m = fmaxf(m, __shfl_xor(m, 32));
      float sq, iq;
      pow2_scale(m, sq, iq);
      (nb ? rs_b : rs_a) = iq * it;
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
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        const float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        split3_x8(v, q1[2 * s + nb], q2[2 * s + nb], q3[2 * s + nb]);
      }
  }
  // acc[2 cb8 + nb][t] = out[row(nb)][16 cb8 + 4 kg + t]
  f32x4 acc[16];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = nb ? row_b : row_a;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (init && row < nrows) {
        const float* ip = init + (long)row * ldi + 16 * cb + 4 * kg;
        if (vec_io) v = *reinterpret_cast<const float4*>(ip);
        else v = make_float4(ip[0], ip[1], ip[2], ip[3]);
      }
      acc[2 * cb + nb][0] = v.x; acc[2 * cb + nb][1] = v.y; acc[2 * cb + nb][2] = v.z; acc[2 * cb + nb][3] = v.w;
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#define RG_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const uint4* tb = Tq + gi * CH16;                                                          \
    const unsigned dst = wave_t + (unsigned)((gi_) & 3) * (CH16 * 16);                         \
    glds_b128(tb, t_off, dst);                                                                 \
    glds_b128(tb + 512, t_off, dst + 8192);                                                    \
    if (NP == 3) glds_b128(tb + 1024, t_off, dst + 16384);                                     \
  }
#define RG_PLOAD(a_)                                                                           \
  {                                                                                            \
    const int aa = (a_) < a_end ? (a_) : a_end - 1;                                            \
    glds_b32(p + aa, prow_off, wave_p + (unsigned)((a_) & 3) * (PST * 4));                     \
  }
  RG_PLOAD(a_beg);
  RG_PLOAD(a_beg + 1);
  RG_TLOAD((long)a_beg * 4 + 0);
  RG_TLOAD((long)a_beg * 4 + 1);
  RG_TLOAD((long)a_beg * 4 + 2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fa3, fb1, fb2, fb3;
  // group (s2, cb): the three planes of one 16-column block at one k-step
#define RG_READ(F1_, F2_, F3_, slot_, s2_, cb_)                                                \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * (CH16) + (((s2_) * NP) * 4 + (cb_)) * 64;              \
    F1_ = fp[0];                                                                               \
    F2_ = fp[4 * 64];                                                                          \
    if (PASSES >= 6) F3_ = fp[8 * 64];                                                         \
  }
#define RG_MFMA1(F1_, F2_, F3_, qi_, P_)                                                       \
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
#define RG_MFMA(F1_, F2_, F3_, s_, cb_)                                                        \
  {                                                                                            \
    RG_MFMA1(F1_, F2_, F3_, 2 * (s_) + 0, part[2 * (cb_) + 0])                                 \
    RG_MFMA1(F1_, F2_, F3_, 2 * (s_) + 1, part[2 * (cb_) + 1])                                 \
  }
  RG_READ(fa1, fa2, fa3, 0, 0, 0);
  f32x4 part[8];
  for (int a = a_beg; a < a_end; ++a) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
      const int half = ch >> 1, c2 = ch & 1;
      RG_TLOAD((long)a * 4 + ch + 3);
      if (ch == 0) RG_PLOAD(a + 2);          // AFTER the T loads: see the wait below
      if (c2 == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const int s = 2 * c2 + s2;
#pragma unroll
        for (int cbp = 0; cbp < 2; ++cbp) {
          // column block 2 cbp on set A (read 2 cbp + 1 into set B first), then 2 cbp + 1 on set B
          RG_READ(fb1, fb2, fb3, ch, s2, 2 * cbp + 1);
          __builtin_amdgcn_sched_barrier(0);
          RG_MFMA(fa1, fa2, fa3, s, 2 * cbp);
          if (cbp == 0) RG_READ(fa1, fa2, fa3, ch, s2, 2)
          else if (s2 == 0) RG_READ(fa1, fa2, fa3, ch, 1, 0)
          else RG_READ(fa1, fa2, fa3, (ch + 1) & 3, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          RG_MFMA(fb1, fb2, fb3, s, 2 * cbp + 1);
        }
      }
      if (c2 == 1) {
        float pva = pst[(a & 3) * PST], pvb = pst[(a & 3) * PST + 16];
        if constexpr (F16) { pva *= rs_a; pvb *= rs_b; }
        const float pas_a = (a & 1) ? -pva : pva, pas_b = (a & 1) ? -pvb : pvb;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[2 * (4 * half + cb) + 0][t] = fmaf(pas_a, part[2 * cb + 0][t], acc[2 * (4 * half + cb) + 0][t]);
            acc[2 * (4 * half + cb) + 1][t] = fmaf(pas_b, part[2 * cb + 1][t], acc[2 * (4 * half + cb) + 1][t]);
          }
      }
      // chunk i + 2 (issued one iteration ago) must have landed.  Younger than it: this iteration's T loads and, for
      // ch < 2, the p load issued right behind the T loads of ch == 0 (needed two `a` later; issued BEFORE them, as it
      // used to be, every ch == 0 wait drained it -- a 64-line strided load -- within one k-step)
      if (ch < 2) wait_vmcnt<NP + 1>();
      else wait_vmcnt<NP>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef RG_TLOAD
#undef RG_PLOAD
#undef RG_READ
#undef RG_MFMA1
#undef RG_MFMA
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = nb ? row_b : row_a;
      if (row < nrows) {
        float* op = out + (long)row * ldo + 16 * cb + 4 * kg;
        const f32x4 v = acc[2 * cb + nb];
        if (vec_io) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else { op[0] = v[0]; op[1] = v[1]; op[2] = v[2]; op[3] = v[3]; }
      }
    }
}

// ---------------------------------------------------------------------------------------
// f16x3c form of the forward contraction (round 4): 24-bit operands at 1.25 x the matrix time of the fp16 form.
// Same workgroup shape, ring, scale-after flush and sign alternation as bilinear_rows128_ring16_kernel<2>; what differs:
//  * a chunk is (a, column half, PAIR of 16-column blocks) over the whole K = 128 (prepare_T_f16c_kernel's image: 16 KB of
//    fp16 planes + 9 KB of 6-bit images, contiguous), so the partial accumulators of a chunk are 2 blocks x 2 row blocks
//    = 16 registers instead of 32 and are flushed at the end of every chunk -- that is what makes room for the 36 registers
//    of the row operand's 6-bit images;
//  * per chunk 8 groups of 6 fp16 MFMAs (k-step s, block cb2) and, riding with the first six groups, the three
//    correction terms (t6 x h6, h6 x t6, l6 x l6: one v_mfma_f32_16x16x128_f8f6f4 per row block each) of the chunk's two
//    column blocks; every fragment is read one group ahead;
//  * 25 LDS-DMA pieces of 1 KB per chunk: three per wave and a fourth by wave 0 (its counted waits allow one more).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void bilinear_rows128_ring16c_kernel(
    const float* __restrict__ p, long ldp, const float* __restrict__ q, long ldq, const uint4* __restrict__ Tq,
    const float* __restrict__ init, long ldi, float* __restrict__ out, long ldo, int nrows, int NA, int tiles, int asplit,
    long slab_stride, int vec_io, const float* __restrict__ tmax) {
  constexpr int CH16 = F16C_CHUNK16;
  constexpr int PST = 8 * 64;
  __shared__ uint4 smem[4 * CH16 + 4 * PST / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int n16 = lane & 15, kg = lane >> 4;
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int a_beg = (int)((long)NA * split / asplit), a_end = (int)((long)NA * (split + 1) / asplit);
  const int row_w = tile * 256 + wave * 32;
  const int row_a = row_w + n16, row_b = row_w + 16 + n16;           // the lane's two output rows
  const long rowc_a = row_a < nrows ? row_a : nrows - 1, rowc_b = row_b < nrows ? row_b : nrows - 1;
  const int row_st = row_w + (lane & 31);                            // the row whose p this lane stages
  const long rowc_st = row_st < nrows ? row_st : nrows - 1;
  if (asplit > 1) {
    out += (long)split * slab_stride;
    if (split > 0) init = nullptr;
  }
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const unsigned wave_p = __builtin_amdgcn_readfirstlane(sbase + 4 * CH16 * 16 + wave * 256);
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + lane;
  const unsigned char* cring = reinterpret_cast<const unsigned char*>(smem) + 16384;
  const float* pst = reinterpret_cast<const float*>(smem + 4 * CH16) + wave * 64 + n16;
  p += (long)tile * 256 * ldp;                                       // scalar tile base + 32-bit lane offsets
  const unsigned prow_off = (unsigned)((rowc_st - (long)tile * 256) * ldp * 4);
  const unsigned t_off = (unsigned)tid * 16;
  const long last_chunk = (long)a_end * 4 - 1;

  // q[row, 32 s + 8 kg + j] of both row blocks, scaled per row: two fp16 planes qf[2 s + nb] + the three 6-bit images
  bf16x8 q1[8], q2[8];
  frag6 ql6[2], qh6[2], qt6[2];
  float rs_a, rs_b;                             // 1 / (scale of the lane's q row * scale of T)
  {
    float qv[2][32];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
        qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
      }
    float st, it;
    pow2_scale(tmax[0], st, it);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
      m = fmaxf(m, __shfl_xor(m, 16));          // the row's 128 values live in the four lanes n16 + 16 kg
      m = fmaxf(m, __shfl_xor(m, 32));
      float sq, iq;
      pow2_scale(m, sq, iq);
      (nb ? rs_b : rs_a) = iq * it;
#pragma unroll
      for (int j = 0; j < 32; ++j) qv[nb][j] *= sq;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = qv[nb][8 * s + j];
        split2_x8_f16(v, q1[2 * s + nb], q2[2 * s + nb]);
      }
      f16c_pack32(qv[nb], ql6[nb], qh6[nb], qt6[nb]);   // element 8 s + j <-> k = 32 s + 8 kg + j, as in the image
    }
  }
  // acc[2 cb8 + nb][t] = out[row(nb)][16 cb8 + 4 kg + t]
  f32x4 acc[16];
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = nb ? row_b : row_a;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (init && row < nrows) {
        const float* ip = init + (long)row * ldi + 16 * cb + 4 * kg;
        if (vec_io) v = *reinterpret_cast<const float4*>(ip);
        else v = make_float4(ip[0], ip[1], ip[2], ip[3]);
      }
      acc[2 * cb + nb][0] = v.x; acc[2 * cb + nb][1] = v.y; acc[2 * cb + nb][2] = v.z; acc[2 * cb + nb][3] = v.w;
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // ... and the compiler must KNOW that these loads have landed: it does not see the wait above, keeps them pending across
  // the loop header and waits for them at their first use -- the flush of every chunk, an `s_waitcnt vmcnt(0)` inside the
  // loop that also drains the LDS-DMA pieces just issued for three chunks ahead (round 5: found in the ISA after the
  // kernel's ablations showed the stream costing 0.3 ms per launch that nothing else accounted for)
#pragma unroll
  for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(acc[i]));

#define RC_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_chunk ? (gi_) : last_chunk;                                   \
    const uint4* tb = Tq + gi * CH16;                                                          \
    const unsigned dst = wave_t + (unsigned)((gi_) & 3) * (CH16 * 16);                         \
    glds_b128(tb, t_off, dst);                                                                 \
    glds_b128(tb + 512, t_off, dst + 8192);                                                    \
    glds_b128(tb + 1024, t_off, dst + 16384);                                                  \
    if (wave_u == 0) glds_b128(tb + 1536, t_off, dst + 24576);                                 \
  }
#define RC_PLOAD(a_)                                                                           \
  {                                                                                            \
    const int aa = (a_) < a_end ? (a_) : a_end - 1;                                            \
    glds_b32(p + aa, prow_off, wave_p + (unsigned)((a_) & 3) * (PST * 4));                     \
  }
  // everything except the N_ youngest vector-memory operations of this wave (wave 0: + its extra piece) has landed
#define RC_WAIT(N_) { if (wave_u == 0) wait_vmcnt<(N_) + 1>(); else wait_vmcnt<(N_)>(); }
  RC_PLOAD(a_beg);
  RC_PLOAD(a_beg + 1);
  RC_TLOAD((long)a_beg * 4 + 0);
  RC_TLOAD((long)a_beg * 4 + 1);
  RC_TLOAD((long)a_beg * 4 + 2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fb1, fb2;
  frag6 ce;
  // group g = 2 s + cb2 of a chunk: the two planes of block cb2 at k-step s
#define RC_READ(F1_, F2_, slot_, g_)                                                           \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * CH16 + ((((g_) >> 1) * 2) * 2 + ((g_) & 1)) * 64;      \
    F1_ = fp[0];                                                                               \
    F2_ = fp[2 * 64];                                                                          \
  }
  // 6-bit fragment j = 3 cb2 + term of a chunk
#define RC_CREAD(slot_, j_)                                                                    \
  {                                                                                            \
    const unsigned char* cp = cring + (slot_) * (CH16 * 16) + (j_) * 1536;                     \
    const uint4 u_ = *reinterpret_cast<const uint4*>(cp + lane * 16);                          \
    const uint2 w_ = *reinterpret_cast<const uint2*>(cp + 1024 + lane * 8);                    \
    ce.w[0] = u_.x; ce.w[1] = u_.y; ce.w[2] = u_.z; ce.w[3] = u_.w; ce.w[4] = w_.x; ce.w[5] = w_.y; \
  }
#define RC_MFMA(F1_, F2_, g_)                                                                  \
  {                                                                                            \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                         \
      f32x4& P_ = part[2 * ((g_) & 1) + nb];                                                   \
      P_ = mma16<true>(F2_, q1[2 * ((g_) >> 1) + nb], P_);                                     \
      P_ = mma16<true>(F1_, q2[2 * ((g_) >> 1) + nb], P_);                                     \
      P_ = mma16<true>(F1_, q1[2 * ((g_) >> 1) + nb], P_);                                     \
    }                                                                                          \
  }
  // correction fragment j (held in ce) into the partial accumulators of its block
#define RC_CORR(j_)                                                                            \
  {                                                                                            \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                         \
      f32x4& P_ = part[2 * ((j_) / 3) + nb];                                                   \
      if ((j_) % 3 == 0) P_ = f16c_mma_th(ce, qh6[nb], P_);                                    \
      else if ((j_) % 3 == 1) P_ = f16c_mma_ht(ce, qt6[nb], P_);                               \
      else P_ = f16c_mma_ll(ce, ql6[nb], P_);                                                  \
    }                                                                                          \
  }
  RC_READ(fa1, fa2, 0, 0);
  RC_CREAD(0, 0);
  f32x4 part[4];
  for (int a = a_beg; a < a_end; ++a) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {           // chunk (a, half = ch >> 1, block pair ch & 1) sits in ring slot ch
      RC_TLOAD((long)a * 4 + ch + 3);
      if (ch == 0) RC_PLOAD(a + 2);            // AFTER the T loads: see the wait below
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int gp = 0; gp < 4; ++gp) {         // groups 2 gp (set A) and 2 gp + 1 (set B)
        RC_READ(fb1, fb2, ch, 2 * gp + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * gp < 6) { RC_CORR(2 * gp); RC_CREAD(ch, 2 * gp + 1); }
        RC_MFMA(fa1, fa2, 2 * gp);
        if (gp < 3) RC_READ(fa1, fa2, ch, 2 * gp + 2)
        else RC_READ(fa1, fa2, (ch + 1) & 3, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * gp + 1 < 6) {
          RC_CORR(2 * gp + 1);
          if (2 * gp + 2 < 6) RC_CREAD(ch, 2 * gp + 2)
          else RC_CREAD((ch + 1) & 3, 0);
        }
        RC_MFMA(fb1, fb2, 2 * gp + 1);
      }
      __builtin_amdgcn_sched_barrier(0);       // the flush stays HERE: moved into the next chunk it would keep two sets
      {                                        // of partial accumulators alive
        float pva = pst[(a & 3) * PST] * rs_a, pvb = pst[(a & 3) * PST + 16] * rs_b;
        const float pas_a = (a & 1) ? -pva : pva, pas_b = (a & 1) ? -pvb : pvb;
#pragma unroll
        for (int cb2 = 0; cb2 < 2; ++cb2)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[2 * (2 * ch + cb2) + 0][t] = fmaf(pas_a, part[2 * cb2 + 0][t], acc[2 * (2 * ch + cb2) + 0][t]);
            acc[2 * (2 * ch + cb2) + 1][t] = fmaf(pas_b, part[2 * cb2 + 1][t], acc[2 * (2 * ch + cb2) + 1][t]);
          }
        // ... and is COMPLETE here: the wave-dependent wait below is control flow, and without this the compiler sinks
        // all four flushes of an `a` behind its last barrier (64 partial accumulators alive instead of 16)
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(acc[4 * ch + i]));
      }
      __builtin_amdgcn_sched_barrier(0);
      // chunk i + 2 (issued one iteration ago) must have landed.  Younger than it: this iteration's three (four) T loads
      // and, for ch < 2, the p load issued right behind the T loads of ch == 0
      if (ch < 2) RC_WAIT(4)
      else RC_WAIT(3)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef RC_TLOAD
#undef RC_PLOAD
#undef RC_WAIT
#undef RC_READ
#undef RC_CREAD
#undef RC_MFMA
#undef RC_CORR
  // the thread id is laundered so that the output addresses are computed HERE instead of being hoisted above the main
  // loop and kept alive (= spilled) across it
  int tl = tid;
  asm volatile("" : "+v"(tl));
  const int e_row = tile * 256 + (tl >> 6) * 32 + (tl & 15), e_kg = (tl >> 4) & 3;
#pragma unroll
  for (int cb = 0; cb < 8; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = e_row + 16 * nb;
      if (row < nrows) {
        float* op = out + (long)row * ldo + 16 * cb + 4 * e_kg;
        const f32x4 v = acc[2 * cb + nb];
        if (vec_io) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else { op[0] = v[0]; op[1] = v[1]; op[2] = v[2]; op[3] = v[3]; }
      }
    }
}

// ---------------------------------------------------------------------------------------
// f16x3c form of the fused backward contraction (round 4): out1 = init1 + sum_a p[:,a] M[:,a,:] and the partial sums of
// dv[n,a] = sum_c zz[n,c] M[n,a,c] from ONE contraction M[n,a,c] = sum_b q[n,b] T[a,b,c] (bilinear_rows128_dual_kernel's
// algebra), on bilinear_rows128_ring16c_kernel's machinery (same prepared image, chunks, ring, correction terms).
//
// Loop order: the 32-column chunk index ch = (half, block pair) is the OUTER loop, `a` the inner one.  The second
// gradient needs zz[n, c] for the chunk's columns at every flush; with `a` outermost (the forward kernel's order) that
// is either 64 registers for all 128 columns -- the dual kernel pays them by giving a wave only 64 columns, i.e. 128
// rows per workgroup and twice the L2 -> LDS traffic per row, which is what bounds it -- or a reload per chunk (tried:
// +41 % vector-memory traffic, 1.42 ms against 1.18 without the loads).  With ch outermost a wave holds the zz values and
// the output accumulators of ONE chunk column range at a time (16 + 16 registers instead of 64 + 64), covers all 128
// columns of its 32 rows in four phases, and a workgroup is 256 rows like the forward kernel's.  The prepared image is
// read in (ch, a) order -- chunks are contiguous 25-KB pieces either way -- and every chunk of T is still streamed once
// per workgroup.  dv comes out as four partial sums per (row, a), one per phase: dvp[ch][a][row] (dual_finish_kernel
// adds them).  The ring slot of a chunk is its sequence number mod 4 (run-time: one address add per chunk).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 2) void bilinear_rows128_dualc_kernel(
    const float* __restrict__ p, long ldp, const float* __restrict__ q, long ldq, const float* __restrict__ zz, long ldz,
    const uint4* __restrict__ Tq, const float* __restrict__ init, long ldi, float* __restrict__ out, long ldo,
    float* __restrict__ dvp, int dv_ld, int nrows, int NA, int tiles, int asplit, long slab_stride, int vec_io,
    const float* __restrict__ tmax) {
  constexpr int CH16 = F16C_CHUNK16;
  constexpr int PST = 8 * 64;
  __shared__ uint4 smem[4 * CH16 + 4 * PST / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);
  const int n16 = lane & 15, kg = lane >> 4;
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int a_beg = (int)((long)NA * split / asplit), a_end = (int)((long)NA * (split + 1) / asplit);
  // chunks of this workgroup: sequence number n = ch * (a_end - a_beg) + (a - a_beg)
  const int row_w = tile * 256 + wave * 32;
  const int row_a = row_w + n16, row_b = row_w + 16 + n16;           // the lane's two output rows
  const long rowc_a = row_a < nrows ? row_a : nrows - 1, rowc_b = row_b < nrows ? row_b : nrows - 1;
  const int row_st = row_w + (lane & 31);                            // the row whose p this lane stages
  const long rowc_st = row_st < nrows ? row_st : nrows - 1;
  if (asplit > 1) {
    out += (long)split * slab_stride;
    if (split > 0) init = nullptr;
  }
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + wave * 1024);
  const unsigned wave_p = __builtin_amdgcn_readfirstlane(sbase + 4 * CH16 * 16 + wave * 256);
  const bf16x8* ring0 = reinterpret_cast<const bf16x8*>(smem) + lane;
  const float* pst = reinterpret_cast<const float*>(smem + 4 * CH16) + wave * 64 + n16;
  p += (long)tile * 256 * ldp;                                       // scalar tile base + 32-bit lane offsets
  const unsigned prow_off = (unsigned)((rowc_st - (long)tile * 256) * ldp * 4);
  const unsigned t_off = (unsigned)tid * 16;

  // q[row, 32 s + 8 kg + j] of both row blocks, scaled per row: two fp16 planes qf[2 s + nb] + the three 6-bit images
  bf16x8 q1[8], q2[8];
  frag6 ql6[2], qh6[2], qt6[2];
  float rs_a, rs_b;                             // 1 / (scale of the lane's q row * scale of T)
  {
    float qv[2][32];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
        qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
      }
    float st, it;
    pow2_scale(tmax[0], st, it);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
      m = fmaxf(m, __shfl_xor(m, 16));          // the row's 128 values live in the four lanes n16 + 16 kg
      m = fmaxf(m, __shfl_xor(m, 32));
      float sq, iq;
      pow2_scale(m, sq, iq);
      (nb ? rs_b : rs_a) = iq * it;
#pragma unroll
      for (int j = 0; j < 32; ++j) qv[nb][j] *= sq;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = qv[nb][8 * s + j];
        split2_x8_f16(v, q1[2 * s + nb], q2[2 * s + nb]);
      }
      f16c_pack32(qv[nb], ql6[nb], qh6[nb], qt6[nb]);   // element 8 s + j <-> k = 32 s + 8 kg + j, as in the image
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // chunk (ch_, a_) with sequence number n_ -> ring slot n_ % 4; its p column -> staging slot n_ % 4 (each wave stages
  // and reads its own rows).  Past the end the last chunk is loaded again (keeps the counted waits uniform).
#define DC_TLOAD(n_, ch_, a_)                                                                  \
  {                                                                                            \
    const int ci_ = __builtin_amdgcn_readfirstlane((a_) * 4 + (ch_));   /* uniform: the DMA base must be scalar */ \
    const uint4* tb = Tq + (long)ci_ * CH16;                                                   \
    const unsigned dst = wave_t + (unsigned)__builtin_amdgcn_readfirstlane((n_) & 3) * (CH16 * 16); \
    glds_b128(tb, t_off, dst);                                                                 \
    glds_b128(tb + 512, t_off, dst + 8192);                                                    \
    glds_b128(tb + 1024, t_off, dst + 16384);                                                  \
    if (wave_u == 0) glds_b128(tb + 1536, t_off, dst + 24576);                                 \
  }
#define DC_PLOAD(n_, a_)                                                                       \
  glds_b32(p + __builtin_amdgcn_readfirstlane(a_), prow_off,                                   \
           wave_p + (unsigned)__builtin_amdgcn_readfirstlane((n_) & 3) * (PST * 4));
  // (ta, tch) = the chunk three sequence numbers ahead of the one being computed, advanced in (ch, a) order
  int ta = a_beg, tch = 0;
#define DC_ADVANCE() { if (ta + 1 < a_end) ++ta; else if (tch < 3) { ta = a_beg; ++tch; } }
  // everything except the N_ youngest vector-memory operations of this wave (wave 0: + its extra piece) has landed
#define DC_WAIT(N_) { if (wave_u == 0) wait_vmcnt<(N_) + 1>(); else wait_vmcnt<(N_)>(); }
  DC_TLOAD(0, tch, ta); DC_PLOAD(0, ta); DC_ADVANCE();
  DC_TLOAD(1, tch, ta); DC_PLOAD(1, ta); DC_ADVANCE();
  DC_TLOAD(2, tch, ta); DC_PLOAD(2, ta); DC_ADVANCE();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fb1, fb2;
  frag6 ce;
  // group g = 2 s + cb2 of the chunk at ring_: the two planes of block cb2 at k-step s
#define DC_READ(F1_, F2_, ring_, g_)                                                           \
  {                                                                                            \
    const bf16x8* fp = (ring_) + ((((g_) >> 1) * 2) * 2 + ((g_) & 1)) * 64;                    \
    F1_ = fp[0];                                                                               \
    F2_ = fp[2 * 64];                                                                          \
  }
  // 6-bit fragment j = 3 cb2 + term of the chunk at ring_
#define DC_CREAD(ring_, j_)                                                                    \
  {                                                                                            \
    const unsigned char* cp = reinterpret_cast<const unsigned char*>((ring_) - lane) + 16384 + (j_) * 1536; \
    const uint4 u_ = *reinterpret_cast<const uint4*>(cp + lane * 16);                          \
    const uint2 w_ = *reinterpret_cast<const uint2*>(cp + 1024 + lane * 8);                    \
    ce.w[0] = u_.x; ce.w[1] = u_.y; ce.w[2] = u_.z; ce.w[3] = u_.w; ce.w[4] = w_.x; ce.w[5] = w_.y; \
  }
#define DC_MFMA(F1_, F2_, g_)                                                                  \
  {                                                                                            \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                         \
      f32x4& P_ = part[2 * ((g_) & 1) + nb];                                                   \
      P_ = mma16<true>(F2_, q1[2 * ((g_) >> 1) + nb], P_);                                     \
      P_ = mma16<true>(F1_, q2[2 * ((g_) >> 1) + nb], P_);                                     \
      P_ = mma16<true>(F1_, q1[2 * ((g_) >> 1) + nb], P_);                                     \
    }                                                                                          \
  }
#define DC_CORR(j_)                                                                            \
  {                                                                                            \
    _Pragma("unroll") for (int nb = 0; nb < 2; ++nb) {                                         \
      f32x4& P_ = part[2 * ((j_) / 3) + nb];                                                   \
      if ((j_) % 3 == 0) P_ = f16c_mma_th(ce, qh6[nb], P_);                                    \
      else if ((j_) % 3 == 1) P_ = f16c_mma_ht(ce, qt6[nb], P_);                               \
      else P_ = f16c_mma_ll(ce, ql6[nb], P_);                                                  \
    }                                                                                          \
  }
  DC_READ(fa1, fa2, ring0, 0);
  DC_CREAD(ring0, 0);
  f32x4 part[4];
  int n = 0;                                   // sequence number of the chunk being computed
#pragma clang loop unroll(disable)
  for (int ch = 0; ch < 4; ++ch) {             // columns 32 ch .. 32 ch + 31
    // this phase's output accumulators and zz values: acc[2 cb2 + nb][t] <-> (row(nb), column 32 ch + 16 cb2 + 4 kg + t)
    f32x4 acc[4], zq[4];
#pragma unroll
    for (int cb2 = 0; cb2 < 2; ++cb2)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int row = nb ? row_b : row_a;
        const int col = 32 * ch + 16 * cb2 + 4 * kg;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (init && row < nrows) {
          const float* ip = init + (long)row * ldi + col;
          if (vec_io) v = *reinterpret_cast<const float4*>(ip);
          else v = make_float4(ip[0], ip[1], ip[2], ip[3]);
        }
        acc[2 * cb2 + nb] = f32x4{v.x, v.y, v.z, v.w};
        const float4 z4 = *reinterpret_cast<const float4*>(zz + (nb ? rowc_b : rowc_a) * ldz + col);
        zq[2 * cb2 + nb] = f32x4{z4.x, z4.y, z4.z, z4.w};
      }
    float* dvc = dvp + (long)ch * NA * dv_ld;   // this phase's partial sums: dvp[ch][a][row]
#pragma clang loop unroll(disable)
    for (int a = a_beg; a < a_end; ++a, ++n) {
      const bf16x8* ring = ring0 + (n & 3) * CH16;
      const bf16x8* ringn = ring0 + ((n + 1) & 3) * CH16;
      DC_TLOAD(n + 3, tch, ta);
      DC_PLOAD(n + 3, ta);
      DC_ADVANCE();
#pragma unroll
      for (int i = 0; i < 4; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int gp = 0; gp < 4; ++gp) {         // groups 2 gp (set A) and 2 gp + 1 (set B)
        DC_READ(fb1, fb2, ring, 2 * gp + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * gp < 6) { DC_CORR(2 * gp); DC_CREAD(ring, 2 * gp + 1); }
        DC_MFMA(fa1, fa2, 2 * gp);
        if (gp < 3) DC_READ(fa1, fa2, ring, 2 * gp + 2)
        else DC_READ(fa1, fa2, ringn, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (2 * gp + 1 < 6) {
          DC_CORR(2 * gp + 1);
          if (2 * gp + 2 < 6) DC_CREAD(ring, 2 * gp + 2)
          else DC_CREAD(ringn, 0);
        }
        DC_MFMA(fb1, fb2, 2 * gp + 1);
      }
      __builtin_amdgcn_sched_barrier(0);       // the flush stays HERE (see bilinear_rows128_ring16c_kernel)
      {
        const float sg = (a & 1) ? -1.f : 1.f;   // part = (-1)^a M[n,a,:] (the prepared T alternates in sign)
        const float sga = sg * rs_a, sgb = sg * rs_b;
        const float pas_a = sga * pst[(n & 3) * PST], pas_b = sgb * pst[(n & 3) * PST + 16];
        float da = 0.f, db = 0.f;
#pragma unroll
        for (int cb2 = 0; cb2 < 2; ++cb2)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[2 * cb2 + 0][t] = fmaf(pas_a, part[2 * cb2 + 0][t], acc[2 * cb2 + 0][t]);
            acc[2 * cb2 + 1][t] = fmaf(pas_b, part[2 * cb2 + 1][t], acc[2 * cb2 + 1][t]);
            da = fmaf(part[2 * cb2 + 0][t], zq[2 * cb2 + 0][t], da);
            db = fmaf(part[2 * cb2 + 1][t], zq[2 * cb2 + 1][t], db);
          }
        asm volatile("" : "+v"(da));             // keep the two sums out of v_pk_* (note in edgez.hip)
        asm volatile("" : "+v"(db));
        da += __shfl_xor(da, 16, 64); da += __shfl_xor(da, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        // one store for both row blocks: lanes 0..15 carry rows 0..15 (da), lanes 16..31 rows 16..31 (db)
        const float dv = (kg & 1) ? sgb * db : sga * da;
        if (kg < 2) dvc[(long)a * dv_ld + row_w + (lane & 31)] = dv;   // dv_ld >= the tile-padded row count
#pragma unroll
        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(acc[i]));   // the flush is complete here (ring16c)
      }
      __builtin_amdgcn_sched_barrier(0);
      // chunk n + 2 (issued one iteration ago) must have landed.  Younger than it: the previous iteration's p load and
      // dv store, this iteration's three (four) T loads, p load and dv store.  (Anything issued between two phases --
      // output stores, zz / init loads -- sits in between and only makes the wait stricter.)  The p value of chunk n + 1
      // was requested two iterations ago, in front of chunk n + 2: it has landed too.
      DC_WAIT(7)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
    // this phase's 32 output columns (the thread id is laundered: addresses computed here, not kept across the loop)
    {
      int tl = tid;
      asm volatile("" : "+v"(tl));
      const int e_row = tile * 256 + (tl >> 6) * 32 + (tl & 15), e_kg = (tl >> 4) & 3;
#pragma unroll
      for (int cb2 = 0; cb2 < 2; ++cb2)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int row = e_row + 16 * nb;
          if (row < nrows) {
            float* op = out + (long)row * ldo + 32 * ch + 16 * cb2 + 4 * e_kg;
            const f32x4 v = acc[2 * cb2 + nb];
            if (vec_io) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            else { op[0] = v[0]; op[1] = v[1]; op[2] = v[2]; op[3] = v[3]; }
          }
        }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef DC_TLOAD
#undef DC_PLOAD
#undef DC_WAIT
#undef DC_ADVANCE
#undef DC_READ
#undef DC_CREAD
#undef DC_MFMA
#undef DC_CORR
}

// ---------------------------------------------------------------------------------------
// Two gradients from one contraction (hypernetwork backward, reference Hypernetworksmp.py:77-83 under autograd):
//     out1[n,c] = init1[n,c] + sum_a p[n,a] * M[n,a,c]              M[n,a,c] = sum_b q[n,b] T[a,b,c]
//     dv  [n,a] =              sum_c zz[n,c] * M[n,a,c]
// With T[a=i][b=o][c=k] = head_w[o,i,k], p = v (layer input), q = g (gradient of the layer's pre-norm output) and
// zz = z (trunk output), out1 is the gradient wrt z and dv the bilinear part of the gradient wrt v: the scale-after
// kernel already holds M[n,a,:] in its partial accumulators when it finishes an `a`, so the second gradient is one
// more multiply-add per accumulator register and a 4-lane reduction -- instead of a second 350-GFLOP launch.
// Layout differences from bilinear_rows128_ring16_kernel: zz must stay in registers (32 VGPRs per 64 columns), so
// a wave owns 32 rows x 64 columns and the eight waves of a workgroup are 4 row groups x 2 column halves (128
// rows); a ring slot holds one 32-deep k-step of BOTH column halves (two 12-KB pieces of the prepared T), every
// wave reads its own half.  dv comes out as two partial sums per row (one per column half) in dvp[half][n][a].
template <int PASSES>
__global__ __launch_bounds__(512, 2) void bilinear_rows128_dual_kernel(
    const float* __restrict__ p, long ldp, const float* __restrict__ q, long ldq, const float* __restrict__ zz, long ldz,
    const uint4* __restrict__ Tq, const float* __restrict__ init, long ldi, float* __restrict__ out, long ldo,
    float* __restrict__ dvp, int dv_ld, int nrows, int NA, int tiles, int asplit, long slab_stride, int vec_io,
    const float* __restrict__ tmax) {
  constexpr bool F16 = PASSES == 2;             // two fp16 planes, three passes; tmax = max |T|
  constexpr int NP = F16 ? 2 : 3;
  constexpr int HP = NP * 256;                  // 16-byte pieces of one (a, half, k-step) block of the prepared T
  constexpr int CH16 = 2 * HP;                  // per ring slot: 24 KB (16 KB): [half][plane][cb][lane]
  constexpr int PST = 8 * 64;
  __shared__ uint4 smem[4 * CH16 + 4 * PST / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n16 = lane & 15, kg = lane >> 4;
  const int rg = wave & 3, hf = wave >> 2;      // row group, column half
  const int split = blockIdx.x / tiles, tile = blockIdx.x % tiles;
  const int a_beg = (int)((long)NA * split / asplit), a_end = (int)((long)NA * (split + 1) / asplit);
  const int row_w = tile * 128 + rg * 32;
  const int row_a = row_w + n16, row_b = row_w + 16 + n16;
  const long rowc_a = row_a < nrows ? row_a : nrows - 1, rowc_b = row_b < nrows ? row_b : nrows - 1;
  const int row_st = row_w + (lane & 31);
  const long rowc_st = row_st < nrows ? row_st : nrows - 1;
  if (asplit > 1) {
    out += (long)split * slab_stride;
    if (split > 0) init = nullptr;
  }
  const unsigned sbase = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;
  const unsigned wave_p = __builtin_amdgcn_readfirstlane(sbase + 4 * CH16 * 16 + wave * 256);
  const bf16x8* ring = reinterpret_cast<const bf16x8*>(smem) + hf * HP + lane;
  const float* pst = reinterpret_cast<const float*>(smem + 4 * CH16) + wave * 64 + n16;
  p += (long)tile * 128 * ldp;
  const unsigned prow_off = (unsigned)((rowc_st - (long)tile * 128) * ldp * 4);
  const unsigned l_off = (unsigned)lane * 16;
  const long last_step = (long)a_end * 4 - 1;
  // the three 1-KB pieces this wave moves per k-step: piece index P = 64 wave + 512 i of the [half0 | half1] image
  const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // scalar copy: the LDS-DMA base pointers must be SGPRs
  const int P0 = 64 * wave_u, P1 = 64 * wave_u + 512, P2 = 64 * wave_u + 1024;
  const unsigned wave_t = __builtin_amdgcn_readfirstlane(sbase + (unsigned)P0 * 16);

  bf16x8 q1[8], q2[8], q3[F16 ? 1 : 8];
  float rs_a = 1.f, rs_b = 1.f;                 // F16: 1 / (scale of the lane's q row * scale of T)
  if constexpr (F16) {
    float qv[2][32];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        qv[nb][8 * s + 0] = t0.x; qv[nb][8 * s + 1] = t0.y; qv[nb][8 * s + 2] = t0.z; qv[nb][8 * s + 3] = t0.w;
        qv[nb][8 * s + 4] = t1.x; qv[nb][8 * s + 5] = t1.y; qv[nb][8 * s + 6] = t1.z; qv[nb][8 * s + 7] = t1.w;
      }
    float st, it;
    pow2_scale(tmax[0], st, it);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) m = fmaxf(m, fabsf(qv[nb][j]));
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      float sq, iq;
      pow2_scale(m, sq, iq);
      (nb ? rs_b : rs_a) = iq * it;
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
        const float4* qp = reinterpret_cast<const float4*>(q + (nb ? rowc_b : rowc_a) * ldq + 32 * s + 8 * kg);
        const float4 t0 = qp[0], t1 = qp[1];
        const float v[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
        split3_x8(v, q1[2 * s + nb], q2[2 * s + nb], q3[2 * s + nb]);
      }
  }
  // acc[2 cb + nb][j] = out[row(nb)][64 hf + 16 cb + 4 kg + j];  zr the same elements of zz
  f32x4 acc[8], zr[8];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = nb ? row_b : row_a;
      const long rowc = nb ? rowc_b : rowc_a;
      const int col = 64 * hf + 16 * cb + 4 * kg;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (init && row < nrows) {
        const float* ip = init + (long)row * ldi + col;
        if (vec_io) v = *reinterpret_cast<const float4*>(ip);
        else v = make_float4(ip[0], ip[1], ip[2], ip[3]);
      }
      acc[2 * cb + nb] = f32x4{v.x, v.y, v.z, v.w};
      const float* zp = zz + rowc * ldz + col;
      zr[2 * cb + nb] = f32x4{zp[0], zp[1], zp[2], zp[3]};
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

#define DU_TLOAD(gi_)                                                                          \
  {                                                                                            \
    const long gi = (gi_) < last_step ? (gi_) : last_step;                                     \
    const long a_ = gi >> 2, s_ = gi & 3;                                                      \
    const uint4* h0 = Tq + ((a_ * 2 + 0) * 4 + s_) * HP;                                       \
    const uint4* h1 = Tq + ((a_ * 2 + 1) * 4 + s_) * HP;                                       \
    const unsigned dst = wave_t + (unsigned)((gi_) & 3) * (CH16 * 16);                         \
    glds_b128(h0 + P0, l_off, dst);                                                            \
    glds_b128(P1 < HP ? h0 + P1 : h1 + (P1 - HP), l_off, dst + 8192);                          \
    if (NP == 3) glds_b128(h1 + (P2 - HP), l_off, dst + 16384);                                \
  }
#define DU_PLOAD(a_)                                                                           \
  {                                                                                            \
    const int aa = (a_) < a_end ? (a_) : a_end - 1;                                            \
    glds_b32(p + aa, prow_off, wave_p + (unsigned)((a_) & 3) * (PST * 4));                     \
  }
  DU_PLOAD(a_beg);
  DU_PLOAD(a_beg + 1);
  DU_TLOAD((long)a_beg * 4 + 0);
  DU_TLOAD((long)a_beg * 4 + 1);
  DU_TLOAD((long)a_beg * 4 + 2);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  bf16x8 fa1, fa2, fa3, fb1, fb2, fb3;
#define DU_READ(F1_, F2_, F3_, slot_, cb_)                                                     \
  {                                                                                            \
    const bf16x8* fp = ring + (slot_) * (CH16) + (cb_) * 64;                                   \
    F1_ = fp[0];                                                                               \
    F2_ = fp[4 * 64];                                                                          \
    if (PASSES >= 6) F3_ = fp[8 * 64];                                                         \
  }
#define DU_MFMA1(F1_, F2_, F3_, qi_, P_)                                                       \
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
#define DU_MFMA(F1_, F2_, F3_, s_, cb_)                                                        \
  {                                                                                            \
    DU_MFMA1(F1_, F2_, F3_, 2 * (s_) + 0, part[2 * (cb_) + 0])                                 \
    DU_MFMA1(F1_, F2_, F3_, 2 * (s_) + 1, part[2 * (cb_) + 1])                                 \
  }
  DU_READ(fa1, fa2, fa3, 0, 0);
  f32x4 part[8];
  // dvp[half][a][row]: the 32 rows of a wave are 128 contiguous bytes per `a` (row-major [row][a] would be 4-byte
  // stores at a 512-byte stride: 12x write amplification, measured with WRITE_SIZE).  32-bit offsets: the launcher
  // checks 2 * dv_ld * NA < 2^31
  const int dv_a = hf * NA * dv_ld + row_a, dv_b = hf * NA * dv_ld + row_b;
  for (int a = a_beg; a < a_end; ++a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) part[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {                // k-step (a, s) sits in ring slot s
      DU_TLOAD((long)a * 4 + s + 3);
      if (s == 0) DU_PLOAD(a + 2);             // AFTER the T loads: see the wait below
#pragma unroll
      for (int cbp = 0; cbp < 2; ++cbp) {
        DU_READ(fb1, fb2, fb3, s, 2 * cbp + 1);
        __builtin_amdgcn_sched_barrier(0);
        DU_MFMA(fa1, fa2, fa3, s, 2 * cbp);
        if (cbp == 0) DU_READ(fa1, fa2, fa3, s, 2)
        else DU_READ(fa1, fa2, fa3, (s + 1) & 3, 0);
        __builtin_amdgcn_sched_barrier(0);
        DU_MFMA(fb1, fb2, fb3, s, 2 * cbp + 1);
      }
      if (s == 3) {
        // part = (-1)^a M[n,a,:] (the prepared T alternates in sign): scale-after flush and the second gradient
        const float pva = pst[(a & 3) * PST], pvb = pst[(a & 3) * PST + 16];
        const float sg = (a & 1) ? -1.f : 1.f;
        const float sga = F16 ? sg * rs_a : sg, sgb = F16 ? sg * rs_b : sg;   // F16: part carries the operand scales
        const float pas_a = sga * pva, pas_b = sgb * pvb;
        float da = 0.f, db = 0.f;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            acc[2 * cb + 0][t] = fmaf(pas_a, part[2 * cb + 0][t], acc[2 * cb + 0][t]);
            acc[2 * cb + 1][t] = fmaf(pas_b, part[2 * cb + 1][t], acc[2 * cb + 1][t]);
            da = fmaf(part[2 * cb + 0][t], zr[2 * cb + 0][t], da);
            db = fmaf(part[2 * cb + 1][t], zr[2 * cb + 1][t], db);
          }
        asm volatile("" : "+v"(da));             // keep the two sums out of v_pk_* (note in edgez.hip)
        asm volatile("" : "+v"(db));
        da += __shfl_xor(da, 16, 64); da += __shfl_xor(da, 32, 64);
        db += __shfl_xor(db, 16, 64); db += __shfl_xor(db, 32, 64);
        if (kg == 0) {
          dvp[dv_a + a * dv_ld] = sga * da;        // dv_ld >= the tile-padded row count: no bounds check needed
          dvp[dv_b + a * dv_ld] = sgb * db;
        }
      }
      // chunk i + 2 (issued one iteration ago) must have landed; everything issued after it may stay in flight
      // (in-order vmcnt, stores included): the previous `a`'s two dv stores + this step's T loads + the p load (s = 0),
      // the p load + T loads (s = 1), T loads (s = 2), T loads + this `a`'s dv stores (s = 3).  With vmcnt(NP)
      // everywhere the s = 3 wait, whose two youngest operations are the stores, drained the T loads issued a
      // quarter of a microsecond earlier.
      if (s == 0) wait_vmcnt<NP + 3>();
      else if (s == 1) wait_vmcnt<NP + 1>();
      else if (s == 2) wait_vmcnt<NP>();
      else wait_vmcnt<NP + 2>();
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef DU_TLOAD
#undef DU_PLOAD
#undef DU_READ
#undef DU_MFMA1
#undef DU_MFMA
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int row = nb ? row_b : row_a;
      if (row < nrows) {
        float* op = out + (long)row * ldo + 64 * hf + 16 * cb + 4 * kg;
        const f32x4 v = acc[2 * cb + nb];
        if (vec_io) *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
        else { op[0] = v[0]; op[1] = v[1]; op[2] = v[2]; op[3] = v[3]; }
      }
    }
}

// out1 = sum of the a-split slabs (if any); out2[n,a] = init2[n,a] + sum_h dvp[h][a][n] (nhalf partial sums: 2 column
// halves from the dual kernel, 4 column phases from the f16x3c one).
// One workgroup per 32 rows: the [128 a][32 n] pieces of dvp are read coalesced and transposed through LDS.
__global__ __launch_bounds__(256) void dual_finish_kernel(const float* __restrict__ slab, int splits, long slab_stride,
                                                          int nrows, float* __restrict__ out1, long ldo1,
                                                          const float* __restrict__ dvp, int dv_ld, int NA,
                                                          const float* __restrict__ init2, long ldi2,
                                                          float* __restrict__ out2, long ldo2, int nhalf) {
  __shared__ float tile[128][33];
  const int n0 = blockIdx.x * 32, tid = threadIdx.x;
  for (int idx = tid; idx < 128 * 32; idx += 256) {   // idx = a * 32 + n
    const int a = idx >> 5, n = idx & 31;
    const long o = (long)a * dv_ld + n0 + n;
    float t = dvp[o];
    for (int h = 1; h < nhalf; ++h) t += dvp[(long)h * NA * dv_ld + o];   // partial sums in a fixed order
    tile[a][n] = t;
  }
  __syncthreads();
  // A thread owns 16 outputs (n = k * 2 + tid / 128, c = tid % 128).  The slab loop is OUTERMOST so that the 16 loads
  // of a slab are independent (with it innermost every output paid `splits` dependent round trips: 104 us for this
  // kernel at 25 slabs of 1 280 rows); each output still adds its slabs in slab order.
  const int c = tid & 127, nh = tid >> 7;
  if (splits > 1) {
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.f;
    for (int z = 0; z < splits; ++z) {
      const float* sl = slab + (long)z * slab_stride + c;
      float v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const long row = n0 + 2 * k + nh;
        v[k] = sl[(row < nrows ? row : nrows - 1) * 128];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) s[k] += v[k];
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const long row = n0 + 2 * k + nh;
      if (row < nrows) out1[row * ldo1 + c] = s[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int n = 2 * k + nh;
    const long row = n0 + n;
    if (row < nrows) out2[row * ldo2 + c] = (init2 ? init2[row * ldi2 + c] : 0.f) + tile[c][n];
  }
}

// The same at a few hundred rows (the harness' shipped batch: 1 280 atoms, up to 32 a-splits): one thread per output,
// the slab loads of an output issued eight at a time -- the 32-row workgroups above are 40 workgroups whose threads each
// walk 32 slabs for 16 outputs (35 us per launch at 1 280 rows, sixteen launches per step); same summation order.
__global__ __launch_bounds__(256) void dual_finish_small_kernel(const float* __restrict__ slab, int splits,
                                                                long slab_stride, int nrows, float* __restrict__ out1,
                                                                long ldo1, const float* __restrict__ dvp, int dv_ld, int NA,
                                                                const float* __restrict__ init2, long ldi2,
                                                                float* __restrict__ out2, long ldo2, int nhalf) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long row = i >> 7;
  const int c = (int)(i & 127);
  if (row >= nrows) return;
  if (splits > 1) {
    const float* sl = slab + row * 128 + c;
    float s = 0.f;
    int z = 0;
    for (; z + 8 <= splits; z += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = sl[(long)(z + k) * slab_stride];
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; z < splits; ++z) s += sl[(long)z * slab_stride];
    out1[row * ldo1 + c] = s;
  }
  const long o = (long)c * dv_ld + row;
  float t = dvp[o];
  for (int h = 1; h < nhalf; ++h) t += dvp[(long)h * NA * dv_ld + o];
  out2[row * ldo2 + c] = (init2 ? init2[row * ldi2 + c] : 0.f) + t;
}

// out[n, c] = sum_s slab[s][n][c] in fixed order, with the hypernetwork's LayerNorm(no affine) + tanh behind it (reference Hypernetworksmp.py:205-209): one
// wave per row sums the slabs into u (kept: backward needs the pre-norm values) and normalises what it holds in
// registers -- the arithmetic of layernorm_tanh_fwd_kernel (rowops.hip) on the same values, one launch and one read of
// u less per predicted layer.
__global__ void slab_sum_ln_tanh_kernel(const float* __restrict__ slab, int splits, long slab_stride, int nrows,
                                        float* __restrict__ out, long ldo, float* __restrict__ y, float eps) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= nrows) return;
  float x0 = 0.f, x1 = 0.f;
  int z = 0;
  for (; z + 4 <= splits; z += 4) {                // eight independent loads per round trip, added in slab order
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = slab[(long)(z + u) * slab_stride + (long)row * 128 + lane];
      b[u] = slab[(long)(z + u) * slab_stride + (long)row * 128 + 64 + lane];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { x0 += a[u]; x1 += b[u]; }
  }
  for (; z < splits; ++z) {
    x0 += slab[(long)z * slab_stride + (long)row * 128 + lane];
    x1 += slab[(long)z * slab_stride + (long)row * 128 + 64 + lane];
  }
  out[(long)row * ldo + lane] = x0;
  out[(long)row * ldo + 64 + lane] = x1;
  float s = 0.f;
  s += x0; s += x1;
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / 128;
  float v = 0.f;
  { const float d0 = x0 - mean; v += d0 * d0; const float d1 = x1 - mean; v += d1 * d1; }
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const float rstd = rsqrtf(v / 128 + eps);
  y[(long)row * 128 + lane] = tanhf((x0 - mean) * rstd);
  y[(long)row * 128 + 64 + lane] = tanhf((x1 - mean) * rstd);
}

static bool rows_fast(const float* q, long ldq, int NB, int NC) {
  return NB == 128 && NC == 128 && (ldq % 4) == 0 && (((uintptr_t)q) & 15) == 0;
}

// how many ways to split the `a` range so that tiles*split fills 256 CUs without a ragged last wave
static int rows_asplit(int nrows, int rows_wg) {
  const int tiles = cdiv(nrows, rows_wg);
  // Few rows (the reference's shipped batch of 64 crystals is 1 280 atoms = 10 tiles): every workgroup streams its share
  // of T through its LDS ring whatever the row count, so the launch takes as long as ONE workgroup needs for 128 / sp
  // slices of T -- with sp <= 4 that left 216 of the 256 CUs idle and ~60-100 us per contraction.  Up to 32 ways then
  // (>= 4 values of `a` per workgroup); the slab sum over sp x [nrows, 128] floats is negligible at these sizes.
  if (tiles * 4 <= 128) {
    int sp = 256 / tiles;
    return sp > 32 ? 32 : (sp < 4 ? 4 : sp);
  }
  int best = 1;
  double best_eff = 0.0;
  for (int sp = 1; sp <= 4; ++sp) {
    double w = (double)tiles * sp / 256.0;
    double eff = w / (double)((long)(w + 0.999999));
    if (eff > best_eff + 0.02) {
      best_eff = eff;
      best = sp;
    }
  }
  return best;
}

// rows per workgroup of the kernel that will run (the split-bf16 ring kernel uses 8 waves = 256 rows)
static int rows_per_wg() { return mode_split() ? 256 : 128; }

// the arithmetic mode (ArithMode, kernels.h)
static int g_bilinear_mode = -1;
int bilinear_mode() {
  if (g_bilinear_mode < 0) {
    const char* e = getenv("CGAT_BILINEAR_MODE");   // f32 | bf16x6 | bf16x3 | f16x3 | f16x3c (default)
    g_bilinear_mode = MODE_F16X3C;
    if (e && !strcmp(e, "f32")) g_bilinear_mode = MODE_F32;
    if (e && !strcmp(e, "bf16x3")) g_bilinear_mode = MODE_BF16X3;
    if (e && !strcmp(e, "bf16x6")) g_bilinear_mode = MODE_BF16X6;
    if (e && !strcmp(e, "f16x3")) g_bilinear_mode = MODE_F16X3;
  }
  return g_bilinear_mode;
}
void bilinear_set_mode(int m) {   // an unknown value selects f32
  g_bilinear_mode = (m == MODE_BF16X6 || m == MODE_BF16X3 || m == MODE_F16X3 || m == MODE_F16X3C) ? m : MODE_F32;
}

size_t bilinear_rows_ws_bytes(int nrows, int NA, int NB, int NC) {
  if (!bilinear_T_interleaved(NB, NC)) return 0;
  int sp = rows_asplit(nrows, rows_per_wg());
  return sp > 1 ? ws_round((size_t)sp * nrows * 128, 4) : 0;
}

// ---- fused pair of contractions (see bilinear_rows128_dual_kernel); widths 128, split-bf16 modes only ----
bool bilinear_dual_fast(int NA, int NB, int NC) {
  return mode_split() && NA == 128 && NB == 128 && NC == 128;
}
static int dual_dv_ld(int nrows) { return cdiv(nrows, 256) * 256; }   // rows padded to whole tiles (128 or 256 rows)
static int dual_asplit_max(int nrows) {   // the f16x3c form runs 256-row workgroups, the others 128-row ones
  const int a = rows_asplit(nrows, 128), b = rows_asplit(nrows, 256);
  return a > b ? a : b;
}
size_t bilinear_dual_ws_bytes(int nrows) {
  const int sp = dual_asplit_max(nrows);
  return ws_round((size_t)4 * dual_dv_ld(nrows) * 128 + (sp > 1 ? (size_t)sp * nrows * 128 : 0), 4);   // <= 4 dv partials
}
// T: bilinear_prepare_T of the [NA,128,128] operand.  out1 = init1 + sum_a p[:,a] M[:,a,:], out2 = init2 + M . zz
int bilinear_dual_launch(const float* p, long ldp, const float* q, long ldq, const float* zz, long ldz, const float* T,
                         const float* init1, long ldi1, float* out1, long ldo1, const float* init2, long ldi2,
                         float* out2, long ldo2, int nrows, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (nrows <= 0) return CGAT_OK;
  CGAT_CHECK_ARG((ldq % 4) == 0 && (((uintptr_t)q) & 15) == 0 && (((uintptr_t)T) & 15) == 0 && ldp < (1l << 22) &&
                     (long)dual_dv_ld(nrows) * 512 < (1l << 31),
                 "bilinear_dual: q and T must be 16-byte aligned with ldq %% 4 == 0, nrows < 2^23");
  const bool c256 = mode_f16c();   // the f16x3c form: 256-row workgroups, dv complete per row
  const int tiles = cdiv(nrows, c256 ? 256 : 128);
  const int sp = rows_asplit(nrows, c256 ? 256 : 128);
  if (!ws || ws_bytes < bilinear_dual_ws_bytes(nrows)) {
    cgat_set_error("bilinear_dual: workspace too small (%zu < %zu)", ws_bytes, bilinear_dual_ws_bytes(nrows));
    return CGAT_ERR_WORKSPACE;
  }
  const int dv_ld = dual_dv_ld(nrows);
  float* dvp = (float*)ws;
  float* slab = dvp + (size_t)4 * dv_ld * 128;
  float* dst = sp > 1 ? slab : out1;
  const long dld = sp > 1 ? 128 : ldo1, stride = sp > 1 ? (long)nrows * 128 : 0;
  const int vec_io = ((dld % 4) == 0 && (((uintptr_t)dst) & 15) == 0 &&
                      (!init1 || ((ldi1 % 4) == 0 && (((uintptr_t)init1) & 15) == 0))) ? 1 : 0;
  {
    CGAT_PROF("bilinear_dual", stream);
    const float* tmax = T + (size_t)128 * 128 * 128;   // f16x3: max |T| behind the two planes
    if (c256) {   // prepare_T_f16c_kernel's image, max |T| behind it
      CGAT_CHECK_ARG((ldz % 4) == 0 && (((uintptr_t)zz) & 15) == 0 && ldz < (1l << 22),
                     "bilinear_dual: zz must be 16-byte aligned with ldz %% 4 == 0");
      hipLaunchKernelGGL(bilinear_rows128_dualc_kernel, dim3(tiles * sp), dim3(512), 0, stream, p, ldp, q, ldq, zz, ldz,
                         (const uint4*)T, init1, ldi1, dst, dld, dvp, dv_ld, nrows, 128, tiles, sp, stride, vec_io,
                         T + (size_t)128 * F16C_A_FLOATS);
    } else {
      const auto kernel = mode_f16() ? bilinear_rows128_dual_kernel<2>
                                     : (mode_bf16x3() ? bilinear_rows128_dual_kernel<3> : bilinear_rows128_dual_kernel<6>);
      hipLaunchKernelGGL(kernel, dim3(tiles * sp), dim3(512), 0, stream, p, ldp, q, ldq, zz, ldz, (const uint4*)T, init1,
                         ldi1, dst, dld, dvp, dv_ld, nrows, 128, tiles, sp, stride, vec_io, tmax);
    }
    CGAT_LAUNCH_CHECK();
  }
  if (nrows <= 8192)
    hipLaunchKernelGGL(dual_finish_small_kernel, dim3(cdiv((long)nrows * 128, 256)), dim3(256), 0, stream, slab, sp, stride,
                       nrows, out1, ldo1, dvp, dv_ld, 128, init2, ldi2, out2, ldo2, c256 ? 4 : 2);
  else
    hipLaunchKernelGGL(dual_finish_kernel, dim3(cdiv(nrows, 32)), dim3(256), 0, stream, slab, sp, stride, nrows, out1, ldo1,
                       dvp, dv_ld, 128, init2, ldi2, out2, ldo2, c256 ? 4 : 2);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}

// One call of bilinear_rows_launch, as its steps take it
struct RowsCall {
  const float *p, *q, *T, *init;
  long ldp, ldq, ldi, ldo;
  float* out;
  int nrows, NA, NB, NC;
  hipStream_t stream;
};

// the width-128 kernel of the current mode into dst (row stride dld): `out`, or sp partial slabs `stride` floats apart
static int rows128_kernel_launch(const RowsCall& c, float* dst, long dld, long stride, int sp) {
  CGAT_PROF("bilinear_rows", c.stream);
  if (!mode_split()) {
    const int tiles = cdiv(c.nrows, 128);
    hipLaunchKernelGGL((bilinear_rows128_kernel<16, 2>), dim3(tiles * sp), dim3(256), 0, c.stream, c.p, c.ldp, c.q, c.ldq,
                       c.T, c.init, c.ldi, dst, dld, c.nrows, c.NA, tiles, sp, stride);
    return CGAT_OK;
  }
  const int tiles2 = cdiv(c.nrows, 256);
  const int vec_io = ((c.ldo % 4) == 0 && (dld % 4) == 0 && (((uintptr_t)dst) & 15) == 0 &&
                      (!c.init || ((c.ldi % 4) == 0 && (((uintptr_t)c.init) & 15) == 0))) ? 1 : 0;
  if (c.ldp >= (1l << 22)) {   // the kernel addresses p with 32-bit lane offsets inside a 256-row tile
    cgat_set_error("bilinear_rows: ldp %ld too large", c.ldp);
    return CGAT_ERR_ARG;
  }
  if (mode_f16c()) {   // max |T| behind prepare_T_f16c_kernel's image
    hipLaunchKernelGGL(bilinear_rows128_ring16c_kernel, dim3(tiles2 * sp), dim3(512), 0, c.stream, c.p, c.ldp, c.q, c.ldq,
                       (const uint4*)c.T, c.init, c.ldi, dst, dld, c.nrows, c.NA, tiles2, sp, stride, vec_io,
                       c.T + (size_t)c.NA * F16C_A_FLOATS);
    return CGAT_OK;
  }
  const float* tmax = c.T + (size_t)c.NA * 128 * 128;   // f16x3: max |T| behind the two planes
  const auto kernel = mode_f16() ? bilinear_rows128_ring16_kernel<2>
                                 : (mode_bf16x3() ? bilinear_rows128_ring16_kernel<3> : bilinear_rows128_ring16_kernel<6>);
  hipLaunchKernelGGL(kernel, dim3(tiles2 * sp), dim3(512), 0, c.stream, c.p, c.ldp, c.q, c.ldq, (const uint4*)c.T, c.init,
                     c.ldi, dst, dld, c.nrows, c.NA, tiles2, sp, stride, vec_io, tmax);
  return CGAT_OK;
}

// Width 128: choose where the kernel writes (out, or slabs of an a-split in the workspace), launch by mode, reduce the
// slabs -- with the LayerNorm behind the sum when ln_out asks for one (*ln_done)
static int rows_width128(const RowsCall& c, void* ws, size_t ws_bytes, float* ln_out, float ln_eps, bool* ln_done) {
  if (!rows_fast(c.q, c.ldq, c.NB, c.NC) || (((uintptr_t)c.T) & 15) != 0) {
    cgat_set_error("bilinear_rows: q and T must be 16-byte aligned with ldq %% 4 == 0 at width 128");
    return CGAT_ERR_ARG;
  }
  const int sp = rows_asplit(c.nrows, rows_per_wg());
  float* out = c.out;
  float* dst = out;
  long dld = c.ldo, stride = 0;
  if (sp > 1) {
    const size_t need = ws_round((size_t)sp * c.nrows * 128, 4);
    if (!ws || ws_bytes < need) {
      cgat_set_error("bilinear_rows: workspace too small (%zu < %zu)", ws_bytes, need);
      return CGAT_ERR_WORKSPACE;
    }
    dst = (float*)ws;
    dld = 128;
    stride = (long)c.nrows * 128;
  }
  CGAT_TRY(rows128_kernel_launch(c, dst, dld, stride, sp));
  CGAT_LAUNCH_CHECK();
  if (sp <= 1) return CGAT_OK;
  if (!ln_out) return sum_slabs_batch_launch((const float*)ws, sp, stride, stride, 1, 0, &out, c.ldo, c.stream);
  hipLaunchKernelGGL(slab_sum_ln_tanh_kernel, dim3(cdiv(c.nrows, 4)), dim3(256), 0, c.stream, (const float*)ws, sp, stride,
                     c.nrows, out, c.ldo, ln_out, ln_eps);
  CGAT_LAUNCH_CHECK();
  *ln_done = true;
  return CGAT_OK;
}

// Widths other than 128: out = init + (p (x) q) T, the row-wise outer product [nrows, NA * NB] formed in the operand
// loader of the fp32 engine (gemm.hip) and T [NA * NB, NC] as it lies: 0.6 ms at 83 340 rows of width 64 where a
// one-thread-per-output kernel took 5.4 (and 850 ms at width 256)
static int rows_other_widths(const RowsCall& c) {
  if (c.init && (c.init != c.out || c.ldi != c.ldo))
    CGAT_TRY(copy2d_launch(c.init, c.ldi, c.out, c.ldo, c.nrows, c.NC, c.stream));
  GemmParams g = gemm_params(c.nrows, c.NC, c.NA * c.NB, c.q, c.ldq, c.T, c.NC, c.out, c.ldo);
  g.b_kmajor = 1;
  g.a_outer = c.p; g.ld_a_outer = c.ldp; g.outer_n = c.NB;
  g.beta = c.init ? 1.f : 0.f;
  return gemm_launch(g, nullptr, 0, c.stream);
}

// y = tanh(LayerNorm(out)) as a pass of its own, where no slab sum carried it
static int rows_trailing_ln(const RowsCall& c, float* ln_out, float ln_eps) {
  if (c.NC != 128 || c.ldo != 128) {
    cgat_set_error("bilinear_rows: the LayerNorm epilogue needs 128 contiguous columns");
    return CGAT_ERR_ARG;
  }
  return layernorm_tanh_fwd_launch(c.out, ln_out, c.nrows, 128, ln_eps, c.stream);
}

// T must come from bilinear_prepare_T (interleaved columns iff bilinear_T_interleaved(NB, NC))
// ln_out (optional, NC = 128): y = tanh(LayerNorm(out)) [nrows,128] contiguous, fused into the slab sum when there is one
int bilinear_rows_launch(const float* p, long ldp, const float* q, long ldq, const float* T, const float* init,
                         long ldi, float* out, long ldo, int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes,
                         hipStream_t stream, float* ln_out, float ln_eps) {
  if (nrows <= 0) return CGAT_OK;
  const RowsCall c = {p, q, T, init, ldp, ldq, ldi, ldo, out, nrows, NA, NB, NC, stream};
  bool ln_done = false;
  if (bilinear_T_interleaved(NB, NC)) CGAT_TRY(rows_width128(c, ws, ws_bytes, ln_out, ln_eps, &ln_done));
  else CGAT_TRY(rows_other_widths(c));
  if (ln_out && !ln_done) return rows_trailing_ln(c, ln_out, ln_eps);
  return CGAT_OK;
}
