// Layer orchestrators: the sequence of kernel launches behind each C-ABI entry point.
// Host code only (no kernel lives here): it decides shapes, carves the caller's workspace and enqueues on the caller's
// stream -- no allocation, no synchronisation.
#include "layers.h"

// =======================================================================================
// GATConvNodes message / softmax / aggregate
// =======================================================================================
struct AttnDims {
  int N, E, C, Ce, H, Hd, D, HHd, W2;
};
static AttnDims attn_dims(const cgat_plan* plan, const cgat_attn_params* p) {
  AttnDims d;
  d.N = plan->N; d.E = plan->E; d.C = p->C; d.Ce = p->Ce; d.H = p->H; d.Hd = p->Hd;
  d.D = 2 * p->C + p->Ce; d.HHd = p->H * p->Hd; d.W2 = 2 * d.HHd;
  return d;
}

struct AttnSaved {
  float *Z, *alpha, *S, *ssum;
};
static AttnSaved attn_saved(float* saved, const AttnDims& d) {
  AttnSaved s;
  s.Z = saved;
  s.alpha = s.Z + (size_t)d.E * d.W2;
  s.S = s.alpha + (size_t)d.E * d.H;
  s.ssum = s.S + (size_t)d.N * d.HHd;
  return s;
}

// ---- storage of the per-edge intermediates Z / gZ: 0 = fp32 (default), 1 = bf16 ("bf16 activations", BASELINE
// configs[4]): halves the bytes that bound the edge phase; softmax statistics, sums and all matrix products stay as
// they are (fp32 accumulation), stated tolerance 1e-2 (tests/test_chunked.py).  Takes effect on the fused
// scalar-attention route at the benchmark widths; everything else ignores it.
static int g_edge_storage = -1;
static int edge_storage() {
  if (g_edge_storage < 0) {
    const char* e = getenv("CGAT_EDGE_STORAGE");
    g_edge_storage = (e && !strcmp(e, "bf16")) ? 1 : (e && !strcmp(e, "f32+gz")) ? 2 : (e && !strcmp(e, "bf16-mma")) ? 3 :
                     (e && !strcmp(e, "f32+za")) ? 4 : 0;
  }
  return g_edge_storage;
}
extern "C" void cgat_set_edge_storage(int32_t mode) { g_edge_storage = (mode >= 1 && mode <= 4) ? mode : 0; }
// mode 4 ("f32+za"): fp32 with the attention pre-activations stored at every shape -- mode 0 without the bit form of the
// saved buffer (attn_z_form), the A/B reference of its tests as "f32+gz" is for the stored gZ
// mode 3 ("bf16-mma"): bf16 storage of Z AND one-pass bf16 operands in the two per-edge backward products (edgebwd.hip)
static bool edge_bf16_storage() { return edge_storage() == 1 || edge_storage() == 3; }
bool edge_mma_bf16() { return edge_storage() == 3; }
extern "C" int32_t cgat_get_edge_storage(void) { return edge_storage(); }
// (f16x3: the K = 256 per-edge forward and the one-kernel segment backward; the 24-bit modes: the six-pass per-edge forward,
// the weighted sum and the three-kernel segment backward, which exist at Hd == 256 only; the f32 mode has no bf16 storage.
// A layer this predicate rejects makes cgat_nodes_attention_forward return CGAT_ERR_UNSUPPORTED under edge storage "bf16"
// -- the forward refuses what the backward could not handle (Hd = 128 / 384 ran forward and failed in backward).)
static bool attn_bf16(const AttnDims& d) {
  if (!(edge_bf16_storage() && (mode_f16() || mode_24bit()) && d.C == 128 && d.Ce == 128 &&
        d.Hd % 128 == 0 && d.W2 % 256 == 0 && d.N > 0 && d.E > 0))
    return false;
  if (!mode_f16() && !(d.Hd == 256 && d.Hd % 4 == 0)) return false;   // seg_bwd_msg / _att<true>: two 128-column blocks per head
  return true;
}

// (the saved buffer keeps its fp32 size in either storage mode: bf16 Z uses the first half of its region)
extern "C" size_t cgat_nodes_attention_saved_floats(int32_t N, int32_t E, int32_t H, int32_t Hd) {
  size_t HHd = (size_t)H * Hd;
  return (size_t)E * 2 * HHd + (size_t)E * H + (size_t)N * HHd + (size_t)N * H;
}

static int stack_in_weights(Ctx& c, const cgat_attn_params* p, const AttnDims& d, float* Wcat, float* bcat) {
  Copy2DJobs j;
  j.n = bcat ? 4 : 2;
  j.job[0] = {p->A_in_w, d.D, Wcat, d.D, d.HHd, d.D};
  j.job[1] = {p->M_in_w, d.D, Wcat + (size_t)d.HHd * d.D, d.D, d.HHd, d.D};
  if (bcat) {
    j.job[2] = {p->A_in_b, d.HHd, bcat, d.HHd, 1, d.HHd};
    j.job[3] = {p->M_in_b, d.HHd, bcat + d.HHd, d.HHd, 1, d.HHd};
  }
  RUN(copy2d_multi_launch(j, c.s));
  return CGAT_OK;
}

// ---- routes (layers.h: decided once per pass, read by every step; a dry pass takes none that depends on an operand) ----

// How the forward forms and stores Z [E, W2] -- and therefore how the backward finds it: both passes call this with the
// same x, e, saved buffer and fc_out_A weight (Z = saved; nullptr where the fused inference forms no Z).
struct ZForm {
  bool zx;        // f16x3 mode at the benchmark widths: the x_j projection is folded into the per-edge kernel
                  // (edge_zx_kernel), so Pj is never formed
  bool fused_z;   // Z and the attention logits from one fused split-bf16 per-edge launch (else: generic GEMM + row-dot)
  bool bf16;      // Z stored as bf16 (edge-storage mode "bf16"): by edge_zx in the f16x3 mode, ...
  bool bf16_six;  // ... by the six-pass per-edge kernel otherwise
  bool bits;      // the bit form of the saved buffer (attn_bit_form_dims below, on 16-byte aligned operands)
};
// The bit form: the forward keeps no attention pre-activations Z_A.  The attention columns of the
// saved buffer's rows -- one hole of H * Hd floats per row, row stride W2 as ever -- hold instead
//   rows n < N: Pi_A[n, :] (bias included) | rows N + n: Pj_A[n, :] | rows 2 N + g: the sign words of edge rows 32 g .. 32 g + 31
// from which the backward forms everything it took from Z_A.  Taken where the forward runs
// edge_z6w_kernel in fp32 storage and the backward rebuilds gZ with the bit-plane form of grad W_e (whose column sums give
// the edge part of grad fc_out_A), and the 2 N + ceil(E / 32) holes exist.  Dims, mode and storage alone:
static bool attn_bit_form_dims(const AttnDims& d) {
  return mode_24bit() && edge_storage() == 0 && d.N > 0 && d.E > 0 && d.C == 128 && edge_rc_shape(d.Ce, d.H, d.Hd) &&
         d.Hd == 256 && edge_z6w_takes(d.N, d.E, d.H, d.Hd) && edge_gw_bitplane_layer(d.H, d.Hd) &&
         2l * d.N + cdiv(d.E, 32) <= (long)d.E;
}
static ZForm attn_z_form(const AttnDims& d, const float* e, const float* x, const float* Z, const float* wA, const void* ws) {
  ZForm z;
  const bool heads = edge_z_heads(d.W2, d.H, d.Hd);
  z.zx = d.N > 0 && heads && edge_zx_dims(d.C, d.Ce, d.W2, d.W2, d.W2) && aligned16(e, x, ws, Z, wA) &&
         edge_z_dims(d.C, d.W2, d.C, d.W2, d.W2);       // (the projection Pi on the per-edge kernel)
  const bool per_edge = heads && edge_z_dims(d.Ce, d.W2, d.Ce, d.W2, d.W2) && aligned16(e, ws, Z, wA);
  z.fused_z = per_edge && !z.zx;
  z.bf16_six = attn_bf16(d) && per_edge && !mode_f16();
  z.bf16 = (attn_bf16(d) && z.zx) || z.bf16_six;
  // (fused_z: e, the workspace, the saved buffer and fc_out_A's weight are 16-byte aligned -- what the backward's vector
  // form asks of the same four)
  z.bits = z.fused_z && !z.bf16 && attn_bit_form_dims(d);
  return z;
}

// The forward without grad (infer): at the shapes edge_infer_fused takes (edgez.hip: the 24-bit modes at width 128, up to
// 2048 columns per half and 8 heads -- the harness' H = 5 -- at any number of edges, its few-row batches included) the
// logits launch and the fused
// message + weighted-sum launch replace the per-edge launch and seg_wsum, and alpha / S / ssum live in the workspace --
// nothing of size E x H x Hd is formed; everywhere else the saved buffer of the training forward is carved out of the
// workspace and the same launches run.  Either way the results are bit-identical to the training forward's.
static bool attn_infer_fused(const AttnDims& d) {
  return edge_infer_fused(d.N, d.E, d.C, d.Ce, d.H, d.Hd) && (!edge_bf16_storage() || attn_bf16(d));
}
// Round 6: fc_out_M as ONE K = H * Hd launch (the 24-bit modes, more rows than the small-row programs take): the H per-head
// weights are not one affine operand, but their six-pass images -- one batched image launch, head h's blocks behind
// head h - 1's -- are exactly the contiguous operand of the K = W2 -> 128 kernel (edgebwd.hip).  Saves five passes over
// aggr (42 MB read + written each at 83 340 atoms) and four launches.
static bool attn_out_one_shape(const AttnDims& d) {
  return mode_24bit() && d.C == 128 && d.Hd % 128 == 0 && d.N > rowprog_max_rows() && d.H <= TPREP_MAX &&
         ((d.Hd / 128) % 2) == 0;      // (even: the per-head block parity is the global one)
}

struct AttnFwdRoute {
  bool fused_infer;   // the no-grad forward on the logits launch + the fused message / weighted-sum launch
  bool zx, fused_z;   // the per-edge phase of the training forward (ZForm)
  bool z_bf16;
  bool z_bits;        // the bit form of the saved buffer (ZForm)
  bool proj_fast;     // the node projections on the per-edge kernel (else: the GEMM pair)
  bool out_fast;      // fc_out_M as H * Hd / 128 accumulating K = 128 launches of the dense-layer kernel
  bool out_one;       // ... as one K = H * Hd launch (attn_out_one_shape)
};
// saved: where Z / alpha / S / ssum of this pass live (nullptr: the fused inference, whose S is a carve-out)
static AttnFwdRoute attn_fwd_route(bool dry, const AttnDims& d, bool infer, const cgat_attn_params* p, const float* x,
                                   const float* e, const float* saved, const float* S, const float* aggr, const void* ws) {
  AttnFwdRoute r = {};
  r.fused_infer = infer && attn_infer_fused(d);
  r.out_fast = mode_split() && d.C == 128 && d.Hd % 128 == 0;
  if (dry) return r;
  const ZForm z = attn_z_form(d, e, x, saved, p->A_out_w, ws);
  r.zx = z.zx; r.fused_z = z.fused_z; r.z_bf16 = z.bf16; r.z_bits = z.bits;
  // (a few hundred atoms: the generic branch, whose products run as 16 x 16 wave tiles -- rowprog.hip -- instead of
  // five 256-row workgroups streaming the whole weight image: 86 -> ~10 us per projection at 1 280 atoms)
  r.proj_fast = d.N > rowprog_max_rows() && edge_z_heads(d.W2, d.H, d.Hd) && edge_z_dims(d.C, d.W2, d.C, d.W2, d.W2) &&
                aligned16(x, ws);
  r.out_one = attn_out_one_shape(d) && edge_ge_dims(128, d.HHd, d.HHd, 128, d.C) && aligned16(S, aggr, p->M_out_w);
  return r;
}

// fc_out_M's backward at the benchmark widths (C = 128, Hd a multiple of 128, at most DW_BATCH_MAX weight-gradient blocks)
static bool attn_bwd_out_shape(const AttnDims& d) {
  return mode_split() && d.C == 128 && d.Hd % 128 == 0 && d.H * (d.Hd / 128) <= DW_BATCH_MAX;
}
struct AttnBwdRoute {
  bool rc;             // gZ is not stored: one bit per element, the consumers rebuild the rows (struct EdgeRC, kernels.h)
  bool vec;            // the segment kernel's 16-byte loads
  bool have_scales;    // f16x3: maxima of gZ and edge_attr -> the per-edge products on two fp16 planes
  bool z_bf16, z_bf16_six;   // how the forward stored Z (ZForm)
  bool z_bits;         // ... in the bit form: no attention values, the sign words and the two half projections
  bool out_fast;       // fc_out_M's input gradients on the dense-layer kernel, its weight gradients in one batched launch
  bool out_heads_one;  // ... the input gradients of all heads in one launch pair (round 6)
};
static AttnBwdRoute attn_bwd_route(bool dry, const AttnDims& d, const cgat_attn_params* p, const float* x, const float* e,
                                   const float* saved, const float* S, const void* ws) {
  AttnBwdRoute r = {};
  // At the benchmark widths gZ [E, W2] is never stored: edge_seg_bwd_kernel leaves one bit per element behind and the
  // three consumers rebuild the rows (struct EdgeRC, kernels.h) -- E * W2 / 8 bytes of workspace instead of 4 E * W2
  // (edge storage mode 2 keeps the stored-gZ backward of round 1 at these widths too: the A/B reference of the tests)
  r.rc = mode_split() && edge_rc_shape(d.Ce, d.H, d.Hd) && d.W2 % 256 == 0 && d.N > 0 && d.E > 0 && edge_storage() != 2;
  r.out_fast = attn_bwd_out_shape(d);     // (a dry pass measures this route's per-head form)
  if (dry || d.N <= 0) { r.out_fast = r.out_fast && dry; return r; }
  r.out_fast = r.out_fast && linear128_fast(d.C, d.Hd, d.C, d.HHd, ws, ws) &&
               rows_dw128_fast((const float*)ws, d.C, S, d.HHd, nullptr, 0);   // (every S block starts 512 bytes further)
  r.out_heads_one = r.out_fast && mode_24bit() && d.N > rowprog_max_rows() && d.H > 1 && aligned16(p->M_out_w);
  r.vec = (d.Hd % 4 == 0) && aligned16(saved, ws, p->A_out_w);
  r.have_scales = r.vec && mode_f16() && d.Ce == 128 && aligned16(e);
  const ZForm z = attn_z_form(d, e, x, saved, p->A_out_w, ws);
  r.z_bf16 = z.bf16; r.z_bf16_six = z.bf16_six;
  r.z_bits = z.bits;   // (implies rc and vec: the same shapes, modes and aligned operands)
  return r;
}

// ---- forward ----
struct AttnFwd {
  AttnDims d;
  const cgat_plan* plan;
  const cgat_attn_params* p;
  const float *x, *e;
  float* aggr;
  float *Wcat, *bcat, *Pi, *Pj, *a, *Wq;
  AttnSaved sv;       // the caller's saved buffer, or (infer) carve-outs
  AttnFwdRoute r;
};
static AttnFwd attn_fwd_carve(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x, const float* e,
                              float* aggr, float* saved, bool infer) {
  AttnFwd f = {};
  const AttnDims d = f.d = attn_dims(plan, p);
  f.plan = plan; f.p = p; f.x = x; f.e = e; f.aggr = aggr;
  f.Wcat = c.take<float>((size_t)d.W2 * d.D);
  f.bcat = c.take<float>((size_t)d.W2);
  f.Pi = c.take<float>((size_t)d.N * d.W2);
  f.Pj = c.take<float>((size_t)d.N * d.W2);
  f.a = c.take<float>((size_t)d.E * d.H);
  f.Wq = c.take<float>(edge_z_wq_floats(d.W2) > edge_zx_wq_floats(d.W2) ? edge_z_wq_floats(d.W2)
                                                                        : edge_zx_wq_floats(d.W2));
  if (infer && attn_infer_fused(d)) {
    f.sv.alpha = c.take<float>((size_t)d.E * d.H);
    f.sv.S = c.take<float>((size_t)d.N * d.HHd);
    f.sv.ssum = c.take<float>((size_t)d.N * d.H);
  } else {
    if (infer) saved = c.take<float>(cgat_nodes_attention_saved_floats(d.N, d.E, d.H, d.Hd));
    if (!c.dry) f.sv = attn_saved(saved, d);
  }
  c.seal();
  f.r = attn_fwd_route(c.dry, d, infer, p, x, e, f.sv.Z, f.sv.S, aggr, f.Pi);
  return f;
}

// first conv layer split by operand: W_in [x_i;e;x_j] = W_i x_i + W_e e + W_j x_j.  The two node projections
// Pi = x W_i^T + bias, Pj = x W_j^T of the stacked weight W [W2, D]: two launches of the per-edge kernel, or the GEMM pair
// (which forms Pj whether or not the per-edge phase reads it)
struct NodeProj { float *Pi, *Pj, *Wq; };
// the plain product [N, C] -> [N, W2] of the per-edge kernel: no gathered addends, no logits; weight and output to be set
static EdgeZParams node_proj_params(const AttnDims& d, const float* x, float* Wq) {
  EdgeZParams z = {};
  z.e = x; z.lde = d.C; z.rows = d.N;
  z.Wq = Wq; z.W2 = d.W2; z.ldz = d.W2;
  z.H = d.H; z.Hd = d.Hd;
  return z;
}
static int node_projections(Ctx& c, const AttnDims& d, bool fast, bool need_Pj, const float* x, const float* W,
                            const float* bias, const NodeProj& o) {
  float *Pi = o.Pi, *Pj = o.Pj, *Wq = o.Wq;
  if (fast) {
    EdgeZParams z = node_proj_params(d, x, Wq);
    z.We = W; z.ldw = d.D; z.Pi = bias; z.Z = Pi;
    RUN(edge_z_launch(z, c.s));
    z.We = W + d.C + d.Ce; z.Pi = nullptr; z.Z = Pj;
    if (need_Pj) RUN(edge_z_launch(z, c.s));
    return CGAT_OK;
  }
  GemmParams g = gemm_params(d.N, d.W2, d.C, x, d.C, W, d.D, Pi, d.W2);
  g.bias = bias;
  CGAT_TRY(c.gemm(g));
  g = gemm_params(d.N, d.W2, d.C, x, d.C, W + d.C + d.Ce, d.D, Pj, d.W2);
  return c.gemm(g);
}

// the per-edge operands of both forwards: edge rows in slot order, W_e, the two gathered projections, the logits
static EdgeZParams attn_edge_params(const AttnFwd& f) {
  const AttnDims& d = f.d;
  EdgeZParams z = {};
  z.e = f.e; z.lde = d.Ce; z.perm = f.plan->dst_perm; z.rows = d.E;
  z.We = f.Wcat + d.C; z.ldw = d.D; z.Wq = f.Wq; z.W2 = d.W2;
  z.Pi = f.Pi; z.dsti = f.plan->dst_sorted; z.Pj = f.Pj; z.srci = f.plan->src_sorted; z.ld_add = d.W2; z.n_add_rows = d.N;
  z.wA = f.p->A_out_w; z.bA = f.p->A_out_b; z.H = d.H; z.Hd = d.Hd; z.a_out = f.a;
  return z;
}

// logits, softmax (the same launch as the training forward's), message columns summed straight into S
static int attn_fwd_edges_infer(Ctx& c, const AttnFwd& f) {
  const AttnDims& d = f.d;
  const cgat_plan* plan = f.plan;
  CGAT_CHECK_ARG(aligned16(f.e, f.Pi, f.Pj) && aligned16(f.p->A_out_w),
                 "nodes_attention_infer: edge_attr and MH_A.fc_out.weight must be 16-byte aligned");
  EdgeZParams z = attn_edge_params(f);   // Z stays null: nothing of size E x W2 is formed
  RUN(edge_logits_launch(z, c.s));
  RUN(seg_softmax_fwd_launch(f.a, nullptr, plan->dst_rowptr, d.N, d.H, 1e-16f, f.sv.alpha, f.sv.ssum, c.s));
  z.N = d.N; z.alpha = f.sv.alpha; z.rowptr = plan->dst_rowptr; z.S = f.sv.S;
  z.store = attn_bf16(d) ? Z_BF16 : Z_F32;
  RUN(edge_msg_wsum_launch(z, c.s));
  return CGAT_OK;
}

// Z[t] = W_e e[perm[t]] + Pi[dst[t]] + Pj[src[t]]      (x_i = x[edge_index[1]], x_j = x[edge_index[0]])
// and the attention logits a[t,h] = fc_out_A(leaky(zA)): one fused split-bf16 kernel at the benchmark widths,
// the generic GEMM + row-dot otherwise (and in the f32 arithmetic mode); then softmax and the weighted sum
// The form the last training forward left its saved buffer in, for the debug reader of the signs: that entry sees the
// buffer alone, not the operands whose alignment decided the form.
static const float* g_fwd_saved = nullptr;
static bool g_fwd_saved_bits = false;
static int attn_fwd_edges_train(Ctx& c, const AttnFwd& f) {
  const AttnDims& d = f.d;
  const cgat_plan* plan = f.plan;
  const cgat_attn_params* p = f.p;
  const AttnFwdRoute& r = f.r;
  const AttnSaved& sv = f.sv;
  if (!c.dry) { g_fwd_saved = sv.Z; g_fwd_saved_bits = r.z_bits; }
  if (!c.dry && edge_bf16_storage() && !r.z_bf16 && d.N > 0 && d.E > 0) {
    cgat_set_error("nodes_attention_forward: edge storage \"bf16\" is set but this layer (C %d, Ce %d, H %d, Hd %d, arithmetic "
                   "mode %d) has no bf16 form -- refusing to run it in fp32 storage under that label", d.C, d.Ce, d.H, d.Hd,
                   bilinear_mode());
    return CGAT_ERR_UNSUPPORTED;
  }
  const int zb = r.z_bf16 ? 1 : 0;
  EdgeZParams z = attn_edge_params(f);
  z.Z = sv.Z; z.ldz = d.W2; z.store = r.z_bits ? Z_BITS : r.z_bf16 ? Z_BF16 : Z_F32;
  if (r.zx) {
    z.x = f.x; z.ldx = d.C; z.Wj = f.Wcat + d.C + d.Ce;
    RUN(edge_zx_launch(z, c.s));
  } else if (r.fused_z) {
    if (r.z_bits) {   // the attention halves of the two projections into the holes of rows 0 .. 2 N - 1 (ZForm)
      Copy2DJobs j;
      j.n = 2;
      j.job[0] = {f.Pi, d.W2, sv.Z, d.W2, d.N, d.HHd};
      j.job[1] = {f.Pj, d.W2, sv.Z + (size_t)d.N * d.W2, d.W2, d.N, d.HHd};
      RUN(copy2d_multi_launch(j, c.s));
    }
    RUN(edge_z_launch(z, c.s));
  } else {
    GemmParams g = gemm_params(d.E, d.W2, d.Ce, f.e, d.Ce, f.Wcat + d.C, d.D, sv.Z, d.W2);
    g.a_rgather = plan->dst_perm;
    g.add1 = f.Pi; g.add1_idx = plan->dst_sorted;
    g.add2 = f.Pj; g.add2_idx = plan->src_sorted;
    g.ld_add = d.W2;
    CGAT_TRY(c.gemm(g));
    RUN(rowdot_launch(sv.Z, d.W2, CGAT_ACT_LEAKY, p->A_out_w, 0, nullptr, p->A_out_b, nullptr, d.E, d.H, d.Hd, f.a, c.s));
  }
  RUN(seg_softmax_fwd_launch(f.a, nullptr, plan->dst_rowptr, d.N, d.H, 1e-16f, sv.alpha, sv.ssum, c.s));
  // S[n,h,:] = sum_{t -> n} alpha[t,h] leaky(zM[t,h,:])  -- fc_out of MH_M commutes with the weighted sum
  RUN(seg_wsum_launch(zb ? reinterpret_cast<const float*>(reinterpret_cast<const __bf16*>(sv.Z) + d.HHd) : sv.Z + d.HHd, d.W2,
                      nullptr, sv.alpha, d.H, d.Hd, plan->dst_rowptr, d.N, d.HHd, CGAT_ACT_LEAKY, sv.S, d.HHd, c.s, 0, zb));
  return CGAT_OK;
}

// aggr = (1/H) [ sum_h S[:,h,:] fc_out_M[h]^T + ssum b ].  At the benchmark widths the H products run as
// H * Hd / 128 accumulating launches of the dense-layer kernel (K = 128 each; the generic f32 GEMM tile took 0.1 ms
// per head) -- or as one launch (attn_out_one_shape) -- and 1/H is applied by the bias product that closes the sum.
static int attn_fwd_out(Ctx& c, const AttnFwd& f) {
  const AttnDims& d = f.d;
  const cgat_attn_params* p = f.p;
  const AttnSaved& sv = f.sv;
  const int ncb_h = d.Hd / 128;
  if (attn_out_one_shape(d)) c.need((size_t)d.H * ncb_h * 24576 * sizeof(float));
  if (f.r.out_one) {
    // operand (a = block of head h, b = column in block, c = output) = M_out_w[h * C * Hd + c * Hd + 128 a + b]
    CGAT_TRY(prepare_T_planes_launch(p->M_out_w, c.scratch, ncb_h, 128, 1, d.Hd, /*alternate=*/1, c.s, nullptr, d.H,
                                     (long)d.C * d.Hd, (long)ncb_h * 24576));
    // (We == null: the image in the scratch region, all heads' blocks as one K = H * Hd operand)
    CGAT_TRY(edge_ge_launch(edge_ge_params(sv.S, d.HHd, 128, nullptr, 0, 0, (float*)c.scratch, d.HHd, f.aggr, d.C, d.N), c.s));
  } else if (f.r.out_fast) {
    for (int h = 0; h < d.H; ++h)
      for (int j = 0; j < ncb_h; ++j) {
        GemmParams g = gemm_params(d.N, d.C, 128, sv.S + (size_t)h * d.Hd + 128 * j, d.HHd,
                                   p->M_out_w + (size_t)h * d.C * d.Hd + 128 * j, d.Hd, f.aggr, d.C);
        g.beta = (h > 0 || j > 0) ? 1.f : 0.f;
        CGAT_TRY(c.gemm(g));
      }
  } else {
    for (int h = 0; h < d.H; ++h) {
      GemmParams g = gemm_params(d.N, d.C, d.Hd, sv.S + (size_t)h * d.Hd, d.HHd, p->M_out_w + (size_t)h * d.C * d.Hd,
                                 d.Hd, f.aggr, d.C);
      g.alpha = 1.f / d.H;
      g.beta = h > 0 ? 1.f : 0.f;
      CGAT_TRY(c.gemm(g));
    }
  }
  // + (1/H) sum_h ssum[n,h] * fc_out bias
  GemmParams g = gemm_params(d.N, d.C, d.H, sv.ssum, d.H, p->M_out_b, d.C, f.aggr, d.C);
  g.b_kmajor = 1;
  g.alpha = 1.f / d.H;
  g.beta = f.r.out_fast ? 1.f / d.H : 1.f;
  return c.gemm(g);
}

static int attn_forward_impl(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x, const float* e,
                             float* aggr, float* saved, bool infer = false) {
  const AttnFwd f = attn_fwd_carve(c, plan, p, x, e, aggr, saved, infer);
  CGAT_TRY(stack_in_weights(c, p, f.d, f.Wcat, f.bcat));
  CGAT_TRY(node_projections(c, f.d, f.r.proj_fast, !f.r.zx, x, f.Wcat, f.bcat, NodeProj{f.Pi, f.Pj, f.Wq}));
  CGAT_TRY(f.r.fused_infer ? attn_fwd_edges_infer(c, f) : attn_fwd_edges_train(c, f));
  CGAT_TRY(attn_fwd_out(c, f));
  return check_ws(c, "nodes_attention_forward");
}

// ---- the forward without grad on shell-indexed edge features: edge_attr[e] = table[index[e]], R rows ----
// W_e edge_attr[e] takes R distinct values, so Te = table W_e^T [R, W2] is formed once and the per-edge phase adds three
// gathered rows (edgeidx.hip): no per-edge product.  fp32 edge storage only -- the dense route rounds z to bf16 under
// edge storage "bf16" and this one would not, so the caller densifies there.  Every arithmetic mode: the per-edge phase
// has no matrix instruction, and the node-side products are the ones of attn_forward_impl.
static bool attn_infer_indexed_ok(const AttnDims& d, int R) {
  return !edge_bf16_storage() && d.N > 0 && d.E > 0 && edge_idx_ok(d.H, d.Hd, R);
}
struct AttnFwdIndexed {
  AttnFwd f;          // e == nullptr; a, sv.alpha, sv.S, sv.ssum: carve-outs, as in the fused inference
  const float* table;
  const int64_t* index;
  int R;
  float* Te;
};
// The saved buffer of the indexed training forward: alpha [E, H] | ssum [N, H], each on a 256-byte boundary of a 256-byte
// aligned buffer.  No Z and no S: the backward forms z again from the three rows, and S [N, H Hd] -- 4 % of the dense
// route's saved buffer by itself -- again with the forward's own launch of edge_idx_wsum on the same inputs (the same bits).
static size_t idx_round64(size_t n) { return (n + 63) / 64 * 64; }
extern "C" size_t cgat_nodes_attention_indexed_saved_floats(int32_t N, int32_t E, int32_t H, int32_t Hd) {
  (void)Hd;
  return idx_round64((size_t)E * H) + (size_t)N * H;
}
static AttnSaved attn_saved_indexed(float* saved, const AttnDims& d, float* S) {
  AttnSaved s;
  s.Z = nullptr;
  s.alpha = saved;
  s.S = S;           // a workspace carve-out of the pass
  s.ssum = s.alpha + idx_round64((size_t)d.E * d.H);
  return s;
}
// train: alpha and ssum live in the caller's saved buffer (`saved`; a dry pass has none) instead of the workspace; S stays
// a carve-out at the place the forward without grad has it (the same fc_out_M route, the same bits)
static AttnFwdIndexed attn_fwd_indexed_carve(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                             const float* table, int R, const int64_t* index, float* aggr,
                                             bool train = false, float* saved = nullptr) {
  AttnFwdIndexed g = {};
  AttnFwd& f = g.f;
  const AttnDims d = f.d = attn_dims(plan, p);
  f.plan = plan; f.p = p; f.x = x; f.aggr = aggr;
  g.table = table; g.index = index; g.R = R;
  f.Wcat = c.take<float>((size_t)d.W2 * d.D);
  f.bcat = c.take<float>((size_t)d.W2);
  f.Pi = c.take<float>((size_t)d.N * d.W2);
  f.Pj = c.take<float>((size_t)d.N * d.W2);
  g.Te = c.take<float>((size_t)R * d.W2);
  f.Wq = c.take<float>(2 * edge_z_wq_floats(d.W2));   // the images of W_i and W_j, made in one launch
  f.a = c.take<float>((size_t)d.E * d.H);            // the logits and alpha: all that grows with E
  if (train) {
    float* S = c.take<float>((size_t)d.N * d.HHd);
    if (!c.dry) f.sv = attn_saved_indexed(saved, d, S);
  } else {
    f.sv.alpha = c.take<float>((size_t)d.E * d.H);
    f.sv.S = c.take<float>((size_t)d.N * d.HHd);
    f.sv.ssum = c.take<float>((size_t)d.N * d.H);
  }
  c.seal();
  f.r = attn_fwd_route(c.dry, d, true, p, x, nullptr, nullptr, f.sv.S, aggr, f.Pi);   // proj_fast, out_fast, out_one
  return g;
}
// node_projections with the images of both weight slices from ONE preparation launch (the per-edge kernel's launches then
// only read them): the same products, one launch fewer per layer
static int node_projections_indexed(Ctx& c, const AttnFwdIndexed& g) {
  const AttnFwd& f = g.f;
  const AttnDims& d = f.d;
  if (!f.r.proj_fast) return node_projections(c, d, false, true, f.x, f.Wcat, f.bcat, NodeProj{f.Pi, f.Pj, f.Wq});
  const int ncb = d.W2 / 128;
  const long img = (long)edge_z_wq_floats(d.W2);
  // operand (a = column block, b = k, c = column in block) = W[(128 a + c) * D + b]; slice 1 starts C + Ce columns further
  if (mode_f16()) RUN(prepare_W_f16_launch(f.Wcat, f.Wq, ncb, 128l * d.D, 1, d.D, c.s, 2, d.C + d.Ce, img));
  else RUN(prepare_T_planes_launch(f.Wcat, f.Wq, ncb, 128l * d.D, 1, d.D, 0, c.s, nullptr, 2, d.C + d.Ce, img));
  EdgeZParams z = node_proj_params(d, f.x, f.Wq);   // We stays null: the images are made
  z.Pi = f.bcat; z.Z = f.Pi;
  RUN(edge_z_launch(z, c.s));
  z.Wq = f.Wq + img; z.Pi = nullptr; z.Z = f.Pj;
  RUN(edge_z_launch(z, c.s));
  return CGAT_OK;
}
// Te = table W_e^T (no bias: Pi carries it) on whichever engine takes R rows: a single-op small-row program below
// rowprog_max_rows(), the generic product of node_projections otherwise
static int indexed_edge_table(Ctx& c, const AttnFwdIndexed& g) {
  const AttnDims& d = g.f.d;
  return c.gemm(gemm_params(g.R, d.W2, d.Ce, g.table, d.Ce, g.f.Wcat + d.C, d.D, g.Te, d.W2));
}
// logits, softmax (the launch of every other forward: eps 1e-16, one rounded division), message columns summed into S
static int attn_fwd_edges_indexed(Ctx& c, const AttnFwdIndexed& g) {
  const AttnFwd& f = g.f;
  const AttnDims& d = f.d;
  const cgat_plan* plan = f.plan;
  CGAT_CHECK_ARG(aligned16(f.p->A_out_w), "nodes_attention_infer_indexed: MH_A.fc_out.weight must be 16-byte aligned");
  RUN(edge_idx_logits_launch(g.Te, g.R, g.index, plan->dst_perm, f.Pi, f.Pj, plan->src_sorted, d.W2, f.p->A_out_w,
                             f.p->A_out_b, d.H, d.Hd, plan->dst_rowptr, d.N, d.E, f.a, c.s));
  RUN(seg_softmax_fwd_launch(f.a, nullptr, plan->dst_rowptr, d.N, d.H, 1e-16f, f.sv.alpha, f.sv.ssum, c.s));
  RUN(edge_idx_wsum_launch(g.Te, g.R, g.index, plan->dst_perm, f.Pi, f.Pj, plan->src_sorted, d.W2, f.sv.alpha, d.H, d.Hd,
                           plan->dst_rowptr, d.N, d.E, f.sv.S, c.s));
  return CGAT_OK;
}
// fc_out_M for this route.  Where attn_fwd_out would take its one K = H * Hd launch, the same kernel runs once per head
// over that head's blocks of the same image (K = Hd each, accumulating into aggr): the accumulation chain of the one
// launch is the largest error of the whole forward, and the dense route leaves it wherever its
// own S is misaligned.  Everything else is attn_fwd_out.
static int attn_fwd_out_indexed(Ctx& c, const AttnFwd& f) {
  const AttnDims& d = f.d;
  if (!f.r.out_one) return attn_fwd_out(c, f);
  const int ncb_h = d.Hd / 128;
  c.need((size_t)d.H * ncb_h * 24576 * sizeof(float));
  CGAT_TRY(prepare_T_planes_launch(f.p->M_out_w, c.scratch, ncb_h, 128, 1, d.Hd, /*alternate=*/1, c.s, nullptr, d.H,
                                   (long)d.C * d.Hd, (long)ncb_h * 24576));
  for (int h = 0; h < d.H; ++h) {   // (We == null: head h's blocks of the image, K = Hd)
    EdgeGeParams g = edge_ge_params(f.sv.S + (size_t)h * d.Hd, d.HHd, 128, nullptr, 0, 0,
                                    reinterpret_cast<float*>(c.scratch) + (size_t)h * ncb_h * 24576, d.Hd, f.aggr, d.C, d.N);
    g.accumulate = h > 0 ? 1 : 0;
    CGAT_TRY(edge_ge_launch(g, c.s));
  }
  GemmParams g = gemm_params(d.N, d.C, d.H, f.sv.ssum, d.H, f.p->M_out_b, d.C, f.aggr, d.C);
  g.b_kmajor = 1;
  g.alpha = 1.f / d.H;
  g.beta = 1.f / d.H;
  return c.gemm(g);
}
// (train: the training forward -- the same steps, alpha and ssum kept for the backward)
static int attn_infer_indexed_impl(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                   const float* table, int R, const int64_t* index, float* aggr, bool train = false,
                                   float* saved = nullptr) {
  const AttnFwdIndexed g = attn_fwd_indexed_carve(c, plan, p, x, table, R, index, aggr, train, saved);
  const AttnFwd& f = g.f;
  CGAT_TRY(stack_in_weights(c, p, f.d, f.Wcat, f.bcat));
  CGAT_TRY(node_projections_indexed(c, g));
  CGAT_TRY(indexed_edge_table(c, g));
  CGAT_TRY(attn_fwd_edges_indexed(c, g));
  CGAT_TRY(attn_fwd_out_indexed(c, f));
  return check_ws(c, train ? "nodes_attention_forward_indexed" : "nodes_attention_infer_indexed");
}

// ---- the operand-split first layer's backward tail ----
// Everything downstream of the pre-activation gradient gZ[t, :] (destination-sorted slots) of the operand-split first
// layer: gradients wrt edge_attr, x, the stacked weight [W2, D] = [W_i | W_e | W_j] and its bias.  Shared by the
// scalar-attention backward (gZ from the fused segment kernel, column-blocked, Gi already summed) and the edge_hidden
// op (gZ row-major from autograd).
struct GzView {
  const float* ptr;   // element (t, 128 a + j) at ptr[t * ld + a * block + j]; nullptr: not stored, rebuilt from *rc
  long ld, block;
};
static EdgeRC edge_rc_make(const unsigned* mask, const float* ga, const float* alpha, const float* gS, const float* wA,
                           const int* dst, int H, int Hd) {
  EdgeRC rc = {};
  rc.mask = mask; rc.ga = ga; rc.alpha = alpha; rc.gS = gS; rc.wA = wA; rc.dst = dst;
  rc.H = H; rc.Hd = Hd; rc.HHd = H * Hd; rc.nw = 2 * H * Hd / 32;
  return rc;
}
struct EdgeTail {
  GzView gZ;
  float *Gi, *Gj;        // [N, W2] segment sums of gZ by destination / by source
  bool have_Gi;          // the caller has summed Gi already
  const float* Wcat;     // the stacked weight [W2, D]
  float *gWcat, *gbcat;
  float *Wq, *gw_ws;     // edge_z_wq_floats(W2) / edge_gw_ws_floats(E, W2) floats of workspace
  const float* scales;   // f16x3 mode, optional: device {max |gZ|, max |e|} -> the per-edge products run on two fp16 planes;
                         // [2..4] then take the node-side maxima {max |Gi|, max |Gj|, max |x|}
  const EdgeRC* rc;      // gZ was not stored; the per-edge launches and the source-side sum rebuild its rows (kernels.h)
  bool node_scales;      // stored gZ: form the node-side maxima by three passes (the rebuilt path's kernels fold them in)
  bool gw_force_six;     // debug entry only: grad W_e's launch keeps its six-pass form
  GwTe te;               // te.out != nullptr (the bit form of the saved buffer): grad W_e's reducer adds the edge part of
                         // grad fc_out_A to te.out (edgebwd.hip)
  const float *x, *e;
  float *g_x, *g_e;
};

enum NodeSide { NODE_KSPLIT, NODE_SMALL_ROWS, NODE_LAUNCHES, NODE_GEMM };
enum EdgeProduct { PRODUCT_KSPLIT, PRODUCT_LAUNCH, PRODUCT_GEMM };
struct TailRoute {
  // node-side products g_x = Gi W_i + Gj W_j, grad W_i = Gi^T x, grad W_j = Gj^T x.  Same shapes as the two edge kernels
  // (K = 1536 -> 128 outputs per row; K = rows -> 1536 x 128): reuse them on the row-major Gi / Gj when the node width is
  // 128 -- g_x as K-split slabs at few row tiles, as the small-row GEMM pair at a few hundred atoms -- generic GEMMs otherwise
  NodeSide node;
  int Sx, Se;           // K groups of the node-side / edge-side K = W2 -> 128 product (1: no split)
  bool node_scales;     // the node-side launches run on {max |Gi|, max |Gj|, max |x|} at scales[2..4] (f16x3)
  EdgeProduct ge, gw;   // grad edge_attr (K-split, per-edge launch or GEMM) and grad W_e (launch or GEMM)
};
static TailRoute tail_route(bool dry, const AttnDims& d, const EdgeTail& t) {
  TailRoute r = {};
  const bool maxima = t.scales && d.C == 128 && aligned16(t.x);
  r.node_scales = t.rc ? maxima
                       : maxima && t.node_scales && !dry && d.N > 0 && d.W2 % 128 == 0 && aligned16(t.Gi, t.Gj);
  // (K-split forms of the two K = W2 -> 128 products at few row tiles, edgebwd.hip: slabs in the scratch region)
  r.Sx = (!r.node_scales && d.C == 128) ? edge_ge_ksplit_groups(d.N, d.W2, false) : 1;
  r.Se = (!t.scales && d.Ce == 128) ? edge_ge_ksplit_groups(d.E, d.W2, t.rc != nullptr) : 1;
  const bool node_fast = !dry && d.N > 0 && edge_ge_dims(d.C, d.W2, d.W2, 128, d.C) && edge_gw_dims(d.C, d.W2, d.W2, 128) &&
                         aligned16(t.Gi, t.g_x, t.Gj, t.x) && d.N <= d.E;
  r.node = !node_fast ? NODE_GEMM : r.Sx > 1 ? NODE_KSPLIT : d.N <= rowprog_max_rows() ? NODE_SMALL_ROWS : NODE_LAUNCHES;
  const bool ge_fast = !dry && edge_ge_dims(d.Ce, d.W2, t.gZ.ld, t.gZ.block, d.Ce) && aligned16(t.gZ.ptr, t.g_e);
  r.ge = !ge_fast ? PRODUCT_GEMM : r.Se > 1 ? PRODUCT_KSPLIT : PRODUCT_LAUNCH;
  r.gw = (!dry && edge_gw_dims(d.Ce, d.W2, t.gZ.ld, t.gZ.block) && aligned16(t.gZ.ptr)) ? PRODUCT_LAUNCH : PRODUCT_GEMM;
  return r;
}
static long tail_xblock(const AttnDims& d, const EdgeTail& t) {   // block stride of a stored gZ; 0 = plain row-major
  return (t.gZ.ld == d.W2) ? 0 : t.gZ.block;
}

// segment sums of gZ: by destination (x_i side) unless the caller already has them, by source (x_j side)
static int tail_segment_sums(Ctx& c, const cgat_plan* plan, const AttnDims& d, const EdgeTail& t, const TailRoute& r) {
  const long xb = tail_xblock(d, t);
  float* ns = r.node_scales ? const_cast<float*>(t.scales) + 2 : nullptr;
  if (!t.have_Gi)
    RUN(seg_wsum_launch(t.gZ.ptr, d.W2, nullptr, nullptr, 0, 1, plan->dst_rowptr, d.N, d.W2, CGAT_ACT_NONE, t.Gi, d.W2, c.s,
                        xb));
  if (t.rc) {
    RUN(edge_gj_launch(*t.rc, plan->src_rowptr, plan->src_pos, d.N, d.W2, t.Gj, d.W2, c.s, ns ? ns + 1 : nullptr));
    return CGAT_OK;
  }
  RUN(seg_wsum_launch(t.gZ.ptr, d.W2, plan->src_pos, nullptr, 0, 1, plan->src_rowptr, d.N, d.W2, CGAT_ACT_NONE, t.Gj, d.W2,
                      c.s, xb));
  if (ns) {
    // stored-gZ path with scales (vector attention): the segment sums carry no maxima, three passes over [N, .] rows
    RUN(absmax_rows128_launch(t.Gi, 128, (int)((long)d.N * d.W2 / 128), ns, c.s));
    RUN(absmax_rows128_launch(t.Gj, 128, (int)((long)d.N * d.W2 / 128), ns + 1, c.s));
    RUN(absmax_rows128_launch(t.x, d.C, d.N, ns + 2, c.s));
  }
  return CGAT_OK;
}

static int tail_gx_gemm_pair(Ctx& c, const AttnDims& d, const EdgeTail& t) {   // g_x = Gi W_i + Gj W_j
  GemmParams g = gemm_params(d.N, d.C, d.W2, t.Gi, d.W2, t.Wcat, d.D, t.g_x, d.C);
  g.b_kmajor = 1;
  CGAT_TRY(c.gemm(g));
  g = gemm_params(d.N, d.C, d.W2, t.Gj, d.W2, t.Wcat + d.C + d.Ce, d.D, t.g_x, d.C);
  g.b_kmajor = 1;
  g.beta = 1.f;
  return c.gemm(g);
}
static int tail_node_products(Ctx& c, const AttnDims& d, const EdgeTail& t, const TailRoute& r) {
  const float* ns = r.node_scales ? t.scales + 2 : nullptr;
  const float* Wj = t.Wcat + d.C + d.Ce;
  // the node-side records: g_x (+)= G W for G = Gi, Gj [N, W2] row-major, and grad W = G^T x
  EdgeGeParams gi = edge_ge_params(t.Gi, d.W2, 128, t.Wcat, d.D, 1, t.Wq, d.W2, t.g_x, d.C, d.N);
  EdgeGeParams gj = edge_ge_params(t.Gj, d.W2, 128, Wj, d.D, 1, t.Wq, d.W2, t.g_x, d.C, d.N);
  EdgeGwParams wi = edge_gw_params(t.Gi, d.W2, 128, t.x, d.C, nullptr, d.N, d.W2, t.gw_ws, t.gWcat, d.D);
  EdgeGwParams wj = edge_gw_params(t.Gj, d.W2, 128, t.x, d.C, nullptr, d.N, d.W2, t.gw_ws, t.gWcat + d.C + d.Ce, d.D);
  if (ns) { gi.amax = wi.gmax = ns; gj.amax = wj.gmax = ns + 1; wi.emax = wj.emax = ns + 2; }
  if (r.Sx > 1) c.need((size_t)2 * r.Sx * d.N * 128 * sizeof(float));
  if (r.node == NODE_GEMM) {
    CGAT_TRY(tail_gx_gemm_pair(c, d, t));
    GemmParams g = gemm_params(d.W2, d.C, d.N, t.Gi, d.W2, t.x, d.C, t.gWcat, d.D);
    g.a_kmajor = 1; g.b_kmajor = 1;
    CGAT_TRY(c.gemm(g, true));
    g = gemm_params(d.W2, d.C, d.N, t.Gj, d.W2, t.x, d.C, t.gWcat + d.C + d.Ce, d.D);
    g.a_kmajor = 1; g.b_kmajor = 1;
    CGAT_TRY(c.gemm(g, true));
    return c.colsum(t.Gi, d.W2, d.N, d.W2, t.gbcat, 1.f);
  }
  if (r.node == NODE_KSPLIT) {
    // g_x = Gi W_i + Gj W_j as 2 Sx slabs, added in order (round 6: 2 x 100 us of fp64 small-row products -> 3 launches)
    float* sl = (float*)c.scratch;
    gi.slabs = sl; gj.slabs = sl + (size_t)r.Sx * d.N * 128;
    gi.S = gj.S = r.Sx;
    RUN(edge_ge_launch(gi, c.s));
    RUN(edge_ge_launch(gj, c.s));
    RUN(sum_slabs_launch(sl, 2 * r.Sx, (long)d.N * 128, t.g_x, (long)d.N * 128, c.s));
  } else if (r.node == NODE_SMALL_ROWS) {
    // a few hundred atoms: the 256-row tiles of the per-edge kernel are 5 workgroups walking K = 1536 (91 us a launch
    // at 1 280 atoms); as 16 x 16 wave tiles with the k range dealt over a workgroup's waves the chip is full
    CGAT_TRY(tail_gx_gemm_pair(c, d, t));
  } else {
    gj.accumulate = 1;
    RUN(edge_ge_launch(gi, c.s));
    RUN(edge_ge_launch(gj, c.s));
  }
  RUN(edge_gw_launch(wi, c.s));
  RUN(edge_gw_launch(wj, c.s));
  return c.colsum(t.Gi, d.W2, d.N, d.W2, t.gbcat, 1.f);
}

// grad edge_attr[perm[t]] = gZ[t] @ W_e: split-bf16 kernel at the benchmark widths, generic GEMM otherwise
static int tail_edge_ge(Ctx& c, const cgat_plan* plan, const AttnDims& d, const EdgeTail& t, const TailRoute& r) {
  if (r.Se > 1) c.need((size_t)r.Se * d.E * 128 * sizeof(float));
  EdgeGeParams g = edge_ge_params(t.gZ.ptr, t.gZ.ld, t.gZ.block, t.Wcat + d.C, d.D, 1, t.Wq, d.W2, t.g_e, d.Ce, d.E);
  g.rc = t.rc; g.scatter = plan->dst_perm;
  if (r.ge == PRODUCT_KSPLIT) {
    g.slabs = (float*)c.scratch; g.S = r.Se;
    RUN(edge_ge_launch(g, c.s));
    RUN(sum_slabs_launch(g.slabs, r.Se, (long)d.E * 128, t.g_e, (long)d.E * 128, c.s));
  } else if (r.ge == PRODUCT_LAUNCH) {
    g.amax = t.scales;
    RUN(edge_ge_launch(g, c.s));
  } else {
    GemmParams g = gemm_params(d.E, d.Ce, d.W2, t.gZ.ptr, t.gZ.ld, t.Wcat + d.C, d.D, t.g_e, d.Ce);
    g.a_block = tail_xblock(d, t);
    g.b_kmajor = 1;
    g.c_scatter = plan->dst_perm;
    CGAT_TRY(c.gemm(g));
  }
  return CGAT_OK;
}
// grad W_e = gZ^T @ e[perm]
static int tail_edge_gw(Ctx& c, const cgat_plan* plan, const AttnDims& d, const EdgeTail& t, const TailRoute& r) {
  if (r.gw == PRODUCT_LAUNCH) {
    EdgeGwParams w = edge_gw_params(t.gZ.ptr, t.gZ.ld, t.gZ.block, t.e, d.Ce, plan->dst_perm, d.E, d.W2, t.gw_ws,
                                    t.gWcat + d.C, d.D);
    w.rc = t.rc; w.force_six = t.gw_force_six;
    if (t.scales) { w.gmax = t.scales; w.emax = t.scales + 1; }
    if (t.te.out) w.te = &t.te;
    RUN(edge_gw_launch(w, c.s));
    return CGAT_OK;
  }
  CGAT_CHECK_ARG(!t.te.out, "nodes_attention_backward: the bit form of the saved buffer needs grad W_e's per-edge launch");
  GemmParams g = gemm_params(d.W2, d.Ce, d.E, t.gZ.ptr, t.gZ.ld, t.e, d.Ce, t.gWcat + d.C, d.D);
  g.a_block = tail_xblock(d, t);
  g.a_kmajor = 1; g.b_kmajor = 1;
  g.b_kgather = plan->dst_perm;
  return c.gemm(g, true);
}
static int tail_edge_products(Ctx& c, const cgat_plan* plan, const AttnDims& d, const EdgeTail& t, const TailRoute& r) {
  if (!c.dry && t.rc)
    CGAT_CHECK_ARG(r.ge != PRODUCT_GEMM && r.gw != PRODUCT_GEMM && t.have_Gi,
                   "nodes_attention_backward: the rebuilt-gZ path needs the split per-edge kernels");
  CGAT_TRY(tail_edge_ge(c, plan, d, t, r));
  return tail_edge_gw(c, plan, d, t, r);
}

static int edge_first_layer_backward_tail(Ctx& c, const cgat_plan* plan, const AttnDims& d, const EdgeTail& t) {
  const TailRoute r = tail_route(c.dry, d, t);
  // Order: the HBM-bound kernels (segment sums, node-side products over the 0.5-GB Gi / Gj) first, the two matrix-bound
  // per-edge products last -- the caller's side stream runs the matrix-bound dT launch on half of the chip meanwhile,
  // and a matrix-bound kernel beside it takes 2.9x as long (edge_ge 1.3 -> 3.7 ms) where an HBM-bound one loses little.
  CGAT_TRY(tail_segment_sums(c, plan, d, t, r));
  CGAT_TRY(tail_node_products(c, d, t, r));
  return tail_edge_products(c, plan, d, t, r);
}

// ---- backward ----
struct AttnBwd {
  AttnDims d;
  const cgat_plan* plan;
  const cgat_attn_params* p;
  const cgat_attn_grads* gr;
  const float *x, *e, *g_aggr;
  float *g_x, *g_e;
  float *Wcat, *gWcat, *gbcat, *gS, *gs, *gas, *tt, *ga, *gZ, *partial, *Gi, *Gj, *Wq, *gw_ws;
  float* scales;      // [0] max |gZ|, [1] max |edge_attr| (f16x3 mode), [2..4] max |Gi|, |Gj|, |x|
  int chunks;         // workgroups of the fused segment kernel
  long gzb, gz_ld;    // gZ is stored in 128-column blocks [W2/128][E][128] when the width allows: the weight-gradient
                      // product gZ^T @ e then streams each block contiguously instead of 512-byte pieces at a 6 KB stride
  AttnSaved sv;
  EdgeRC rc;
  AttnBwdRoute r;
};
static AttnBwd attn_bwd_carve(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x, const float* e,
                              const float* saved, const float* g_aggr, float* g_x, float* g_e, const cgat_attn_grads* gr) {
  AttnBwd b = {};
  const AttnDims d = b.d = attn_dims(plan, p);
  b.plan = plan; b.p = p; b.gr = gr; b.x = x; b.e = e; b.g_aggr = g_aggr; b.g_x = g_x; b.g_e = g_e;
  b.chunks = edge_seg_bwd_chunks(d.N);
  if (!c.dry) b.sv = attn_saved(const_cast<float*>(saved), d);
  b.Wcat = c.take<float>((size_t)d.W2 * d.D);
  b.r = attn_bwd_route(c.dry, d, p, x, e, saved, b.sv.S, b.Wcat);
  b.gWcat = c.take<float>((size_t)d.W2 * d.D);
  b.gbcat = c.take<float>((size_t)d.W2);
  b.gS = c.take<float>((size_t)d.N * d.HHd);
  b.gs = c.take<float>((size_t)d.N * d.H);
  b.gas = mode_split() ? c.take<float>((size_t)d.N * d.C) : nullptr;   // g_aggr / H (fast fc_out path)
  b.tt = c.take<float>((size_t)d.E * d.H);
  b.ga = c.take<float>((size_t)d.E * d.H);
  b.gZ = c.take<float>(b.r.rc ? (size_t)d.E * (d.W2 / 32) : (size_t)d.E * d.W2);
  b.partial = c.take<float>((size_t)b.chunks * d.HHd);
  b.Gi = c.take<float>((size_t)d.N * d.W2);
  b.Gj = c.take<float>((size_t)d.N * d.W2);
  b.Wq = c.take<float>(edge_z_wq_floats(d.W2));
  b.gw_ws = c.take<float>(edge_gw_ws_floats(d.E, d.W2));
  b.scales = c.take<float>(64);
  c.seal();
  b.gzb = (d.W2 % 128 == 0) ? (long)d.E * 128 : 0;
  b.gz_ld = b.gzb ? 128 : d.W2;
  if (b.r.rc && !c.dry)
    b.rc = edge_rc_make(reinterpret_cast<const unsigned*>(b.gZ), b.ga, b.sv.alpha, b.gS, p->A_out_w, plan->dst_sorted, d.H, d.Hd);
  return b;
}

// The per-head second layer of the message network: gS = (1/H) g_aggr fc_out_M[h], grad fc_out_M, gs and grad bias_M.
// At the benchmark widths (C = 128, Hd a multiple of 128): the input gradients on the dense-layer kernel (K = 128 -> Hd
// outputs per head), the H * Hd / 128 weight-gradient blocks in one batched launch of the rows kernel (rowsdw.hip); 1/H
// is folded into one scaled copy of g_aggr.
static int attn_bwd_out_layer(Ctx& c, const AttnBwd& b) {
  const AttnDims& d = b.d;
  const cgat_attn_params* p = b.p;
  const float invH = 1.f / d.H;
  if (attn_bwd_out_shape(d)) {
    c.need(rows_dw128_batch_ws_bytes(d.H * (d.Hd / 128), d.N));
    c.need(linear128_ws_bytes(d.Hd));
    c.need((size_t)d.H * linear128_heads_image_floats(d.Hd) * sizeof(float));
  }
  if (b.r.out_fast) {
    RUN(scale_launch(b.g_aggr, invH, b.gas, (long)d.N * d.C, c.s));
    if (b.r.out_heads_one) {
      // all heads in one launch pair (round 6): head h reads the same gas, its weight at + h * C * Hd, writes gS + h * Hd
      Linear128Params l = linear128_params(b.gas, d.C, p->M_out_w, 1, d.Hd, b.gS, d.HHd, d.N, d.Hd);
      l.heads = d.H; l.s_w = (long)d.C * d.Hd; l.s_out = d.Hd;
      CGAT_TRY(linear128_heads_launch(l, c.scratch, c.s));
    } else {
      for (int h = 0; h < d.H; ++h) {   // gS[:,h,:] = gas @ fc_out_M[h]
        GemmParams g = gemm_params(d.N, d.Hd, d.C, b.gas, d.C, p->M_out_w + (size_t)h * d.C * d.Hd, d.Hd,
                                   b.gS + (size_t)h * d.Hd, d.HHd);
        g.b_kmajor = 1;
        CGAT_TRY(c.gemm(g));
      }
    }
    if (!c.dry) {   // grad fc_out_M[h] = gas^T S[:,h,:]
      DwBatchDesc w;
      memset(&w, 0, sizeof(w));
      w.rows = d.N; w.ldg = d.C; w.ldx = d.HHd; w.ldo = d.Hd;
      for (int h = 0; h < d.H; ++h)
        for (int j = 0; j < d.Hd / 128; ++j)
          w.it[w.n++] = {b.gas, b.sv.S + (size_t)h * d.Hd + 128 * j, b.gr->M_out_w + (size_t)h * d.C * d.Hd + 128 * j, nullptr};
      CGAT_TRY(rows_dw128_batch_launch(w, c.scratch, c.scratch_bytes, c.s));
    }
  } else {
    for (int h = 0; h < d.H; ++h) {
      const float* Wo = p->M_out_w + (size_t)h * d.C * d.Hd;
      // gS[:,h,:] = (1/H) g_aggr @ fc_out_M[h]
      GemmParams g = gemm_params(d.N, d.Hd, d.C, b.g_aggr, d.C, Wo, d.Hd, b.gS + (size_t)h * d.Hd, d.HHd);
      g.b_kmajor = 1;
      g.alpha = invH;
      CGAT_TRY(c.gemm(g));
      // grad fc_out_M[h] = (1/H) g_aggr^T S[:,h,:]
      g = gemm_params(d.C, d.Hd, d.N, b.g_aggr, d.C, b.sv.S + (size_t)h * d.Hd, d.HHd,
                      b.gr->M_out_w + (size_t)h * d.C * d.Hd, d.Hd);
      g.a_kmajor = 1; g.b_kmajor = 1;
      g.alpha = invH;
      CGAT_TRY(c.gemm(g, true));
    }
  }
  // gs[n,h] = (1/H) g_aggr[n,:] . bias_M[h,:]
  GemmParams g = gemm_params(d.N, d.H, d.C, b.g_aggr, d.C, p->M_out_b, d.C, b.gs, d.H);
  g.alpha = invH;
  CGAT_TRY(c.gemm(g));
  // grad bias_M[h,c] = (1/H) sum_n ssum[n,h] g_aggr[n,c]
  g = gemm_params(d.H, d.C, d.N, b.sv.ssum, d.H, b.g_aggr, d.C, b.gr->M_out_b, d.C);
  g.a_kmajor = 1; g.b_kmajor = 1;
  g.alpha = invH;
  return c.gemm(g, true);
}

// g_alpha, softmax backward, gZ, the destination-side segment sum Gi and the partial sums for
// grad fc_out_A, all per whole destination segment in one pass (edge_seg_bwd_kernel); then the f16x3 maxima and grad fc_out_A
static int attn_bwd_segments(Ctx& c, const AttnBwd& b) {
  const AttnDims& d = b.d;
  const AttnBwdRoute& r = b.r;
  if (!c.dry && d.N > 0) {
    if (edge_bf16_storage() && !r.z_bf16) {
      cgat_set_error("nodes_attention_backward: edge storage \"bf16\" is set but this layer has no bf16 form");
      return CGAT_ERR_UNSUPPORTED;
    }
    CGAT_CHECK_ARG(!r.z_bits || (r.rc && r.vec), "nodes_attention_backward: the bit form of the saved buffer without its route");
    // (attn_bwd_tail lends tt to grad W_e's reducer as 4 H Hd doubles)
    CGAT_CHECK_ARG(!r.z_bits || ((size_t)d.E * d.H * sizeof(float) >= (size_t)4 * d.HHd * sizeof(double) &&
                                 (((uintptr_t)b.tt) & 7) == 0),
                   "nodes_attention_backward: the bit form needs %d doubles of scratch in tt", 4 * d.HHd);
    if (r.rc)
      CGAT_CHECK_ARG(r.vec && aligned16(b.e),
                     "nodes_attention_backward: saved, edge_attr and MH_A.fc_out.weight must be 16-byte aligned at these widths");
    unsigned* mask = r.rc ? reinterpret_cast<unsigned*>(b.gZ) : nullptr;
    float* gzmax = r.have_scales ? b.scales : nullptr;
    // [2] max |Gi|, [3] max |Gj|, [4] max |x|: with them the node-side products run in the fp16 form too (rebuilt path)
    float* gimax = (r.have_scales && r.rc) ? b.scales + 2 : nullptr;
    CGAT_TRY(edge_seg_bwd_launch(b.sv.Z, b.gZ, b.gzb, b.sv.alpha, b.gS, b.gs, b.plan->dst_rowptr, b.p->A_out_w, d.N, d.H, d.Hd,
                                 b.tt, b.ga, b.Gi, b.partial, gzmax, mask, gimax, r.vec, r.z_bf16_six, r.z_bf16, r.rc,
                                 r.have_scales, c.s, r.z_bits ? b.plan->src_sorted : nullptr));
  }
  if (r.have_scales) RUN(absmax_rows128_launch(b.e, d.Ce, d.E, b.scales + 1, c.s));
  if (r.have_scales && r.rc && d.C == 128 && aligned16(b.x)) RUN(absmax_rows128_launch(b.x, d.C, d.N, b.scales + 4, c.s));
  CGAT_TRY(c.colsum(b.ga, d.H, d.E, d.H, b.gr->A_out_b, 1.f));
  return c.colsum(b.partial, d.HHd, d.N > 0 ? b.chunks : 0, d.HHd, b.gr->A_out_w, 1.f);
}

static EdgeTail attn_bwd_tail(const AttnBwd& b) {
  EdgeTail t = {};
  t.gZ = {b.r.rc ? nullptr : b.gZ, b.gz_ld, b.gzb};
  t.Gi = b.Gi; t.Gj = b.Gj; t.have_Gi = true;
  t.Wcat = b.Wcat; t.gWcat = b.gWcat; t.gbcat = b.gbcat;
  t.Wq = b.Wq; t.gw_ws = b.gw_ws;
  t.scales = b.r.have_scales ? b.scales : nullptr;
  t.rc = b.r.rc ? &b.rc : nullptr;
  t.x = b.x; t.e = b.e; t.g_x = b.g_x; t.g_e = b.g_e;
  // (tt, E * H floats on a 256-byte boundary, is dead behind the softmax backward: the 4 H Hd doubles of the reducer's
  // quarter sums fit from E = 2048 on -- attn_bwd_segments checks both)
  if (b.r.z_bits && b.gr) t.te = {b.Wcat + b.d.C, b.d.D, reinterpret_cast<double*>(b.tt), b.gr->A_out_w};   // (no gr: the route query)
  return t;
}

static int attn_bwd_scatter_grads(Ctx& c, const AttnBwd& b) {
  const AttnDims& d = b.d;
  Copy2DJobs j;
  j.n = 4;
  j.job[0] = {b.gWcat, d.D, b.gr->A_in_w, d.D, d.HHd, d.D};
  j.job[1] = {b.gWcat + (size_t)d.HHd * d.D, d.D, b.gr->M_in_w, d.D, d.HHd, d.D};
  j.job[2] = {b.gbcat, d.HHd, b.gr->A_in_b, d.HHd, 1, d.HHd};
  j.job[3] = {b.gbcat + d.HHd, d.HHd, b.gr->M_in_b, d.HHd, 1, d.HHd};
  RUN(copy2d_multi_launch(j, c.s));
  return CGAT_OK;
}

static int attn_backward_impl(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x, const float* e,
                              const float* saved, const float* g_aggr, float* g_x, float* g_e,
                              const cgat_attn_grads* gr) {
  const AttnBwd b = attn_bwd_carve(c, plan, p, x, e, saved, g_aggr, g_x, g_e, gr);
  CGAT_TRY(stack_in_weights(c, p, b.d, b.Wcat, nullptr));
  CGAT_TRY(attn_bwd_out_layer(c, b));
  CGAT_TRY(attn_bwd_segments(c, b));
  CGAT_TRY(edge_first_layer_backward_tail(c, plan, b.d, attn_bwd_tail(b)));
  CGAT_TRY(attn_bwd_scatter_grads(c, b));
  return check_ws(c, "nodes_attention_backward");
}

// ---- the backward of the indexed training forward (reference CGAT.py:319-329 + PyG aggregate, on edge_attr = table[index]) ----
// No Z and no S were stored: Pi, Pj, Te and then S are formed again by the forward's launches on the forward's inputs (the
// same bits) and the segment backward forms z from them (edgeidx.hip).  grad edge_attr and grad W_e are linear in e, and e takes R
// values: with gT[r, :] = the sum of the gZ rows of class r, grad table = gT W_e and grad W_e = gT^T table -- two products
// over R rows in place of the two per-edge products.  The node-side products run without the f16x3 maxima (this segment
// backward folds none): in that mode they take the form that needs none, bf16x6.
static bool attn_train_indexed_ok(const AttnDims& d, int R) {
  return edge_storage() == 0 && d.N > 0 && d.E > 0 && edge_idx_train_ok(d.H, d.Hd, R);
}
struct AttnClassPlan {          // built once per (index, plan) by cgat_indexed_class_plan
  const int32_t *cls_pos, *piece_rowptr, *piece_start;
};
struct AttnBwdIndexed {
  AttnBwd b;                    // e == nullptr, g_e == nullptr; gZ: the mask words
  AttnFwdIndexed g;             // the recomputation: Wcat, bcat, Pi, Pj, Te, Wq
  AttnClassPlan cls;
  float *g_table, *gT, *cpart;
};
static AttnBwdIndexed attn_bwd_indexed_carve(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                             const float* table, int R, const int64_t* index, const AttnClassPlan& cls,
                                             const float* saved, const float* g_aggr, float* g_x, float* g_table,
                                             const cgat_attn_grads* gr) {
  AttnBwdIndexed q = {};
  AttnBwd& b = q.b;
  AttnFwd& f = q.g.f;
  const AttnDims d = b.d = f.d = attn_dims(plan, p);
  b.plan = f.plan = plan; b.p = f.p = p; b.gr = gr; b.x = f.x = x; b.g_aggr = g_aggr; b.g_x = g_x;
  q.g.table = table; q.g.index = index; q.g.R = R; q.cls = cls; q.g_table = g_table;
  b.chunks = edge_idx_bwd_chunks(d.N);
  b.Wcat = f.Wcat = c.take<float>((size_t)d.W2 * d.D);
  float* S = c.take<float>((size_t)d.N * d.HHd);                      // formed again by the forward's launch
  if (!c.dry) b.sv = attn_saved_indexed(const_cast<float*>(saved), d, S);
  f.bcat = c.take<float>((size_t)d.W2);
  b.gWcat = c.take<float>((size_t)d.W2 * d.D);
  b.gbcat = c.take<float>((size_t)d.W2);
  b.gS = c.take<float>((size_t)d.N * d.HHd);
  b.gs = c.take<float>((size_t)d.N * d.H);
  b.gas = mode_split() ? c.take<float>((size_t)d.N * d.C) : nullptr;
  b.tt = c.take<float>((size_t)d.E * d.H);
  b.ga = c.take<float>((size_t)d.E * d.H);
  b.gZ = c.take<float>((size_t)d.E * (d.W2 / 32));                    // the sign words, EdgeRC's layout
  b.partial = c.take<float>((size_t)b.chunks * d.HHd);
  b.Gi = c.take<float>((size_t)d.N * d.W2);
  b.Gj = c.take<float>((size_t)d.N * d.W2);
  f.Pi = c.take<float>((size_t)d.N * d.W2);
  f.Pj = c.take<float>((size_t)d.N * d.W2);
  q.g.Te = c.take<float>((size_t)R * d.W2);
  b.Wq = f.Wq = c.take<float>(2 * edge_z_wq_floats(d.W2));            // the projections' images, then the tail's
  b.gw_ws = c.take<float>(edge_gw_ws_floats(d.N, d.W2));              // (the node-side weight gradients: N rows)
  q.gT = c.take<float>((size_t)R * d.W2);
  q.cpart = c.take<float>((size_t)edge_idx_class_pieces(d.E, R) * d.W2);
  c.seal();
  b.r = attn_bwd_route(c.dry, d, p, x, nullptr, saved, b.sv.S, b.Wcat);   // out_fast, out_heads_one
  f.r = attn_fwd_route(c.dry, d, true, p, x, nullptr, nullptr, b.sv.S, nullptr, f.Pi);   // proj_fast, as the forward
  if (!c.dry)
    b.rc = edge_rc_make(reinterpret_cast<const unsigned*>(b.gZ), b.ga, b.sv.alpha, b.gS, p->A_out_w, plan->dst_sorted, d.H, d.Hd);
  return q;
}
// tt, ga, the sign words, Gi and the partial rows of grad fc_out_A.weight on recomputed z; then grad fc_out_A
static int attn_bwd_segments_indexed(Ctx& c, const AttnBwdIndexed& q) {
  const AttnBwd& b = q.b;
  const AttnFwd& f = q.g.f;
  const AttnDims& d = b.d;
  CGAT_CHECK_ARG(c.dry || aligned16(b.p->A_out_w, b.sv.alpha),
                 "nodes_attention_backward_indexed: saved and MH_A.fc_out.weight must be 16-byte aligned");
  RUN(edge_idx_bwd_launch(q.g.Te, q.g.R, q.g.index, b.plan->dst_perm, f.Pi, f.Pj, b.plan->src_sorted, d.W2, b.sv.alpha, b.gS,
                          b.gs, b.p->A_out_w, d.H, d.Hd, b.plan->dst_rowptr, d.N, d.E, b.tt, b.ga,
                          reinterpret_cast<unsigned*>(b.gZ), b.Gi, b.partial, c.s));
  CGAT_TRY(c.colsum(b.ga, d.H, d.E, d.H, b.gr->A_out_b, 1.f));
  return c.colsum(b.partial, d.HHd, b.chunks, d.HHd, b.gr->A_out_w, 1.f);
}
static EdgeTail attn_bwd_tail_indexed(const AttnBwdIndexed& q) {
  const AttnBwd& b = q.b;
  EdgeTail t = {};
  t.gZ = {nullptr, b.d.W2, 0};
  t.Gi = b.Gi; t.Gj = b.Gj; t.have_Gi = true;
  t.Wcat = b.Wcat; t.gWcat = b.gWcat; t.gbcat = b.gbcat;
  t.Wq = b.Wq; t.gw_ws = b.gw_ws;
  t.scales = nullptr;            // no maxima on this route: the node-side products in the form that needs none
  t.rc = &b.rc;
  t.x = b.x; t.g_x = b.g_x;
  return t;
}
// gT, then grad table = gT W_e and grad W_e = gT^T table (into the W_e columns of gWcat)
static int attn_bwd_class_products(Ctx& c, const AttnBwdIndexed& q) {
  const AttnBwd& b = q.b;
  const AttnDims& d = b.d;
  RUN(edge_idx_class_sum_launch(b.rc, q.cls.piece_rowptr, q.cls.piece_start, q.cls.cls_pos, q.g.R, d.E, d.W2, q.cpart, q.gT,
                                c.s));
  GemmParams g = gemm_params(q.g.R, d.Ce, d.W2, q.gT, d.W2, b.Wcat + d.C, d.D, q.g_table, d.Ce);
  g.b_kmajor = 1;
  CGAT_TRY(c.gemm(g));
  g = gemm_params(d.W2, d.Ce, q.g.R, q.gT, d.W2, q.g.table, d.Ce, b.gWcat + d.C, d.D);
  g.a_kmajor = 1; g.b_kmajor = 1;
  return c.gemm(g);
}
static int attn_backward_indexed_impl(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                      const float* table, int R, const int64_t* index, const AttnClassPlan& cls,
                                      const float* saved, const float* g_aggr, float* g_x, float* g_table,
                                      const cgat_attn_grads* gr) {
  const AttnBwdIndexed q = attn_bwd_indexed_carve(c, plan, p, x, table, R, index, cls, saved, g_aggr, g_x, g_table, gr);
  const AttnBwd& b = q.b;
  CGAT_TRY(stack_in_weights(c, p, b.d, b.Wcat, q.g.f.bcat));
  CGAT_TRY(node_projections_indexed(c, q.g));
  CGAT_TRY(indexed_edge_table(c, q.g));
  RUN(edge_idx_wsum_launch(q.g.Te, R, index, plan->dst_perm, q.g.f.Pi, q.g.f.Pj, plan->src_sorted, b.d.W2, b.sv.alpha, b.d.H,
                           b.d.Hd, plan->dst_rowptr, b.d.N, b.d.E, b.sv.S, c.s));   // S, not saved: the forward's bits
  CGAT_TRY(attn_bwd_out_layer(c, b));
  CGAT_TRY(attn_bwd_segments_indexed(c, q));
  const EdgeTail t = attn_bwd_tail_indexed(q);
  const TailRoute r = tail_route(c.dry, b.d, t);
  RUN(edge_gj_launch(b.rc, plan->src_rowptr, plan->src_pos, b.d.N, b.d.W2, b.Gj, b.d.W2, c.s, nullptr));
  CGAT_TRY(tail_node_products(c, b.d, t, r));
  CGAT_TRY(attn_bwd_class_products(c, q));
  CGAT_TRY(attn_bwd_scatter_grads(c, b));
  return check_ws(c, "nodes_attention_backward_indexed");
}

// =======================================================================================
// edge_hidden: H[t, :] = LeakyReLU( W_in [x_i ; edge_attr ; x_j] + b ) for all heads of any number of message networks
// stacked in W_in [W2, D], rows in destination-sorted slot order t (plan->dst_perm).  The first layer of
// MultiHeadNetwork (CGAT.py:96,105-108) with the operand split; used by the vector-attention variants, whose second
// layers / channel-wise softmax then run on H (CGAT.py:286-290, 319-329).
// =======================================================================================
static AttnDims hidden_dims(const cgat_plan* plan, int C, int Ce, int W2) {
  AttnDims d;
  d.N = plan->N; d.E = plan->E; d.C = C; d.Ce = Ce; d.H = 1; d.Hd = W2 / 2; d.D = 2 * C + Ce; d.HHd = W2 / 2; d.W2 = W2;
  return d;
}

// ---- routes of the two passes: decided once from the dims, the arithmetic mode and the alignment of the operands, by
// the carve functions that the real pass, its dry pass and cgat_debug_edge_hidden_route all go through ----
struct HiddenFwd {
  float *Pi, *Pj, *Wq;
  bool fast;          // the node projections and the per-edge phase on the split per-edge kernel (else: the GEMM engine)
};
static HiddenFwd hidden_fwd_carve(Ctx& c, const AttnDims& d, const float* b_in, const float* x, const float* e,
                                  const float* Hout) {
  HiddenFwd f = {};
  f.Pi = c.take<float>((size_t)d.N * d.W2);
  f.Pj = c.take<float>((size_t)d.N * d.W2);
  f.Wq = c.take<float>(edge_z_wq_floats(d.W2));
  c.seal();
  f.fast = !c.dry && d.N > 0 && d.W2 % 256 == 0 && d.C == 128 && edge_z_dims(d.Ce, d.W2, d.Ce, d.W2, d.W2) &&
           aligned16(e, f.Pi, Hout, b_in, x);
  return f;
}

static int edge_hidden_forward_impl(Ctx& c, const cgat_plan* plan, const AttnDims& d, const float* w_in,
                                    const float* b_in, const float* x, const float* e, float* Hout, float* hmax) {
  const HiddenFwd f = hidden_fwd_carve(c, d, b_in, x, e, Hout);
  CGAT_TRY(node_projections(c, d, f.fast, true, x, w_in, b_in, NodeProj{f.Pi, f.Pj, f.Wq}));
  if (f.fast) {
    EdgeZParams z = {};
    z.e = e; z.lde = d.Ce; z.perm = plan->dst_perm; z.rows = d.E;
    z.We = w_in + d.C; z.ldw = d.D; z.Wq = f.Wq; z.W2 = d.W2;
    z.Pi = f.Pi; z.dsti = plan->dst_sorted; z.Pj = f.Pj; z.srci = plan->src_sorted; z.ld_add = d.W2;
    z.n_add_rows = 0;   // not given, as ever: this launch never runs the 256-row kernel (the table of forms)
    z.Z = Hout; z.ldz = d.W2;
    z.H = d.H; z.Hd = d.Hd;   // (hidden_dims: one "head" of W2 / 2 columns; no logits)
    z.act = CGAT_ACT_LEAKY; z.omax = hmax;
    RUN(edge_z_launch(z, c.s));
  } else {
    GemmParams g = gemm_params(d.E, d.W2, d.Ce, e, d.Ce, w_in + d.C, d.D, Hout, d.W2);
    g.a_rgather = plan->dst_perm;
    g.add1 = f.Pi; g.add1_idx = plan->dst_sorted;
    g.add2 = f.Pj; g.add2_idx = plan->src_sorted;
    g.ld_add = d.W2;
    g.act = CGAT_ACT_LEAKY;
    CGAT_TRY(c.gemm(g));
    if (hmax && !c.dry && d.E > 0) RUN(absmax_launch(Hout, (long)d.E * d.W2, hmax, c.s));   // (zeroes and fills the slot)
  }
  return check_ws(c, "edge_hidden_forward");
}

struct HiddenBwd {
  EdgeTail t;
  float* gZ;          // the pre-activation gradient the tail reads: a carve-out, or (g_is_pre) g_H itself
  float* scales;      // f16x3: [0] max |gZ|, [1] max |e|, [2..4] max |Gi|, |Gj|, |x| (set by the tail)
  // f16x3 mode: the LeakyReLU backward also yields max |gZ| and one pass over edge_attr max |e| -- with them the per-edge
  // products of the tail (K = W2 -> 128 and K = E) run on two fp16 planes (three passes) instead of the six-pass bf16
  // form they fell back to without scales: 43 + 22 ms of the harness-default network's 252-ms step
  bool have_scales;
};
// g_is_pre: g_H already is the gradient of the PRE-activation (cgat_linear_backward_dact folded LeakyReLU' into the
// product that made it) and, if has_absmax, the caller holds its maximum: no elementwise pass, no copy -- the tail reads
// g_H itself
static HiddenBwd hidden_bwd_carve(Ctx& c, const AttnDims& d, const float* w_in, const float* x, const float* e,
                                  const float* Hsaved, const float* g_H, float* g_x, float* g_e, float* g_w_in,
                                  float* g_b_in, int g_is_pre, bool has_absmax) {
  HiddenBwd b = {};
  b.gZ = g_is_pre ? const_cast<float*>(g_H) : c.take<float>((size_t)d.E * d.W2);
  EdgeTail& t = b.t;
  t.gZ = {b.gZ, d.W2, 128};
  t.Gi = c.take<float>((size_t)d.N * d.W2);
  t.Gj = c.take<float>((size_t)d.N * d.W2);
  t.Wq = c.take<float>(edge_z_wq_floats(d.W2));
  t.gw_ws = c.take<float>(edge_gw_ws_floats(d.E, d.W2));
  b.scales = c.take<float>(8);
  c.seal();
  const bool f16_ok = !c.dry && mode_f16() && d.Ce == 128 && aligned16(e) && d.E > 0;
  b.have_scales = f16_ok && (g_is_pre ? has_absmax : act_bwd_leaky_max_fast(Hsaved, g_H, b.gZ, (long)d.E * d.W2));
  t.Wcat = w_in; t.gWcat = g_w_in; t.gbcat = g_b_in;
  t.scales = b.have_scales ? b.scales : nullptr;
  t.node_scales = b.have_scales;
  t.x = x; t.e = e; t.g_x = g_x; t.g_e = g_e;
  return b;
}

static int edge_hidden_backward_impl(Ctx& c, const cgat_plan* plan, const AttnDims& d, const float* w_in, const float* x,
                                     const float* e, const float* Hsaved, const float* g_H, float* g_x, float* g_e,
                                     float* g_w_in, float* g_b_in, int g_is_pre = 0, const float* gpre_absmax = nullptr) {
  const HiddenBwd b = hidden_bwd_carve(c, d, w_in, x, e, Hsaved, g_H, g_x, g_e, g_w_in, g_b_in, g_is_pre,
                                       gpre_absmax != nullptr);
  if (b.have_scales) CGAT_TRY(fill_launch(b.scales, 0.f, 8, c.s));
  if (!g_is_pre && !b.have_scales)
    RUN(act_bwd_launch(Hsaved, g_H, b.gZ, (long)d.E * d.W2, CGAT_ACT_LEAKY, c.s));
  else if (!g_is_pre)
    RUN(act_bwd_leaky_max_launch(Hsaved, g_H, b.gZ, (long)d.E * d.W2, b.scales, c.s));
  else if (b.have_scales)   // (a kernel node, like every fill: rowops.hip)
    CGAT_TRY(copy2d_launch(gpre_absmax, 1, b.scales, 1, 1, 1, c.s));
  if (b.have_scales) RUN(absmax_rows128_launch(e, d.Ce, d.E, b.scales + 1, c.s));
  CGAT_TRY(edge_first_layer_backward_tail(c, plan, d, b.t));
  return check_ws(c, "edge_hidden_backward");
}

static int hidden_check(const cgat_plan* plan, int C, int Ce, int W2) {
  CGAT_CHECK_ARG(plan && plan->N >= 0 && plan->E >= 0, "edge_hidden: bad plan");
  CGAT_CHECK_ARG(C > 0 && Ce > 0 && W2 > 0, "edge_hidden: bad dims C=%d Ce=%d W2=%d", C, Ce, W2);
  return CGAT_OK;
}
extern "C" size_t cgat_edge_hidden_forward_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2) {
  return dry_total([&](Ctx& c) {
    return edge_hidden_forward_impl(c, plan, hidden_dims(plan, C, Ce, W2), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  });
}
extern "C" size_t cgat_edge_hidden_backward_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2) {
  return dry_total([&](Ctx& c) {
    return edge_hidden_backward_impl(c, plan, hidden_dims(plan, C, Ce, W2), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                     nullptr, nullptr, nullptr);
  });
}
extern "C" int cgat_edge_hidden_forward(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in,
                                        const float* b_in, const float* x, const float* edge_attr, float* hidden,
                                        float* hidden_absmax, void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(hidden_check(plan, C, Ce, W2));
  if (hidden_absmax) CGAT_TRY(fill_launch(hidden_absmax, 0.f, 1, (hipStream_t)stream));
  return run_sized("edge_hidden_forward", ws, ws_bytes, stream, [&](Ctx& c) {
    return edge_hidden_forward_impl(c, plan, hidden_dims(plan, C, Ce, W2), w_in, b_in, x, edge_attr, hidden, hidden_absmax);
  });
}
extern "C" int cgat_edge_hidden_backward(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in,
                                         const float* x, const float* edge_attr, const float* hidden,
                                         const float* g_hidden, int32_t g_is_pre, const float* gpre_absmax, float* g_x,
                                         float* g_edge_attr, float* g_w_in, float* g_b_in, void* ws, size_t ws_bytes,
                                         void* stream) {
  CGAT_TRY(hidden_check(plan, C, Ce, W2));
  // (sized as cgat_edge_hidden_backward_workspace_bytes sizes it, i.e. with a gZ buffer, whatever g_is_pre says)
  return run_sized("edge_hidden_backward", ws, ws_bytes, stream, [&](Ctx& c) {
    return edge_hidden_backward_impl(c, plan, hidden_dims(plan, C, Ce, W2), w_in, x, edge_attr, hidden, g_hidden, g_x,
                                     g_edge_attr, g_w_in, g_b_in, c.dry ? 0 : g_is_pre, gpre_absmax);
  });
}

// ---- edge_hidden on shell-indexed edge features: edge_attr[e] = table[index[e]], R rows (reference CGAT.py:96,105-108 on
// the message of 316-318 with the lookups of 569 / 583; include/cgat_hip.h).  `hidden` stays; what goes is everything the
// layer does per edge with edge_attr: Te = table W_e^T over R rows and a gather of three rows forward; backward the class
// sum gT of the stored gZ and two R-row products in place of grad edge_attr = gZ W_e and grad W_e = gZ^T e -- the algebra
// of attn_backward_indexed_impl.  No tensor maxima on this route: under f16x3 the node-side products run in the form that
// needs none (bf16x6), as the scalar indexed route's do.
static bool hidden_indexed_ok(const AttnDims& d, int R) {
  return edge_storage() == 0 && d.N > 0 && d.E > 0 && d.C > 0 && d.Ce > 0 && edge_idx_hidden_ok(d.W2, R);
}
struct HiddenFwdIndexed {
  float *Pi, *Pj, *Te, *Wq;
  bool fast;          // the node projections on the split per-edge kernel (else: the GEMM engine), as hidden_fwd_carve
};
static HiddenFwdIndexed hidden_fwd_indexed_carve(Ctx& c, const AttnDims& d, int R, const float* b_in, const float* x,
                                                 const float* Hout) {
  HiddenFwdIndexed f = {};
  f.Pi = c.take<float>((size_t)d.N * d.W2);
  f.Pj = c.take<float>((size_t)d.N * d.W2);
  f.Te = c.take<float>((size_t)R * d.W2);
  f.Wq = c.take<float>(edge_z_wq_floats(d.W2));
  c.seal();
  f.fast = !c.dry && d.N > 0 && d.W2 % 256 == 0 && edge_z_dims(d.C, d.W2, d.C, d.W2, d.W2) &&
           aligned16(x, f.Pi, Hout, b_in);
  return f;
}
static int edge_hidden_forward_indexed_impl(Ctx& c, const cgat_plan* plan, const AttnDims& d, const float* w_in,
                                            const float* b_in, const float* x, const float* table, int R,
                                            const int64_t* index, float* Hout, float* hmax) {
  const HiddenFwdIndexed f = hidden_fwd_indexed_carve(c, d, R, b_in, x, Hout);
  if (hmax) RUN(fill_launch(hmax, 0.f, 1, c.s));
  CGAT_TRY(node_projections(c, d, f.fast, true, x, w_in, b_in, NodeProj{f.Pi, f.Pj, f.Wq}));
  CGAT_TRY(c.gemm(gemm_params(R, d.W2, d.Ce, table, d.Ce, w_in + d.C, d.D, f.Te, d.W2)));   // (no bias: Pi carries it)
  RUN(edge_idx_hidden_launch(f.Te, R, index, plan->dst_perm, f.Pi, f.Pj, plan->src_sorted, plan->dst_sorted, d.W2, d.E, Hout,
                             hmax, c.s));
  return check_ws(c, "edge_hidden_forward_indexed");
}

struct HiddenBwdIndexed {
  EdgeTail t;         // e == nullptr, g_e == nullptr, rc == nullptr: the segment sums and the node-side products alone
  float *gZ, *gT, *cpart;
};
static HiddenBwdIndexed hidden_bwd_indexed_carve(Ctx& c, const AttnDims& d, int R, const float* w_in, const float* x,
                                                 const float* g_H, float* g_x, float* g_w_in, float* g_b_in, int g_is_pre) {
  HiddenBwdIndexed b = {};
  b.gZ = g_is_pre ? const_cast<float*>(g_H) : c.take<float>((size_t)d.E * d.W2);
  EdgeTail& t = b.t;
  t.gZ = {b.gZ, d.W2, 128};
  t.Gi = c.take<float>((size_t)d.N * d.W2);
  t.Gj = c.take<float>((size_t)d.N * d.W2);
  t.Wq = c.take<float>(edge_z_wq_floats(d.W2));
  t.gw_ws = c.take<float>(edge_gw_ws_floats(d.N, d.W2));              // (the node-side weight gradients: N rows)
  b.gT = c.take<float>((size_t)R * d.W2);
  b.cpart = c.take<float>((size_t)edge_idx_class_pieces(d.E, R) * d.W2);
  c.seal();
  t.Wcat = w_in; t.gWcat = g_w_in; t.gbcat = g_b_in;
  t.scales = nullptr;            // no maxima on this route
  t.x = x; t.g_x = g_x;
  return b;
}
static int edge_hidden_backward_indexed_impl(Ctx& c, const cgat_plan* plan, const AttnDims& d, const float* w_in,
                                             const float* x, const float* table, int R, const AttnClassPlan& cls,
                                             const float* Hsaved, const float* g_H, int g_is_pre, float* g_x,
                                             float* g_table, float* g_w_in, float* g_b_in) {
  const HiddenBwdIndexed b = hidden_bwd_indexed_carve(c, d, R, w_in, x, g_H, g_x, g_w_in, g_b_in, g_is_pre);
  if (!g_is_pre) RUN(act_bwd_launch(Hsaved, g_H, b.gZ, (long)d.E * d.W2, CGAT_ACT_LEAKY, c.s));
  const TailRoute r = tail_route(c.dry, d, b.t);
  CGAT_TRY(tail_segment_sums(c, plan, d, b.t, r));
  CGAT_TRY(tail_node_products(c, d, b.t, r));
  // gT, then grad table = gT W_e and grad W_e = gT^T table (into the W_e columns of g_w_in): attn_bwd_class_products' pair
  RUN(edge_idx_class_sum_launch(b.gZ, cls.piece_rowptr, cls.piece_start, cls.cls_pos, R, d.E, d.W2, b.cpart, b.gT, c.s));
  GemmParams g = gemm_params(R, d.Ce, d.W2, b.gT, d.W2, w_in + d.C, d.D, g_table, d.Ce);
  g.b_kmajor = 1;
  CGAT_TRY(c.gemm(g));
  g = gemm_params(d.W2, d.Ce, R, b.gT, d.W2, table, d.Ce, g_w_in + d.C, d.D);
  g.a_kmajor = 1; g.b_kmajor = 1;
  CGAT_TRY(c.gemm(g));
  return check_ws(c, "edge_hidden_backward_indexed");
}
static int hidden_indexed_refuse(const char* who, const cgat_plan* plan, int C, int Ce, int W2, int R) {
  cgat_set_error("%s: not taken for N %d, E %d, C %d, Ce %d, W2 %d, R %d under edge storage %d "
                 "(cgat_edge_hidden_indexed_ok); densify and call the dense entry", who, plan->N, plan->E, C, Ce, W2, R,
                 edge_storage());
  return CGAT_ERR_UNSUPPORTED;
}
extern "C" int32_t cgat_edge_hidden_indexed_ok(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t R) {
  if (hidden_check(plan, C, Ce, W2) != CGAT_OK) return 0;
  return hidden_indexed_ok(hidden_dims(plan, C, Ce, W2), R) ? 1 : 0;
}
extern "C" size_t cgat_edge_hidden_forward_indexed_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2,
                                                                   int32_t R) {
  if (R < 1) R = 1;
  return dry_total([&](Ctx& c) {
    return edge_hidden_forward_indexed_impl(c, plan, hidden_dims(plan, C, Ce, W2), nullptr, nullptr, nullptr, nullptr, R,
                                            nullptr, nullptr, nullptr);
  });
}
extern "C" int cgat_edge_hidden_forward_indexed(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in,
                                                const float* b_in, const float* x, const float* table, int32_t R,
                                                const int64_t* index, float* hidden, float* hidden_absmax, void* ws,
                                                size_t ws_bytes, void* stream) {
  CGAT_TRY(hidden_check(plan, C, Ce, W2));
  if (!hidden_indexed_ok(hidden_dims(plan, C, Ce, W2), R))
    return hidden_indexed_refuse("edge_hidden_forward_indexed", plan, C, Ce, W2, R);
  CGAT_CHECK_ARG(w_in && b_in && x && table && index && hidden && aligned16(hidden),
                 "edge_hidden_forward_indexed: null operand, or hidden not 16-byte aligned");
  return run_sized("edge_hidden_forward_indexed", ws, ws_bytes, stream, [&](Ctx& c) {
    return edge_hidden_forward_indexed_impl(c, plan, hidden_dims(plan, C, Ce, W2), w_in, b_in, x, table, R, index, hidden,
                                            hidden_absmax);
  });
}
extern "C" size_t cgat_edge_hidden_backward_indexed_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2,
                                                                    int32_t R) {
  if (R < 1) R = 1;
  const AttnClassPlan cls = {};
  return dry_total([&](Ctx& c) {
    return edge_hidden_backward_indexed_impl(c, plan, hidden_dims(plan, C, Ce, W2), nullptr, nullptr, nullptr, R, cls, nullptr,
                                             nullptr, 0, nullptr, nullptr, nullptr, nullptr);
  });
}
extern "C" int cgat_edge_hidden_backward_indexed(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in,
                                                 const float* x, const float* table, int32_t R, const int64_t* index,
                                                 const int32_t* cls_pos, const int32_t* piece_rowptr,
                                                 const int32_t* piece_start, const float* hidden, const float* g_hidden,
                                                 int32_t g_is_pre, const float* gpre_absmax, float* g_x, float* g_table,
                                                 float* g_w_in, float* g_b_in, void* ws, size_t ws_bytes, void* stream) {
  (void)gpre_absmax;   // (the dense entry's call shape: no product of this route takes maxima)
  CGAT_TRY(hidden_check(plan, C, Ce, W2));
  if (!hidden_indexed_ok(hidden_dims(plan, C, Ce, W2), R))
    return hidden_indexed_refuse("edge_hidden_backward_indexed", plan, C, Ce, W2, R);
  CGAT_CHECK_ARG(w_in && x && table && index && cls_pos && piece_rowptr && piece_start && g_hidden && (g_is_pre || hidden) &&
                 g_x && g_table && g_w_in && g_b_in && aligned16(g_hidden),
                 "edge_hidden_backward_indexed: null operand, or g_hidden not 16-byte aligned");
  const AttnClassPlan cls = {cls_pos, piece_rowptr, piece_start};
  // (sized as cgat_edge_hidden_backward_indexed_workspace_bytes sizes it, i.e. with a gZ buffer, whatever g_is_pre says)
  return run_sized("edge_hidden_backward_indexed", ws, ws_bytes, stream, [&](Ctx& c) {
    return edge_hidden_backward_indexed_impl(c, plan, hidden_dims(plan, C, Ce, W2), w_in, x, table, R, cls, hidden, g_hidden,
                                             c.dry ? 0 : g_is_pre, g_x, g_table, g_w_in, g_b_in);
  });
}

static int attn_check(const cgat_plan* plan, const cgat_attn_params* p) {
  CGAT_CHECK_ARG(plan && p, "nodes_attention: null plan/params");
  CGAT_CHECK_ARG(plan->N >= 0 && plan->E >= 0, "nodes_attention: negative N/E");
  CGAT_CHECK_ARG(p->C > 0 && p->Ce > 0 && p->H > 0 && p->Hd > 0, "nodes_attention: bad dims C=%d Ce=%d H=%d Hd=%d",
                 p->C, p->Ce, p->H, p->Hd);
  return CGAT_OK;
}

extern "C" size_t cgat_nodes_attention_forward_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p) {
  return dry_total([&](Ctx& c) { return attn_forward_impl(c, plan, p, nullptr, nullptr, nullptr, nullptr); });
}
extern "C" size_t cgat_nodes_attention_backward_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p) {
  cgat_attn_grads g = {};
  return dry_total([&](Ctx& c) { return attn_backward_impl(c, plan, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &g); });
}
extern "C" int cgat_nodes_attention_forward(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                            const float* edge_attr, float* aggr, float* saved, void* ws,
                                            size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  return run_sized("nodes_attention_forward", ws, ws_bytes, stream,
                   [&](Ctx& c) { return attn_forward_impl(c, plan, p, x, edge_attr, aggr, saved); });
}
extern "C" int32_t cgat_nodes_attention_infer_fused(const cgat_plan* plan, const cgat_attn_params* p) {
  if (attn_check(plan, p) != CGAT_OK) return 0;
  return attn_infer_fused(attn_dims(plan, p)) ? 1 : 0;
}
extern "C" size_t cgat_nodes_attention_infer_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p) {
  return dry_total([&](Ctx& c) { return attn_forward_impl(c, plan, p, nullptr, nullptr, nullptr, nullptr, true); });
}
extern "C" int cgat_nodes_attention_infer(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                          const float* edge_attr, float* aggr, void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  return run_sized("nodes_attention_infer", ws, ws_bytes, stream,
                   [&](Ctx& c) { return attn_forward_impl(c, plan, p, x, edge_attr, aggr, nullptr, true); });
}
extern "C" int32_t cgat_nodes_attention_infer_indexed_ok(const cgat_plan* plan, const cgat_attn_params* p, int32_t R) {
  if (attn_check(plan, p) != CGAT_OK) return 0;
  return attn_infer_indexed_ok(attn_dims(plan, p), R) ? 1 : 0;
}
extern "C" size_t cgat_nodes_attention_infer_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p,
                                                                     int32_t R) {
  if (R < 1) R = 1;
  return dry_total([&](Ctx& c) { return attn_infer_indexed_impl(c, plan, p, nullptr, nullptr, R, nullptr, nullptr); });
}
extern "C" int cgat_nodes_attention_infer_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                                  const float* table, int32_t R, const int64_t* index, float* aggr,
                                                  void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  if (!attn_infer_indexed_ok(attn_dims(plan, p), R)) {
    cgat_set_error("nodes_attention_infer_indexed: not taken for N %d, E %d, H %d, Hd %d, R %d under edge storage %d "
                   "(cgat_nodes_attention_infer_indexed_ok); densify and call cgat_nodes_attention_infer", plan->N, plan->E,
                   p->H, p->Hd, R, edge_storage());
    return CGAT_ERR_UNSUPPORTED;
  }
  CGAT_CHECK_ARG(x && table && index && aggr, "nodes_attention_infer_indexed: null operand");
  return run_sized("nodes_attention_infer_indexed", ws, ws_bytes, stream,
                   [&](Ctx& c) { return attn_infer_indexed_impl(c, plan, p, x, table, R, index, aggr); });
}
// ---- the indexed training route (include/cgat_hip.h) ----
extern "C" int32_t cgat_nodes_attention_train_indexed_ok(const cgat_plan* plan, const cgat_attn_params* p, int32_t R) {
  if (attn_check(plan, p) != CGAT_OK) return 0;
  return attn_train_indexed_ok(attn_dims(plan, p), R) ? 1 : 0;
}
static int train_indexed_refuse(const char* who, const cgat_plan* plan, const cgat_attn_params* p, int R) {
  cgat_set_error("%s: not taken for N %d, E %d, H %d, Hd %d, R %d under edge storage %d "
                 "(cgat_nodes_attention_train_indexed_ok); densify and call the dense entry", who, plan->N, plan->E, p->H, p->Hd,
                 R, edge_storage());
  return CGAT_ERR_UNSUPPORTED;
}
extern "C" size_t cgat_nodes_attention_forward_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p,
                                                                       int32_t R) {
  if (R < 1) R = 1;
  return dry_total([&](Ctx& c) { return attn_infer_indexed_impl(c, plan, p, nullptr, nullptr, R, nullptr, nullptr, true); });
}
extern "C" int cgat_nodes_attention_forward_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                                    const float* table, int32_t R, const int64_t* index, float* aggr,
                                                    float* saved, void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  if (!attn_train_indexed_ok(attn_dims(plan, p), R)) return train_indexed_refuse("nodes_attention_forward_indexed", plan, p, R);
  CGAT_CHECK_ARG(x && table && index && aggr && saved && (((uintptr_t)saved) & 255) == 0,
                 "nodes_attention_forward_indexed: null operand, or saved not on a 256-byte boundary");
  return run_sized("nodes_attention_forward_indexed", ws, ws_bytes, stream,
                   [&](Ctx& c) { return attn_infer_indexed_impl(c, plan, p, x, table, R, index, aggr, true, saved); });
}
extern "C" size_t cgat_nodes_attention_backward_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p,
                                                                        int32_t R) {
  if (R < 1) R = 1;
  cgat_attn_grads g = {};
  const AttnClassPlan cls = {};
  return dry_total([&](Ctx& c) {
    return attn_backward_indexed_impl(c, plan, p, nullptr, nullptr, R, nullptr, cls, nullptr, nullptr, nullptr, nullptr, &g);
  });
}
extern "C" int cgat_nodes_attention_backward_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                                     const float* table, int32_t R, const int64_t* index,
                                                     const int32_t* cls_pos, const int32_t* piece_rowptr,
                                                     const int32_t* piece_start, const float* saved, const float* g_aggr,
                                                     float* g_x, float* g_table, const cgat_attn_grads* g, void* ws,
                                                     size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  if (!attn_train_indexed_ok(attn_dims(plan, p), R)) return train_indexed_refuse("nodes_attention_backward_indexed", plan, p, R);
  CGAT_CHECK_ARG(x && table && index && cls_pos && piece_rowptr && piece_start && saved && g_aggr && g_x && g_table && g &&
                 (((uintptr_t)saved) & 255) == 0,
                 "nodes_attention_backward_indexed: null operand, or saved not on a 256-byte boundary");
  const AttnClassPlan cls = {cls_pos, piece_rowptr, piece_start};
  return run_sized("nodes_attention_backward_indexed", ws, ws_bytes, stream, [&](Ctx& c) {
    return attn_backward_indexed_impl(c, plan, p, x, table, R, index, cls, saved, g_aggr, g_x, g_table, g);
  });
}
// the class grouping of the slots (edgeidx.hip): cls_pos [E] = the slots of class 0, 1, ... in ascending slot order,
// piece_start [R + 1], piece_rowptr [cgat_indexed_class_pieces(E, R) + 1]; once per (index, plan), outside the hot path
extern "C" int32_t cgat_indexed_class_pieces(int32_t E, int32_t R) { return edge_idx_class_pieces(E, R); }
extern "C" size_t cgat_indexed_class_plan_workspace_bytes(int32_t E, int32_t R) { return edge_idx_class_plan_ws_bytes(E, R) + 256; }
extern "C" int cgat_indexed_class_plan(const cgat_plan* plan, const int64_t* index, int32_t R, int32_t* cls_pos,
                                       int32_t* piece_start, int32_t* piece_rowptr, void* ws, size_t ws_bytes, void* stream) {
  CGAT_CHECK_ARG(plan && plan->E > 0, "indexed_class_plan: null plan or no edges");
  return edge_idx_class_plan_launch(index, plan->dst_perm, plan->E, R, cls_pos, piece_start, piece_rowptr, ws, ws_bytes,
                                    (hipStream_t)stream);
}
// debug: the signs of z as this route forms it, uint8 [E, W2] in original edge order: the projections and Te by the
// forward's launches, z by idx_z
static int debug_signs_indexed_impl(Ctx& c, const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                    const float* table, int R, const int64_t* index, uint8_t* mask) {
  const AttnFwdIndexed g = attn_fwd_indexed_carve(c, plan, p, x, table, R, index, nullptr);
  const AttnFwd& f = g.f;
  CGAT_TRY(stack_in_weights(c, p, f.d, f.Wcat, f.bcat));
  CGAT_TRY(node_projections_indexed(c, g));
  CGAT_TRY(indexed_edge_table(c, g));
  RUN(edge_idx_signs_launch(g.Te, R, index, plan->dst_perm, f.Pi, f.Pj, plan->src_sorted, plan->dst_sorted, f.d.W2, (long)f.d.E,
                            mask, c.s));
  return check_ws(c, "debug_nodes_attention_signs_indexed");
}
extern "C" size_t cgat_debug_nodes_attention_signs_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p,
                                                                           int32_t R) {
  if (R < 1) R = 1;
  return dry_total([&](Ctx& c) { return debug_signs_indexed_impl(c, plan, p, nullptr, nullptr, R, nullptr, nullptr); });
}
extern "C" int cgat_debug_nodes_attention_signs_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                                        const float* table, int32_t R, const int64_t* index, uint8_t* mask,
                                                        void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  if (!attn_train_indexed_ok(attn_dims(plan, p), R))
    return train_indexed_refuse("debug_nodes_attention_signs_indexed", plan, p, R);
  CGAT_CHECK_ARG(x && table && index && mask, "debug_nodes_attention_signs_indexed: null operand");
  return run_sized("debug_nodes_attention_signs_indexed", ws, ws_bytes, stream,
                   [&](Ctx& c) { return debug_signs_indexed_impl(c, plan, p, x, table, R, index, mask); });
}
extern "C" int cgat_nodes_attention_backward(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                             const float* edge_attr, const float* saved, const float* g_aggr,
                                             float* g_x, float* g_edge_attr, const cgat_attn_grads* g, void* ws,
                                             size_t ws_bytes, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  CGAT_CHECK_ARG(g, "nodes_attention_backward: null grads");
  return run_sized("nodes_attention_backward", ws, ws_bytes, stream, [&](Ctx& c) {
    return attn_backward_impl(c, plan, p, x, edge_attr, saved, g_aggr, g_x, g_edge_attr, g);
  });
}

// ---- debug: the routes of a layer as bit masks (include/cgat_hip.h), for 16-byte aligned operands: the carve and route
// functions of the real pass over a null, unbounded workspace ----
extern "C" uint32_t cgat_debug_nodes_attention_route(const cgat_plan* plan, const cgat_attn_params* p, int32_t backward) {
  if (attn_check(plan, p) != CGAT_OK) return 0;
  Ctx c(nullptr, (size_t)-1 / 2, false, nullptr);
  if (!backward) {
    const AttnFwdRoute r = attn_fwd_carve(c, plan, p, nullptr, nullptr, nullptr, nullptr, false).r;
    return route_bits({attn_infer_fused(attn_dims(plan, p)), r.zx, r.fused_z, r.z_bf16, r.proj_fast, r.out_fast, r.out_one});
  }
  const AttnBwd b = attn_bwd_carve(c, plan, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  const TailRoute t = tail_route(false, b.d, attn_bwd_tail(b));
  return route_bits({b.r.rc, b.r.vec, b.r.have_scales, b.r.z_bf16, b.r.z_bf16_six, b.r.out_fast, b.r.out_heads_one,
                     t.node == NODE_KSPLIT, t.node == NODE_SMALL_ROWS, t.node == NODE_LAUNCHES, t.node == NODE_GEMM,
                     t.node_scales, t.ge == PRODUCT_KSPLIT, t.ge == PRODUCT_LAUNCH, t.ge == PRODUCT_GEMM,
                     t.gw == PRODUCT_LAUNCH, t.gw == PRODUCT_GEMM});
}

extern "C" uint32_t cgat_debug_edge_hidden_route(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t backward,
                                                 int32_t g_is_pre, int32_t has_absmax) {
  if (hidden_check(plan, C, Ce, W2) != CGAT_OK) return 0;
  const AttnDims d = hidden_dims(plan, C, Ce, W2);
  // (a non-null aligned base: no carve-out is a null pointer, as none is in a real pass; nothing is dereferenced)
  Ctx c((void*)256, (size_t)-1 / 2, false, nullptr);
  if (!backward) return route_bits({hidden_fwd_carve(c, d, nullptr, nullptr, nullptr, nullptr).fast});
  const HiddenBwd b = hidden_bwd_carve(c, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                       g_is_pre, has_absmax != 0);
  const TailRoute t = tail_route(false, d, b.t);
  return route_bits({b.have_scales, t.node == NODE_KSPLIT, t.node == NODE_SMALL_ROWS, t.node == NODE_LAUNCHES,
                     t.node == NODE_GEMM, t.node_scales, t.ge == PRODUCT_KSPLIT, t.ge == PRODUCT_LAUNCH,
                     t.ge == PRODUCT_GEMM, t.gw == PRODUCT_LAUNCH, t.gw == PRODUCT_GEMM});
}

// ---- debug: the sign pattern of the saved pre-activations in original edge order (include/cgat_hip.h) ----
extern "C" int cgat_debug_nodes_attention_signs(const cgat_plan* plan, const cgat_attn_params* p, const float* saved,
                                                uint8_t* mask, void* stream) {
  CGAT_TRY(attn_check(plan, p));
  CGAT_CHECK_ARG(saved && mask, "debug_nodes_attention_signs: null pointer");
  const AttnDims d = attn_dims(plan, p);
  if (attn_bf16(d)) {
    cgat_set_error("debug_nodes_attention_signs: fp32 edge storage only");
    return CGAT_ERR_UNSUPPORTED;
  }
  // The bit form: as the forward that filled THIS buffer decided it on its real operands (recorded there); for any other
  // buffer, as a forward on 16-byte aligned x and edge_attr with this buffer and this fc_out_A weight decides it.
  const bool bits = saved == g_fwd_saved ? g_fwd_saved_bits : attn_z_form(d, saved, saved, saved, p->A_out_w, saved).bits;
  return attn_signs_launch(saved, plan->dst_perm, (long)d.E, d.W2, mask, (hipStream_t)stream,
                           bits ? reinterpret_cast<const unsigned*>(saved + 2 * (size_t)d.N * d.W2) : nullptr);
}

// Does the training forward of this layer keep its saved buffer in the bit form (16-byte aligned operands assumed)
extern "C" int32_t cgat_nodes_attention_bit_form(const cgat_plan* plan, const cgat_attn_params* p) {
  if (attn_check(plan, p) != CGAT_OK) return 0;
  const void* al = (const void*)256;
  return attn_z_form(attn_dims(plan, p), (const float*)al, (const float*)al, (const float*)al, (const float*)al, al).bits ? 1 : 0;
}

// ---- debug: one per-edge product of the tail alone, on caller-supplied ingredients of the rebuilt gZ rows (struct EdgeRC,
// kernels.h), through the step attn_backward_impl takes for it.  The "layer" is the W_e slice alone: no node columns
// (C = 0, D = 128), the weight / its gradient [W2, 128], gZ column-blocked as the backward's.
struct EdgeProductDebug {
  AttnDims d;
  cgat_plan plan;    // dst_perm alone is read
  EdgeRC rc;
  EdgeTail t;
};
static void edge_product_debug(EdgeProductDebug& q, const EdgeRC& rc, const int32_t* perm, int32_t E) {
  memset(&q, 0, sizeof(q));
  q.d.E = E; q.d.Ce = 128; q.d.H = rc.H; q.d.Hd = rc.Hd; q.d.D = 128; q.d.HHd = rc.HHd; q.d.W2 = 2 * rc.HHd;
  q.plan.E = E; q.plan.dst_perm = perm;
  q.rc = rc;
  q.t.gZ = {nullptr, 128, (long)E * 128};
  q.t.rc = &q.rc;
  q.t.have_Gi = true;
}
// grad edge_attr's product: the K-group form at few row tiles, the plain launch otherwise
static int debug_edge_ge_impl(Ctx& c, const EdgeRC& rc, const float* We, int32_t E, float* out) {
  EdgeProductDebug q;
  edge_product_debug(q, rc, nullptr, E);
  q.t.Wq = c.take<float>(edge_z_wq_floats(q.d.W2));
  c.seal();
  q.t.Wcat = We; q.t.g_e = out;
  CGAT_TRY(tail_edge_ge(c, &q.plan, q.d, q.t, tail_route(c.dry, q.d, q.t)));
  return check_ws(c, "debug_edge_ge_rebuilt");
}
extern "C" size_t cgat_debug_edge_ge_rebuilt_workspace_bytes(int32_t E, int32_t H, int32_t Hd) {
  return dry_total([&](Ctx& c) { return debug_edge_ge_impl(c, edge_rc_make(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, H, Hd), nullptr, E, nullptr); });
}
extern "C" int cgat_debug_edge_ge_rebuilt(const uint32_t* mask, const float* ga, const float* alpha, const float* gS,
                                          const float* wA, const int32_t* dst, const float* We, int32_t H, int32_t Hd,
                                          int32_t E, float* out, void* ws, size_t ws_bytes, void* stream) {
  const int W2 = 2 * H * Hd;
  CGAT_CHECK_ARG(mask && ga && alpha && gS && wA && dst && We && out && ws, "debug_edge_ge_rebuilt: null pointer");
  CGAT_CHECK_ARG(E > 0 && edge_rc_shape(128, H, Hd) && W2 % 256 == 0 && mode_24bit() && !edge_mma_bf16(),
                 "debug_edge_ge_rebuilt: H = %d, Hd = %d in a 24-bit mode with fp32 edge storage", H, Hd);
  CGAT_CHECK_ARG(ws_bytes >= cgat_debug_edge_ge_rebuilt_workspace_bytes(E, H, Hd) && aligned16(gS, wA, We) && aligned16(out, ws),
                 "debug_edge_ge_rebuilt: workspace too small or operands not 16-byte aligned");
  const EdgeRC rc = edge_rc_make(mask, ga, alpha, gS, wA, dst, H, Hd);
  return run_sized("debug_edge_ge_rebuilt", ws, ws_bytes, stream,
                   [&](Ctx& c) { return debug_edge_ge_impl(c, rc, We, E, out); });
}

// grad W_e's product; force_six: THIS launch keeps the six-pass form whatever the route would be (an argument of
// the launch, no shared state); cgat_debug_edge_gw_force_six: the one process-wide switch (edgebwd.hip)
extern "C" int32_t cgat_debug_edge_gw_force_six(int32_t on) { return edge_gw_force_six(on != 0) ? 1 : 0; }
static int debug_edge_gw_impl(Ctx& c, const EdgeRC& rc, const float* e, const int32_t* perm, int32_t E, bool force_six,
                              float* out) {
  EdgeProductDebug q;
  edge_product_debug(q, rc, perm, E);
  q.t.gw_ws = c.take<float>(edge_gw_ws_floats(E, q.d.W2));
  c.seal();
  q.t.e = e; q.t.gWcat = out; q.t.gw_force_six = force_six;
  CGAT_TRY(tail_edge_gw(c, &q.plan, q.d, q.t, tail_route(c.dry, q.d, q.t)));
  return check_ws(c, "debug_edge_gw_rebuilt");
}
extern "C" size_t cgat_debug_edge_gw_rebuilt_workspace_bytes(int32_t E, int32_t H, int32_t Hd) {
  return dry_total([&](Ctx& c) { return debug_edge_gw_impl(c, edge_rc_make(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, H, Hd), nullptr, nullptr, E, false, nullptr); });
}
extern "C" int cgat_debug_edge_gw_rebuilt(const uint32_t* mask, const float* ga, const float* alpha, const float* gS,
                                          const float* wA, const float* e, const int32_t* perm, const int32_t* dst,
                                          int32_t H, int32_t Hd, int32_t E, int32_t force_six, float* out,
                                          int32_t* took_bitplane, void* ws, size_t ws_bytes, void* stream) {
  const int W2 = 2 * H * Hd;
  CGAT_CHECK_ARG(mask && ga && alpha && gS && wA && e && perm && dst && out && ws, "debug_edge_gw_rebuilt: null pointer");
  if (!mode_split()) {   // the f32 mode has no such launch: its layers run the generic GEMM on a stored gZ
    cgat_set_error("debug_edge_gw_rebuilt: split arithmetic modes only");
    return CGAT_ERR_UNSUPPORTED;
  }
  CGAT_CHECK_ARG(E > 0 && edge_rc_shape(128, H, Hd) && W2 % 256 == 0, "debug_edge_gw_rebuilt: H = %d, Hd = %d", H, Hd);
  CGAT_CHECK_ARG(ws_bytes >= cgat_debug_edge_gw_rebuilt_workspace_bytes(E, H, Hd) && aligned16(gS, wA, e) && aligned16(out, ws),
                 "debug_edge_gw_rebuilt: workspace too small or operands not 16-byte aligned");
  const EdgeRC rc = edge_rc_make(mask, ga, alpha, gS, wA, dst, H, Hd);
  if (took_bitplane) {   // the form of a record like the launch's own (tail_edge_gw); not launched
    EdgeGwParams w = edge_gw_params(nullptr, 128, (long)E * 128, e, 128, perm, E, W2, nullptr, out, 128);
    w.rc = &rc; w.force_six = force_six != 0;
    *took_bitplane = edge_gw_form(w).bitplane ? 1 : 0;
  }
  return run_sized("debug_edge_gw_rebuilt", ws, ws_bytes, stream,
                   [&](Ctx& c) { return debug_edge_gw_impl(c, rc, e, perm, E, force_six != 0, out); });
}
