// Hypernetwork orchestrators (Pooling_NN: H_Net_0 / H_Net): the sequence of kernel launches behind cgat_hnet_forward,
// cgat_hnet_backward and cgat_hnet_backward_overlapped.  Host code only, like layers.hip: it carves the caller's
// workspace, decides the route of the pass once (HnetFwdRoute / HnetBwdRoute) and enqueues the steps on the caller's
// stream(s) -- no allocation, no synchronisation.
#include "layers.h"

struct HnetSaved {  // acts[l][s] (s < n_fc), u[l], vin[l] (l >= 1), hin
  float* base;
  size_t rw;  // rows * W
  int n_fc, n_hyper;
  float* act(int l, int s) const { return base + ((size_t)l * n_fc + s) * rw; }
  float* u(int l) const { return base + ((size_t)n_hyper * n_fc + l) * rw; }
  float* vin(int l) const { return base + ((size_t)n_hyper * n_fc + n_hyper + l) * rw; }  // l >= 1 used
  float* hin() const { return base + ((size_t)n_hyper * n_fc + 2 * (size_t)n_hyper) * rw; }
};
extern "C" size_t cgat_hnet_saved_floats(int32_t rows, const cgat_hnet_params* p) {
  return ((size_t)p->n_hyper * p->n_fc + 2 * (size_t)p->n_hyper + 1) * (size_t)rows * p->W;
}
static HnetSaved hnet_saved(float* base, int rows, const cgat_hnet_params* p) {
  return HnetSaved{base, (size_t)rows * p->W, p->n_fc, p->n_hyper};
}

static int hnet_check(int rows, const cgat_hnet_params* p) {
  CGAT_CHECK_ARG(p, "hnet: null params");
  CGAT_CHECK_ARG(rows >= 0 && p->W > 0, "hnet: bad rows/W");
  CGAT_CHECK_ARG(p->n_fc >= 1 && p->n_fc <= CGAT_MAX_FC && p->n_hyper >= 1 && p->n_hyper <= CGAT_MAX_HYPER,
                 "hnet: n_fc=%d n_hyper=%d out of range", p->n_fc, p->n_hyper);
  return CGAT_OK;
}

// `side`: optional second stream + workspace.  The four dT contractions (the weight-gradient kernel and its operand
// preparation) feed nothing else in the backward pass, and they are matrix-core bound while what follows them (the
// attention backward of the layer) is HBM bound: issued on the side stream they run beside it (measured in isolation:
// 7.3 ms of contractions + 7.7 ms of streaming take 10.8 ms on two streams instead of 15.0).  Their inputs must then
// outlive this call's main-stream buffers: every layer's g_u gets its own buffer in the side workspace.
struct HnetSide {
  hipStream_t s;
  void* ws;
  size_t bytes;
  int wgrad_wgs;      // workgroups of the dT launch: 0 = one per CU, 128 = half of the chip
};
// side workspace: [g_u of every predicted layer][g_pre of every trunk layer][slabs of the batched dense-layer weight
// gradients][workspace of the dT launch]
struct HnetSideLayout { size_t gu, gpre, dw, wgrad, total; };
static HnetSideLayout hnet_side_layout(int rows, const cgat_hnet_params* p) {
  const size_t rw = (size_t)rows * p->W;
  HnetSideLayout L;
  L.gu = 0;
  L.gpre = L.gu + ws_round((size_t)p->n_hyper * rw, 4);
  L.dw = L.gpre + ws_round((size_t)p->n_hyper * (p->n_fc > 0 ? p->n_fc : 1) * rw, 4);
  L.wgrad = L.dw + rows_dw128_batch_ws_bytes(p->n_hyper * (p->n_fc + 2), rows);
  L.total = L.wgrad + bilinear_wgrad_batch_ws_bytes(p->n_hyper, rows, p->W, p->W, p->W) + 256;
  return L;
}

// Makes `waiter` wait for everything issued on `signaller` so far.  Events come from a small ring created lazily and
// never destroyed: under a hipGraph capture (cgat_amd.GraphedStep) the captured dependency keeps referring to the event
// object, and destroying it right after the wait -- legal in eager mode -- crashed hipStreamEndCapture on the second
// capture of a process.
static hipEvent_t g_wait_ring[64];
static unsigned g_wait_next = 0, g_wait_made = 0;
static int stream_wait_stream(hipStream_t waiter, hipStream_t signaller) {
  const unsigned slot = g_wait_next++ % 64;
  if (slot >= g_wait_made) {
    CGAT_HIP(hipEventCreateWithFlags(&g_wait_ring[slot], hipEventDisableTiming));
    g_wait_made = slot + 1;
  }
  CGAT_HIP(hipEventRecord(g_wait_ring[slot], signaller));
  CGAT_HIP(hipStreamWaitEvent(waiter, g_wait_ring[slot], 0));
  return CGAT_OK;
}

// ---- what a pass batches, by dims and arithmetic mode alone: hnet_carve sizes its buffers by these (the dry pass as the
// real one), and the routes start from them ----
// the re-laid T of every predicted layer prepared up front in two launches (f16x3, f16x3c)
static bool hnet_batch_T(const cgat_hnet_params* p, bool backward) {
  return p->W == 128 && mode_f16_T() && p->n_hyper <= TPREP_MAX && (!backward || bilinear_dual_fast(p->W, p->W, p->W));
}
// every dense-layer weight image of the pass prepared in one launch
static bool hnet_batch_w(const cgat_hnet_params* p) { return p->W == 128 && p->n_hyper * (p->n_fc + 2) <= WPREP_MAX; }
// backward: a trunk's backward as one chain launch (chain.hip), which leaves every trunk layer's pre-activation gradient
// behind, ...
static bool hnet_chain_ok(const cgat_hnet_params* p) {
  return hnet_batch_w(p) && wprep_image_floats() != 0 && p->n_fc >= 1 && p->n_fc <= CHAIN_MAX;
}
// ... so the weight gradients of all dense layers of all predicted layers can wait for ONE batched launch at the end
// (rowsdw.hip): they feed nothing else in the backward pass.  g_pre then needs a buffer per predicted layer.
static bool hnet_defer_dw(const cgat_hnet_params* p) {
  return hnet_chain_ok(p) && p->n_hyper * (p->n_fc + 2) <= DW_BATCH_MAX;
}
// At a few thousand rows (the harness' shipped batch: 1 280 atoms) a trunk chain is 10 workgroups, and the four chains of
// a backward pass -- one per predicted layer, each 57 us, none feeding another: they feed the weight gradients and the
// SUM g_hin -- were 1.1 ms of an 18-ms step.  There they wait for ONE batched launch behind the loop (round 6): every
// predicted layer keeps its own g_t and writes its g_hin term to a slab; the slabs are added in the order the
// accumulating chains ran in (bit-identical).
static bool hnet_chain_batch(int rows, const cgat_hnet_params* p) {
  return hnet_defer_dw(p) && rows <= 8192 && p->n_hyper > 1 && p->n_hyper <= CHAIN_BATCH_MAX && !mode_f16();
}

// The carved buffers of one hypernetwork pass: made once by hnet_carve, read by every step.
struct HnetPlan {
  int rows, W;
  size_t WW, rw, Tfl;    // W * W, rows * W, floats of one re-laid T
  float *Tp, *Tpart;     // Tp: one re-laid T per predicted layer under hnet_batch_T, else one for all
  // backward only
  int nfc1;              // trunk layers with a g_pre buffer (at least one)
  float *g_hin, *g_u, *gvin_buf[2], *g_t_all, *ghin_slabs, *g_pre_all;
  size_t g_t_stride, g_pre_stride;   // floats between two predicted layers' buffers: 0 = all share one
  HnetSideLayout SL;
  float* T(int l, bool batched) const { return Tp + (batched ? (size_t)l * Tfl : 0); }
  float* g_t(int l) const { return g_t_all + (size_t)l * g_t_stride; }
  float* g_pre(int l) const { return g_pre_all + (size_t)l * g_pre_stride; }
};

// Every dense-layer weight of the pass, listed for one image launch per kind (hnet_prepare_weights): forward orientation
// [out][in], or `transposed` for the backward's g_in = g_out W.  Bm = head_b[:W*W] as [o,i], U = head_w[W*W:].  Host only:
// an image's address is its place in the list times the image size, so the routes can ask for it before the launch.
static void hnet_list_weights(Ctx& c, const HnetPlan& h, const cgat_hnet_params* p, bool transposed) {
  const long so = transposed ? 1 : h.W, sk = transposed ? h.W : 1;
  for (int l = 0; l < p->n_hyper; ++l) {
    const float* U = p->layer[l].head_w + h.WW * h.W;
    for (int s = 0; s < p->n_fc; ++s) c.wprep_add(p->layer[l].fc_w[s], so, sk);
    if (mode_f16()) {
      c.wprep_add(p->layer[l].head_b, so, sk);   // read by linear128_launch in that mode only
    } else {                                     // (the 24-bit modes: the dense-layer kernel's image)
      c.tprep_add(p->layer[l].head_b, so, sk);
      if (transposed) c.tprep_add(U, so, sk);
    }
    c.wprep_add(U, so, sk);
  }
}

// Carves the persistent buffers, lists the weights whose images the pass prepares and seals the workspace.  The ORDER and
// sizes of the take / reserve calls are the workspace layout, the same in the dry and the real pass.
static HnetPlan hnet_carve(Ctx& c, int rows, const cgat_hnet_params* p, bool backward, const HnetSide* side) {
  HnetPlan h = {};
  const int W = p->W;
  h.rows = rows; h.W = W; h.WW = (size_t)W * W; h.rw = (size_t)rows * W; h.Tfl = bilinear_T_floats(W, W, W);
  const size_t rw = h.rw;
  const bool defer_dw = hnet_defer_dw(p), chain_batch = hnet_chain_batch(rows, p);
  h.Tp = c.take<float>((hnet_batch_T(p, backward) ? (size_t)p->n_hyper : 1) * h.Tfl);
  h.Tpart = c.take<float>(bilinear_prepare_T_batch_ws_floats(p->n_hyper));
  if (backward) {
    h.g_hin = c.take<float>(rw);
    h.g_u = c.take<float>((size_t)p->n_hyper * rw);   // one per predicted layer: all dT run in ONE launch at the end
    h.gvin_buf[0] = c.take<float>(rw);
    h.gvin_buf[1] = c.take<float>(rw);
    h.nfc1 = p->n_fc > 0 ? p->n_fc : 1;
    h.g_t_stride = chain_batch ? rw : 0;
    h.g_pre_stride = defer_dw ? (size_t)h.nfc1 * rw : 0;
    h.g_t_all = c.take<float>((chain_batch ? (size_t)p->n_hyper : 1) * rw);
    h.ghin_slabs = chain_batch ? c.take<float>((size_t)p->n_hyper * rw) : nullptr;
    h.SL = hnet_side_layout(rows, p);
    h.g_pre_all = (side && defer_dw) ? (c.dry ? nullptr : (float*)((char*)side->ws + h.SL.gpre))
                                     : c.take<float>((size_t)(defer_dw ? p->n_hyper : 1) * h.nfc1 * rw);
  }
  if (hnet_batch_w(p)) {
    c.wprep_reserve(p->n_hyper * (p->n_fc + 2));
    c.tprep_reserve(2 * p->n_hyper);
    hnet_list_weights(c, h, p, /*transposed=*/backward);
  }
  c.seal();
  if (backward) {
    if (defer_dw && !side) c.need(rows_dw128_batch_ws_bytes(p->n_hyper * (p->n_fc + 2), rows));
    if (defer_dw) c.need(rows_dw128_ws_bytes(rows, 2));   // an operand off the 16-byte grid takes the per-layer launch
  }
  return h;
}

// the listed weight images, one launch per image kind
static int hnet_prepare_weights(Ctx& c) {
  CGAT_TRY(c.wprep_run());
  CGAT_TRY(c.tprep_run());
  return CGAT_OK;
}

// Can the re-laid T operands of ALL predicted layers be prepared in two launches (hnet_prepare_T_all)?  perm1 / perm2: the
// last two indices of the caller's view of T[o,i,k] = head_w[(o*W+i)*W + k].  Where not, the caller prepares each layer's
// operand when it gets there.
static bool hnet_T_batched(const HnetPlan& h, const cgat_hnet_params* p, bool backward, int perm1, int perm2) {
  if (!hnet_batch_T(p, backward)) return false;
  const float* tsrc[TPREP_MAX];
  for (int l = 0; l < p->n_hyper; ++l) tsrc[l] = p->layer[l].head_w;
  return bilinear_prepare_T_batch_takes(p->n_hyper, tsrc, h.W, h.W, h.W, perm1, perm2);
}
static int hnet_prepare_T_all(Ctx& c, const HnetPlan& h, const cgat_hnet_params* p, int perm0, int perm1, int perm2) {
  const float* tsrc[TPREP_MAX];
  float* tdst[TPREP_MAX];
  for (int l = 0; l < p->n_hyper; ++l) { tsrc[l] = p->layer[l].head_w; tdst[l] = h.T(l, true); }
  return bilinear_prepare_T_batch(p->n_hyper, tsrc, tdst, h.W, h.W, h.W, perm0, perm1, perm2, h.Tpart, c.s);
}

// =======================================================================================
// forward
// =======================================================================================
struct HnetFwdRoute {
  bool T_batched;   // every predicted layer's re-laid T up front in two launches (else: one by one in the loop)
  bool w_batched;   // every dense-layer weight image of the pass in one launch per image kind
  bool chained;     // trunk + trunk-side linear term of the head as ONE chain per predicted layer, CHAIN_BATCH_MAX chains per
                    // launch (else: one product per dense layer)
  bool ln_fused;    // LayerNorm + tanh of every layer but the last in the contraction's slab sum (width 128)
};

// The trunk (n_fc x [Linear + Tanh]) and the trunk-side linear term of the head, u = z @ U^T + b0, as ONE chain per
// predicted layer (chain.hip) on the listed weight images (width 128, <= 4 trunk layers); the remaining linear term
// u += vin @ Bm^T follows per layer.  Fills cds[l] and says whether the chain kernel takes every one of them.
static bool hnet_forward_chain_descs(const Ctx& c, const HnetPlan& h, const cgat_hnet_params* p, const float* hin,
                                     const HnetSaved& sv, float* y, ChainDesc* cds) {
  const int W = h.W;
  for (int l = 0; l < p->n_hyper; ++l) {
    const cgat_hyperlinear_params& L = p->layer[l];
    ChainDesc& cd = cds[l];
    memset(&cd, 0, sizeof(cd));
    cd.n_layers = p->n_fc + 1; cd.rows = h.rows; cd.x = hin; cd.ldx = W;
    for (int s = 0; s < p->n_fc; ++s) {
      ChainLayer& cl = cd.layer[s];
      cl.W = (const uint4*)c.wprep_find(L.fc_w[s], W, 1);
      cl.bias = L.fc_b[s]; cl.act = CGAT_ACT_TANH; cl.out = sv.act(l, s); cl.ld_out = W;
      if (!cl.W) return false;
    }
    ChainLayer& cu = cd.layer[p->n_fc];
    cu.W = (const uint4*)c.wprep_find(L.head_w + h.WW * W, W, 1);
    cu.bias = L.head_b + h.WW; cu.act = CGAT_ACT_NONE; cu.out = (l == p->n_hyper - 1) ? y : sv.u(l); cu.ld_out = W;
    if (!cu.W || !mlp_chain128_fast(cd)) return false;
  }
  return true;
}

// cds: the chains of a `chained` route (CGAT_MAX_HYPER descriptors of the caller's)
static HnetFwdRoute hnet_fwd_route(const Ctx& c, const HnetPlan& h, const cgat_hnet_params* p, const float* hin,
                                   const HnetSaved& sv, float* y, ChainDesc* cds) {
  HnetFwdRoute r = {};
  r.w_batched = hnet_batch_w(p);
  r.ln_fused = h.W == 128;
  // (a dry pass measures the per-layer products and the one-by-one T preparation: the chains and the batched preparation
  // need no scratch of their own)
  if (c.dry) return r;
  r.T_batched = hnet_T_batched(h, p, /*backward=*/false, 2, 0);
  r.chained = r.w_batched && wprep_image_floats() != 0 && p->n_fc + 1 <= CHAIN_MAX &&
              hnet_forward_chain_descs(c, h, p, hin, sv, y, cds);
  return r;
}

static int hnet_forward_impl(Ctx& c, int rows, const cgat_hnet_params* p, const float* h0, const float* v, float* y,
                             float* saved) {
  const HnetPlan h = hnet_carve(c, rows, p, /*backward=*/false, nullptr);
  const int W = h.W;
  HnetSaved sv = hnet_saved(saved, rows, p);
  const float* hin = p->damping ? sv.hin() : h0;
  ChainDesc cds[CGAT_MAX_HYPER];
  const HnetFwdRoute r = hnet_fwd_route(c, h, p, hin, sv, y, cds);
  if (r.T_batched) CGAT_TRY(hnet_prepare_T_all(c, h, p, 1, 2, 0));   // T re-laid as Tp[i,k,o]
  if (r.w_batched) CGAT_TRY(hnet_prepare_weights(c));
  if (p->damping) RUN(mix_launch(h0, v, p->damping, sv.hin(), (long)rows * W, c.s));
  if (r.chained)   // every predicted layer's trunk reads the same hyper input: CHAIN_BATCH_MAX chains per launch (round 5)
    for (int l0 = 0; l0 < p->n_hyper; l0 += CHAIN_BATCH_MAX)
      CGAT_TRY(mlp_chain128_batch_launch(cds + l0, p->n_hyper - l0 < CHAIN_BATCH_MAX ? p->n_hyper - l0 : CHAIN_BATCH_MAX, c.s));
  const float* vin = v;
  for (int l = 0; l < p->n_hyper; ++l) {
    const cgat_hyperlinear_params& L = p->layer[l];
    float* u = c.dry ? nullptr : ((l == p->n_hyper - 1) ? y : sv.u(l));
    const float* z = c.dry ? nullptr : sv.act(l, p->n_fc - 1);
    if (r.chained) {   // u holds z @ U^T + b0
      GemmParams g = gemm_params(rows, W, W, vin, W, L.head_b, W, u, W);
      g.beta = 1.f;
      CGAT_TRY(c.gemm(g));
    } else {
      const float* t = hin;
      for (int s = 0; s < p->n_fc; ++s) {  // trunk: Linear + Tanh
        GemmParams g = gemm_params(rows, W, W, t, W, L.fc_w[s], W, c.dry ? nullptr : sv.act(l, s), W);
        g.bias = L.fc_b[s];
        g.act = CGAT_ACT_TANH;
        CGAT_TRY(c.gemm(g));
        t = c.dry ? nullptr : sv.act(l, s);
      }
      // bias-row terms of the head:  u = vin @ Bm^T + z @ U^T + b0
      GemmParams g = gemm_params(rows, W, W, vin, W, L.head_b, W, u, W);
      CGAT_TRY(c.gemm(g));
      g = gemm_params(rows, W, W, z, W, L.head_w + h.WW * W, W, u, W);
      g.bias = L.head_b + h.WW;
      g.beta = 1.f;
      CGAT_TRY(c.gemm(g));
    }
    // trilinear term with T[o,i,k] = head_w[(o*W+i)*W + k] re-laid as Tp[i,k,o]
    float* Tl = h.T(l, r.T_batched);
    if (!r.T_batched) RUN(bilinear_prepare_T(L.head_w, Tl, W, W, W, 1, 2, 0, c.s));
    // (+ LayerNorm + tanh of every layer but the last, fused into the contraction's slab sum at width 128)
    const bool ln = l < p->n_hyper - 1;
    const bool ln_fused = ln && r.ln_fused;
    CGAT_TRY(c.bilinear(vin, W, z, W, Tl, u, W, u, W, rows, W, W, W, (ln_fused && !c.dry) ? sv.vin(l + 1) : nullptr, 1e-5f));
    if (ln) {
      if (!ln_fused) RUN(layernorm_tanh_fwd_launch(u, sv.vin(l + 1), rows, W, 1e-5f, c.s));
      vin = c.dry ? nullptr : sv.vin(l + 1);
    }
  }
  return check_ws(c, "hnet_forward");
}

// =======================================================================================
// backward
// =======================================================================================
// the trunk backward of one predicted layer
enum HnetTrunk {
  TRUNK_LAYERS,        // layer by layer: activation backward, weight gradient, product (what the dry pass sizes)
  TRUNK_CHAIN,         // one chain launch now, accumulating into g_hin
  TRUNK_CHAIN_QUEUED,  // the chain waits for the batched launch of the tail and writes its g_hin term to a slab
};
// the weight (and bias) gradient of one dense layer
enum HnetDw {
  DW_GENERIC,          // generic products + column sum
  DW_ROWS,             // the rows kernel now (rowsdw.hip)
  DW_QUEUED,           // queued for the batched launch of the tail (its operands stay as they are until then)
};
// stream and workspace of that batched launch
enum HnetDwBatch {
  DWB_MAIN,            // main stream, the scratch of the main workspace (the serial backward)
  DWB_MAIN_SIDE_WS,    // main stream; the slabs live in the side workspace, like the operands
  DWB_SIDE,            // side stream, behind the dT launch
};
struct HnetBwdRoute {
  bool T_batched;      // every predicted layer's re-laid T up front in two launches
  bool w_batched;      // every (transposed) dense-layer weight image of the pass in one launch per image kind
  bool dual;           // both bilinear parts of the head's input gradients from ONE contraction (else: two bilinear ones)
  bool dw_wait;        // dense weight gradients on 16-byte aligned operands wait for the batched launch (hnet_defer_dw)
  bool dT_side;        // the dT launch on the side stream, on `wgrad_wgs` workgroups (the overlapped backward)
  bool early_prep;     // ... its operands prepared per layer on the side stream as soon as the layer's gu exists
  HnetDwBatch dw_batch;
  struct Layer {
    HnetTrunk trunk;
    HnetDw head_dw;                  // Bm, U and bias gradients of the head: gu^T [vin | z]
    HnetDw trunk_dw[CGAT_MAX_FC];    // trunk layer s: g_pre_s^T (its input rows)
  } layer[CGAT_MAX_HYPER];
};

// backward: what its steps share -- the carved buffers, the operands, the route's chain descriptors and the three queues
// that wait for a batched launch in the tail
struct HnetBwd {
  HnetPlan h;
  const cgat_hnet_params* p;
  const cgat_hnet_grads* gr;
  const HnetSide* side;
  HnetSaved sv;
  const float* hin;
  ChainDesc chain[CGAT_MAX_HYPER];        // layer l's trunk chain where the route runs one (hnet_trunk_chain_desc)
  DwBatchDesc dwb;                        // dense-layer weight gradients (rowsdw.hip)
  ChainDesc pending[CHAIN_BATCH_MAX];     // trunk chains (TRUNK_CHAIN_QUEUED); chain i writes slab i of ghin_slabs
  int n_pending;
  const float *dT_gu[CGAT_MAX_HYPER], *dT_vin[CGAT_MAX_HYPER], *dT_z[CGAT_MAX_HYPER];   // dT: all predicted layers in one launch
  float* dT_out[CGAT_MAX_HYPER];
  int n_deferred;
  const float* below(int l, int s) const { return s == 0 ? hin : sv.act(l, s - 1); }   // input rows of trunk layer s
  const float* vin(int l, const float* v) const { return l == 0 ? v : sv.vin(l); }     // input rows of predicted layer l
};

static HnetDw hnet_dw_form(bool wait, int W, const float* G, const float* X1, const float* X2) {
  if (!rows_dw128_fast(G, W, X1, W, X2, X2 ? W : 0)) return DW_GENERIC;
  return wait ? DW_QUEUED : (W == 128 ? DW_ROWS : DW_GENERIC);
}

// The trunk backward of predicted layer l as one chain on the transposed weight images (chain.hip): rows = g_t *
// tanh'(t_last) = the last layer's pre-activation gradient, layer i multiplies by W_(n_fc-1-i) and by tanh' of the
// activation below it, every pre-activation gradient is stored for the weight-gradient kernel, the last product is added
// to g_hin -- or, `slab` given, written there.  Says whether the chain kernel takes it.
static bool hnet_trunk_chain_desc(const Ctx& c, const HnetBwd& b, int l, float* slab, ChainDesc& cd) {
  const HnetPlan& h = b.h;
  const int W = h.W, nf = b.p->n_fc;
  const size_t rw = h.rw;
  float* g_pre = h.g_pre(l);
  memset(&cd, 0, sizeof(cd));
  cd.n_layers = nf; cd.rows = h.rows; cd.x = h.g_t(l); cd.ldx = W;
  cd.in_dact = b.sv.act(l, nf - 1); cd.ld_in_dact = W; cd.in_dact_type = CGAT_ACT_TANH;
  cd.in_store = g_pre + (size_t)(nf - 1) * rw; cd.ld_in_store = W;
  for (int i = 0; i < nf; ++i) {
    const int sl = nf - 1 - i;                      // trunk layer whose weight this chain layer multiplies by
    ChainLayer& cl = cd.layer[i];
    cl.W = (const uint4*)c.wprep_find(b.p->layer[l].fc_w[sl], 1, W);
    if (!cl.W) return false;
    cl.act = CGAT_ACT_NONE;
    cl.ld_out = W;
    if (sl > 0) {
      cl.dact = b.sv.act(l, sl - 1); cl.ld_dact = W; cl.dact_type = CGAT_ACT_TANH;
      cl.out = g_pre + (size_t)(sl - 1) * rw;
    } else if (slab) {
      cl.out = slab;                                // (summed in the tail, in queue order)
    } else {
      cl.out = h.g_hin; cl.accumulate = 1;          // every predicted layer's trunk reads the same hyper input
    }
  }
  return mlp_chain128_fast(cd);
}

// b: carved, operands set, queues empty.  Fills b.chain[l] for every layer whose route is a chain.
static HnetBwdRoute hnet_bwd_route(const Ctx& c, HnetBwd& b, const float* v, const float* g_y) {
  const HnetPlan& h = b.h;
  const cgat_hnet_params* p = b.p;
  const int W = h.W, nf = p->n_fc;
  HnetBwdRoute r = {};
  r.w_batched = hnet_batch_w(p);
  r.dual = bilinear_dual_fast(W, W, W);
  r.dw_wait = hnet_defer_dw(p);
  // A dry pass sizes the layer-by-layer trunk and the rows kernel: a chain needs no scratch, hnet_carve has asked for the
  // batched weight-gradient launch and the per-layer one where gradients wait, and run_sized sizes with no side stream.
  for (int l = 0; l < p->n_hyper; ++l) {
    r.layer[l].trunk = TRUNK_LAYERS;
    r.layer[l].head_dw = r.dw_wait ? DW_QUEUED : (W == 128 ? DW_ROWS : DW_GENERIC);
    for (int s = 0; s < nf; ++s) r.layer[l].trunk_dw[s] = W == 128 ? DW_ROWS : DW_GENERIC;
  }
  if (c.dry) return r;
  r.T_batched = hnet_T_batched(h, p, /*backward=*/true, 0, 2);
  const bool chain_ok = hnet_chain_ok(p), chain_batch = hnet_chain_batch(h.rows, p);
  const float *q[CGAT_MAX_HYPER], *z[CGAT_MAX_HYPER];
  int n_queued = 0;
  for (int l = p->n_hyper - 1; l >= 0; --l) {   // (the order the loop runs in: a queued chain's slab is its place in the queue)
    HnetBwdRoute::Layer& L = r.layer[l];
    q[l] = b.vin(l, v); z[l] = b.sv.act(l, nf - 1);
    const float* gu = l == p->n_hyper - 1 ? g_y : (b.side ? (float*)b.side->ws : h.g_u) + (size_t)l * h.rw;
    L.head_dw = hnet_dw_form(r.dw_wait, W, gu, q[l], z[l]);
    // (queued: a weight gradient that cannot wait for the batched launch would read g_pre before the chain has run)
    bool queue = chain_batch;
    for (int s = 0; s < nf; ++s) queue = queue && rows_dw128_fast(h.g_pre(l) + (size_t)s * h.rw, W, b.below(l, s), W, nullptr, 0);
    const bool chain = chain_ok &&
                       hnet_trunk_chain_desc(c, b, l, queue ? h.ghin_slabs + (size_t)n_queued * h.rw : nullptr, b.chain[l]);
    L.trunk = !chain ? TRUNK_LAYERS : queue ? TRUNK_CHAIN_QUEUED : TRUNK_CHAIN;
    if (L.trunk == TRUNK_CHAIN_QUEUED) ++n_queued;
    for (int s = 0; s < nf; ++s)   // (layer by layer, g_pre is ONE buffer for all trunk layers: no weight gradient can wait)
      L.trunk_dw[s] = hnet_dw_form(chain && r.dw_wait, W, h.g_pre(l) + (chain ? (size_t)s * h.rw : 0), b.below(l, s), nullptr);
  }
  // Capacity of the queues: under hnet_defer_dw a predicted layer queues at most n_fc + 2 weight gradients and
  // n_hyper * (n_fc + 2) <= DW_BATCH_MAX; under hnet_chain_batch at most n_hyper <= CHAIN_BATCH_MAX chains wait.  So the
  // steps that queue check their capacity as an invariant, not as a route.
  r.dT_side = b.side != nullptr;
  // (small batches: 9 more launches cost more than they hide; and only where the batched kernel will take the operands)
  r.early_prep = b.side && h.rows >= 16384 && bilinear_wgrad_batch_takes(p->n_hyper, p->n_hyper, q, W, z, W, h.rows, W, W, W);
  // The batched dense-layer weight gradients: f16x3 -- main stream (behind the dT launch on the side stream the batch
  // collided with the matrix-bound edge_ge: 24.14 vs 23.95 ms per step); f16x3c -- side stream (the 24-bit dT launch is
  // twice as long and still running when edge_ge starts either way: 29.0-29.4 vs 29.5 ms, serial order 29.9-30.0;
  // profiles/r05_side_stream_sweep.txt)
  r.dw_batch = !b.side ? DWB_MAIN : mode_f16c() ? DWB_SIDE : DWB_MAIN_SIDE_WS;
  return r;
}

// Weight (and bias) gradients of one dense layer in the route's form: out1 = G^T X1 (and out2 = G^T X2 when X2 is given),
// bsum = column sums of G.
static int dense_wgrad(Ctx& c, HnetBwd& b, HnetDw form, const float* G, const float* X1, float* out1, const float* X2,
                       float* out2, float* bsum) {
  const int W = b.h.W, rows = b.h.rows;
  switch (form) {
    case DW_QUEUED:
      if (c.dry) return CGAT_OK;   // (hnet_carve has sized the batched launch and the per-layer one)
      CGAT_CHECK_ARG(b.dwb.n + (X2 ? 2 : 1) <= DW_BATCH_MAX, "hnet_backward: more than %d queued weight gradients", DW_BATCH_MAX);
      b.dwb.it[b.dwb.n++] = {G, X1, out1, bsum};
      if (X2) b.dwb.it[b.dwb.n++] = {G, X2, out2, nullptr};
      return CGAT_OK;
    case DW_ROWS: {
      const int rc_ = c.dw128(G, W, X1, W, out1, W, X2, X2 ? W : 0, out2, X2 ? W : 0, bsum, rows);
      CGAT_CHECK_ARG(rc_ >= 0, "hnet_backward: the rows kernel does not take a weight gradient routed to it");
      return rc_;
    }
    case DW_GENERIC: {
      GemmParams g = gemm_params(W, W, rows, G, W, X1, W, out1, W);
      g.a_kmajor = 1; g.b_kmajor = 1;
      CGAT_TRY(c.gemm(g, true));
      if (X2) {
        g = gemm_params(W, W, rows, G, W, X2, W, out2, W);
        g.a_kmajor = 1; g.b_kmajor = 1;
        CGAT_TRY(c.gemm(g, true));
      }
      return c.colsum(G, W, rows, W, bsum, 1.f);
    }
  }
  return CGAT_ERR_ARG;
}

// ---- head parameter gradients of predicted layer l ----
static int hnet_head_param_grads(Ctx& c, HnetBwd& b, const HnetBwdRoute& r, int l, const float* gu, const float* vin,
                                 const float* z) {
  const HnetPlan& h = b.h;
  const int W = h.W;
  const cgat_hyperlinear_grads& G = b.gr->layer[l];
  // dT[o][i][k] = sum_n gu[n,o] vin[n,i] z[n,k]: deferred, all predicted layers in one launch (hnet_backward_tail)
  b.dT_gu[b.n_deferred] = gu; b.dT_vin[b.n_deferred] = vin; b.dT_z[b.n_deferred] = z; b.dT_out[b.n_deferred++] = G.head_w;
  // its operands are prepared (maxima, scaled transposes, fp16 planes: HBM-bound, 0.25 ms a layer) on the side stream as
  // soon as the layer's gu exists, beside that layer's matrix-bound contraction on the main stream, so that the dT launch
  // itself can start the moment the backward has issued its last kernel
  if (r.early_prep) {
    CGAT_TRY(stream_wait_stream(b.side->s, c.s));
    const int rc_ = bilinear_wgrad_batch_prep(b.n_deferred - 1, b.p->n_hyper, gu, W, vin, W, z, W, h.rows, W, W, W,
                                              (char*)b.side->ws + h.SL.wgrad, b.side->bytes - h.SL.wgrad, b.side->s);
    CGAT_CHECK_ARG(rc_ != CGAT_ERR_UNSUPPORTED, "hnet_backward: the batched dT does not take operands routed to it");
    CGAT_TRY(rc_);
  }
  // Bm grad [o][i] = gu^T vin, U grad [o][k] = gu^T z, bias grad = column sums of gu: one pass over the three operands
  return dense_wgrad(c, b, r.layer[l].head_dw, gu, vin, G.head_b, z, G.head_w + h.WW * W, G.head_b + h.WW);
}

// ---- the head's input gradients: g_t = g_z (wrt the trunk output), g_vin (wrt the layer's input) ----
static int hnet_head_input_grads(Ctx& c, const HnetBwd& b, const HnetBwdRoute& r, int l, const float* gu, const float* vin,
                                 const float* z, float* g_t, float* g_vin) {
  const HnetPlan& h = b.h;
  const int W = h.W, rows = h.rows;
  const cgat_hyperlinear_params& L = b.p->layer[l];
  {  // g_z = gu @ U + sum_{o,i} gu[o] vin[i] T[o,i,k]
    GemmParams g = gemm_params(rows, W, W, gu, W, L.head_w + h.WW * W, W, g_t, W);
    g.b_kmajor = 1;
    CGAT_TRY(c.gemm(g));
  }
  {  // g_vin = gu @ Bm + sum_{o,k} gu[o] z[k] T[o,i,k]
    GemmParams g = gemm_params(rows, W, W, gu, W, L.head_b, W, g_vin, W);
    g.b_kmajor = 1;
    CGAT_TRY(c.gemm(g));
  }
  if (r.dual) {
    // both bilinear parts from one contraction: M[n,i,k] = sum_o gu[o] T[o,i,k];  g_z += vin . M,  g_vin += M . z
    float* Tl = h.T(l, r.T_batched);
    if (!r.T_batched) RUN(bilinear_prepare_T(L.head_w, Tl, W, W, W, 1, 0, 2, c.s));   // operand [a = i][b = o][c = k]
    CGAT_TRY(c.dual(vin, W, gu, W, z, W, Tl, g_t, W, g_t, W, g_vin, W, g_vin, W, rows));
  } else {
    RUN(bilinear_prepare_T(L.head_w, h.Tp, W, W, W, 0, 1, 2, c.s));
    CGAT_TRY(c.bilinear(gu, W, vin, W, h.Tp, g_t, W, g_t, W, rows, W, W, W));
    RUN(bilinear_prepare_T(L.head_w, h.Tp, W, W, W, 0, 2, 1, c.s));   // T re-laid as [o,k,i]
    CGAT_TRY(c.bilinear(gu, W, z, W, h.Tp, g_vin, W, g_vin, W, rows, W, W, W));
  }
  return CGAT_OK;
}

// ---- trunk backward of predicted layer l (g_t holds the gradient wrt the trunk output z) ----
// the route's chain (hnet_trunk_chain_desc), launched now or queued for the batched launch of the tail; then the weight
// gradients on the pre-activation gradients it leaves (or will have left) in g_pre
static int hnet_trunk_backward_chain(Ctx& c, HnetBwd& b, const HnetBwdRoute& r, int l, const float* g_pre) {
  const cgat_hyperlinear_grads& G = b.gr->layer[l];
  if (r.layer[l].trunk == TRUNK_CHAIN_QUEUED) {
    CGAT_CHECK_ARG(b.n_pending < CHAIN_BATCH_MAX, "hnet_backward: more than %d queued trunk chains", CHAIN_BATCH_MAX);
    b.pending[b.n_pending++] = b.chain[l];
  } else {
    CGAT_TRY(mlp_chain128_launch(b.chain[l], c.s));
  }
  for (int s = b.p->n_fc - 1; s >= 0; --s)
    CGAT_TRY(dense_wgrad(c, b, r.layer[l].trunk_dw[s], g_pre + (size_t)s * b.h.rw, b.below(l, s), G.fc_w[s], nullptr, nullptr,
                         G.fc_b[s]));
  return CGAT_OK;
}

// ... or layer by layer (what the dry pass sizes): g_pre is ONE buffer for all trunk layers, no weight gradient can wait
static int hnet_trunk_backward_layers(Ctx& c, HnetBwd& b, const HnetBwdRoute& r, int l, float* g_t, float* g_pre) {
  const HnetPlan& h = b.h;
  const int W = h.W, rows = h.rows;
  const cgat_hyperlinear_params& L = b.p->layer[l];
  const cgat_hyperlinear_grads& G = b.gr->layer[l];
  for (int s = b.p->n_fc - 1; s >= 0; --s) {
    const float* tout = c.dry ? nullptr : b.sv.act(l, s);
    const float* tin = (s == 0) ? b.hin : (c.dry ? nullptr : b.sv.act(l, s - 1));
    RUN(act_bwd_launch(tout, g_t, g_pre, (long)h.rw, CGAT_ACT_TANH, c.s));
    CGAT_TRY(dense_wgrad(c, b, r.layer[l].trunk_dw[s], g_pre, tin, G.fc_w[s], nullptr, nullptr, G.fc_b[s]));
    GemmParams g = gemm_params(rows, W, W, g_pre, W, L.fc_w[s], W, s == 0 ? h.g_hin : g_t, W);
    g.b_kmajor = 1;
    g.beta = (s == 0) ? 1.f : 0.f;  // every predicted layer's trunk reads the same hyper input
    CGAT_TRY(c.gemm(g));
  }
  return CGAT_OK;
}

// ---- behind the loop: the three queues, and the gradient of the hyper input ----
static int hnet_backward_tail(Ctx& c, HnetBwd& b, const HnetBwdRoute& r, const float* h0, const float* v, float* g_h0,
                              float* g_v) {
  const HnetPlan& h = b.h;
  const HnetSide* side = b.side;
  const int W = h.W, rows = h.rows;
  if (b.n_pending > 0) {
    CGAT_TRY(mlp_chain128_batch_launch(b.pending, b.n_pending, c.s));
    if (b.n_pending == b.p->n_hyper) {   // (g_hin was zero: 0.f + c_last + ... + c_0)
      RUN(sum_slabs_launch(h.ghin_slabs, b.n_pending, (long)h.rw, h.g_hin, (long)h.rw, c.s));
    } else {      // some layer took the accumulating route: add the slabs to what it left
      for (int z = 0; z < b.n_pending; ++z) RUN(axpy_launch(h.g_hin, h.ghin_slabs + (size_t)z * h.rw, 1.f, (long)h.rw, c.s));
    }
  }
  if (b.p->damping) {
    CGAT_TRY(c.mix_bwd(h.g_hin, h0, v, b.p->damping, g_h0, g_v, b.gr->damping, (long)h.rw));
  } else {
    RUN(copy2d_launch(h.g_hin, W, g_h0, W, rows, W, c.s));
  }
  bool side_waits = false;   // the side stream has been made to wait for everything issued above
  auto side_wait = [&]() -> int {
    if (side_waits) return CGAT_OK;
    side_waits = true;
    return stream_wait_stream(side->s, c.s);
  };
  if (b.n_deferred > 0) {
    if (r.dT_side) {
      // On the side stream the dT launch starts when everything above has been issued on the main stream, i.e. together
      // with whatever the caller enqueues next (the HBM-bound attention backward), on `wgrad_wgs` workgroups.
      CGAT_TRY(side_wait());
      CGAT_TRY(bilinear_wgrad_batch_launch(b.n_deferred, b.dT_gu, W, b.dT_vin, W, b.dT_z, W, b.dT_out, rows, W, W, W,
                                           (char*)side->ws + h.SL.wgrad, side->bytes - h.SL.wgrad, side->s, side->wgrad_wgs,
                                           r.early_prep));
    } else {
      CGAT_TRY(c.wgrad_batch(b.n_deferred, b.dT_gu, b.dT_vin, b.dT_z, b.dT_out, rows, W));
    }
  }
  if (b.dwb.n > 0) {
    // HBM-bound, 0.7 ms for 24 products at 83 340 rows; in f16x3 on the main stream, right here.  On the side stream
    // (f16x3c) it goes BEHIND the dT launch: that launch must be resident before the caller's next kernel floods
    // the chip with small workgroups (its 132-KB workgroups are not placed while those keep arriving -- measured: 9.5 ms
    // instead of 6.2 when it started 0.7 ms later), and there it ends up beside the matrix-bound edge_ge (1.3 -> 2.5 ms)
    switch (r.dw_batch) {
      case DWB_SIDE:
        CGAT_TRY(side_wait());
        CGAT_TRY(rows_dw128_batch_launch(b.dwb, (char*)side->ws + h.SL.dw, h.SL.wgrad - h.SL.dw, side->s));
        break;
      case DWB_MAIN_SIDE_WS:
        CGAT_TRY(rows_dw128_batch_launch(b.dwb, (char*)side->ws + h.SL.dw, h.SL.wgrad - h.SL.dw, c.s));
        break;
      case DWB_MAIN:
        CGAT_TRY(rows_dw128_batch_launch(b.dwb, c.scratch, c.scratch_bytes, c.s));
        break;
    }
  }
  return CGAT_OK;
}

// the carved buffers and the operands, the queues empty: what hnet_bwd_route decides on
static HnetBwd hnet_bwd_carve(Ctx& c, int rows, const cgat_hnet_params* p, const float* h0, const float* saved,
                              const cgat_hnet_grads* gr, const HnetSide* side) {
  HnetBwd b = {};
  b.h = hnet_carve(c, rows, p, /*backward=*/true, side);
  b.p = p; b.gr = gr; b.side = side;
  b.dwb.rows = rows; b.dwb.ldg = p->W; b.dwb.ldx = p->W; b.dwb.ldo = p->W;
  b.sv = hnet_saved(const_cast<float*>(saved), rows, p);
  b.hin = p->damping ? b.sv.hin() : h0;
  return b;
}

static int hnet_backward_impl(Ctx& c, int rows, const cgat_hnet_params* p, const float* h0, const float* v,
                              const float* saved, const float* g_y, float* g_h0, float* g_v,
                              const cgat_hnet_grads* gr, const HnetSide* side = nullptr) {
  HnetBwd b = hnet_bwd_carve(c, rows, p, h0, saved, gr, side);
  const HnetPlan& h = b.h;
  const int W = h.W;
  const HnetBwdRoute r = hnet_bwd_route(c, b, v, g_y);
  if (r.w_batched) CGAT_TRY(hnet_prepare_weights(c));
  if (r.T_batched) CGAT_TRY(hnet_prepare_T_all(c, h, p, 1, 0, 2));   // the [a = i][b = o][c = k] operands
  RUN(fill_launch(h.g_hin, 0.f, (long)h.rw, c.s));
  const float* gout = g_y;  // gradient wrt the output of predicted layer l (post norm for l < last)
  for (int l = p->n_hyper - 1; l >= 0; --l) {
    const float* gu = gout;  // gradient wrt the pre-norm output u_l
    if (l < p->n_hyper - 1) {
      float* gu_buf = c.dry ? nullptr : ((side ? (float*)side->ws : h.g_u) + (size_t)l * h.rw);
      RUN(layernorm_tanh_bwd_launch(b.sv.u(l), b.sv.vin(l + 1), gout, gu_buf, rows, W, 1e-5f, c.s));
      gu = gu_buf;
    }
    float* g_vin = (l == 0) ? g_v : h.gvin_buf[l & 1];  // gradient wrt this layer's input
    float* g_t = c.dry ? nullptr : h.g_t(l);
    float* g_pre = c.dry ? nullptr : h.g_pre(l);
    const float* vin = b.vin(l, v);
    const float* z = c.dry ? nullptr : b.sv.act(l, p->n_fc - 1);
    CGAT_TRY(hnet_head_param_grads(c, b, r, l, gu, vin, z));
    CGAT_TRY(hnet_head_input_grads(c, b, r, l, gu, vin, z, g_t, g_vin));
    if (r.layer[l].trunk == TRUNK_LAYERS) CGAT_TRY(hnet_trunk_backward_layers(c, b, r, l, g_t, g_pre));
    else CGAT_TRY(hnet_trunk_backward_chain(c, b, r, l, g_pre));
    gout = g_vin;
  }
  CGAT_TRY(hnet_backward_tail(c, b, r, h0, v, g_h0, g_v));
  return check_ws(c, "hnet_backward");
}

extern "C" size_t cgat_hnet_forward_workspace_bytes(int32_t rows, const cgat_hnet_params* p) {
  return dry_total([&](Ctx& c) { return hnet_forward_impl(c, rows, p, nullptr, nullptr, nullptr, nullptr); });
}
extern "C" size_t cgat_hnet_backward_workspace_bytes(int32_t rows, const cgat_hnet_params* p) {
  cgat_hnet_grads g = {};
  return dry_total([&](Ctx& c) { return hnet_backward_impl(c, rows, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &g); });
}
extern "C" int cgat_hnet_forward(int32_t rows, const cgat_hnet_params* p, const float* h0, const float* v, float* y,
                                 float* saved, void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(hnet_check(rows, p));
  return run_sized("hnet_forward", ws, ws_bytes, stream,
                   [&](Ctx& c) { return hnet_forward_impl(c, rows, p, h0, v, y, saved); });
}
extern "C" size_t cgat_hnet_backward_side_workspace_bytes(int32_t rows, const cgat_hnet_params* p) {
  return hnet_side_layout(rows, p).total;
}
extern "C" int cgat_hnet_backward_overlapped(int32_t rows, const cgat_hnet_params* p, const float* h0, const float* v,
                                             const float* saved, const float* g_y, float* g_h0, float* g_v,
                                             const cgat_hnet_grads* g, void* ws, size_t ws_bytes, void* stream,
                                             void* side_ws, size_t side_ws_bytes, void* side_stream) {
  CGAT_TRY(hnet_check(rows, p));
  CGAT_CHECK_ARG(g, "hnet_backward: null grads");
  CGAT_CHECK_ARG(side_stream && side_ws && side_ws_bytes >= hnet_side_layout(rows, p).total,
                 "hnet_backward_overlapped: side stream / workspace missing or too small");
  // 128 workgroups: half of the chip stays free for the main stream's HBM-bound kernels
  const HnetSide side = {(hipStream_t)side_stream, side_ws, side_ws_bytes, /*wgrad_wgs=*/128};
  // (sized as cgat_hnet_backward_workspace_bytes sizes it: the main workspace of the serial backward)
  return run_sized("hnet_backward", ws, ws_bytes, stream, [&](Ctx& c) {
    return hnet_backward_impl(c, rows, p, h0, v, saved, g_y, g_h0, g_v, g, c.dry ? nullptr : &side);
  });
}
extern "C" int cgat_hnet_backward(int32_t rows, const cgat_hnet_params* p, const float* h0, const float* v,
                                  const float* saved, const float* g_y, float* g_h0, float* g_v,
                                  const cgat_hnet_grads* g, void* ws, size_t ws_bytes, void* stream) {
  CGAT_TRY(hnet_check(rows, p));
  CGAT_CHECK_ARG(g, "hnet_backward: null grads");
  return run_sized("hnet_backward", ws, ws_bytes, stream,
                   [&](Ctx& c) { return hnet_backward_impl(c, rows, p, h0, v, saved, g_y, g_h0, g_v, g); });
}

// ---- debug: the route of a pass as a bit mask (include/cgat_hip.h), for 16-byte aligned operands: the carve and route
// functions of the real pass over a null, unbounded workspace.  Host only.  Every predicted layer takes the same forms
// on such operands; the mask names those of layer 0 ----
extern "C" uint32_t cgat_debug_hnet_route(int32_t rows, const cgat_hnet_params* p, int32_t backward, int32_t overlapped) {
  if (hnet_check(rows, p) != CGAT_OK) return 0;
  // (a non-null aligned base: no carve-out is a null pointer, as none is in a real pass; nothing is dereferenced)
  Ctx c((void*)256, (size_t)-1 / 2, false, nullptr);
  if (!backward) {
    const HnetPlan h = hnet_carve(c, rows, p, /*backward=*/false, nullptr);
    ChainDesc cds[CGAT_MAX_HYPER];
    const HnetFwdRoute r = hnet_fwd_route(c, h, p, nullptr, hnet_saved(nullptr, rows, p), nullptr, cds);
    return route_bits({r.T_batched, r.w_batched, r.chained, r.ln_fused});
  }
  const HnetSide side = {nullptr, (void*)256, (size_t)-1 / 2, 128};
  cgat_hnet_grads g = {};
  HnetBwd b = hnet_bwd_carve(c, rows, p, nullptr, nullptr, &g, overlapped ? &side : nullptr);
  const HnetBwdRoute r = hnet_bwd_route(c, b, nullptr, nullptr);
  const HnetBwdRoute::Layer& L = r.layer[0];
  return route_bits({r.T_batched, r.w_batched, r.dual, L.trunk == TRUNK_CHAIN, L.trunk == TRUNK_CHAIN_QUEUED,
                     r.dw_wait, L.head_dw == DW_QUEUED, L.head_dw == DW_ROWS, r.dT_side,
                     r.early_prep, r.dw_batch == DWB_SIDE, r.dw_batch == DWB_MAIN_SIDE_WS});
}
