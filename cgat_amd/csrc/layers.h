// What the orchestrator files (layers.hip: the node and edge layers; hnet.hip: the hypernetwork) share: the launch
// context over the caller's workspace, the "size, check, run" wrapper and the helpers of the route structs.
// Host code only; every function is file-local to the orchestrator that includes this.
#pragma once
#include <string.h>

#include <initializer_list>

#include "../../include/cgat_hip.h"
#include "common.h"
#include "kernels.h"
#include "mfma_bf16.h"

// ---------------------------------------------------------------------------------------
// launch context: persistent workspace carve-outs + one scratch region shared (in stream
// order) by split-K slabs / column-sum partials.  `dry` only measures.
// ---------------------------------------------------------------------------------------
struct Ctx {
  Workspace w;
  bool dry;
  hipStream_t s;
  size_t scratch_need;
  char* scratch;
  size_t scratch_bytes;
  // 128 x 128 dense-layer weights prepared ahead in one launch (f16x3 mode): looked up by (pointer, strides) in gemm()
  WPrepBatch wprep;
  float* wprep_images;
  // ... and, in the 24-bit modes, the dense-layer kernel's own images (three bf16 planes) of the weights gemm() multiplies
  // by: one launch for all of them instead of one per product
  WPrepBatch tprep;
  float* tprep_images;
  Ctx(void* ws, size_t bytes, bool dry_, hipStream_t st)
      : w(dry_ ? nullptr : ws, dry_ ? (size_t)-1 / 2 : bytes), dry(dry_), s(st), scratch_need(0), scratch(nullptr),
        scratch_bytes(0), wprep_images(nullptr), tprep_images(nullptr) { wprep.n = 0; tprep.n = 0; }
  void tprep_reserve(int max_items) { tprep_images = take<float>((size_t)max_items * 24576); }
  void tprep_add(const float* W, long so, long sk) {
    if (tprep.n < WPREP_MAX) { tprep.src[tprep.n] = W; tprep.sb[tprep.n] = sk; tprep.sc[tprep.n] = so; ++tprep.n; }
  }
  int tprep_run() {
    if (dry || !mode_24bit() || tprep.n == 0 || !tprep_images) { if (!mode_24bit()) tprep.n = 0; return CGAT_OK; }
    return prepare_T_bf16_batch_launch(tprep, tprep_images, s);
  }
  const void* tprep_find(const float* W, long so, long sk) const {
    if (dry || !mode_24bit() || !tprep_images) return nullptr;
    for (int i = 0; i < tprep.n; ++i)
      if (tprep.src[i] == W && tprep.sb[i] == sk && tprep.sc[i] == so) return tprep_images + (size_t)i * 24576;
    return nullptr;
  }
  // call before seal(): reserves the image space; add items, then wprep_run() once
  // (images of the current arithmetic mode: the fp16 chain's in "f16x3", the six-pass bf16 chain's in the 24-bit modes;
  // the space is reserved for the larger of the two so that a size query does not depend on the mode)
  void wprep_reserve(int max_items) { wprep_images = take<float>((size_t)max_items * WPREP_IMAGE_FLOATS_MAX); }
  void wprep_add(const float* W, long so, long sk) {
    if (wprep.n < WPREP_MAX) { wprep.src[wprep.n] = W; wprep.sb[wprep.n] = sk; wprep.sc[wprep.n] = so; ++wprep.n; }
  }
  int wprep_run() {
    if (dry || wprep_image_floats() == 0 || wprep.n == 0) { if (wprep_image_floats() == 0) wprep.n = 0; return CGAT_OK; }
    return prepare_W_batch_launch(wprep, wprep_images, s);
  }
  const void* wprep_find(const float* W, long so, long sk) const {
    if (dry || wprep_image_floats() == 0) return nullptr;
    for (int i = 0; i < wprep.n; ++i)
      if (wprep.src[i] == W && wprep.sb[i] == sk && wprep.sc[i] == so) return wprep_images + (size_t)i * wprep_image_floats();
    return nullptr;
  }
  template <typename T>
  T* take(size_t n) { return w.take<T>(n); }
  void seal() {  // everything after the persistent carve-outs is scratch
    if (!dry) {
      scratch = w.base + w.off;
      scratch_bytes = w.cap > w.off ? w.cap - w.off : 0;
    }
  }
  size_t total() const { return w.off + scratch_need + 256; }
  void need(size_t b) { if (b > scratch_need) scratch_need = b; }

  int gemm(GemmParams p, bool auto_split = false) {
    if (auto_split) p.splits = gemm_pick_splits(p.M, p.N, p.K);
    if (p.splits > 1) need(ws_round((size_t)p.splits * p.M * p.N, 4));
    // [rows,128] x [128,128] dense layers (trunks, linear terms of the predicted layers): the split-bf16 kernel
    const bool dense128 = p.K == 128 && p.N >= 128 && p.N % 128 == 0 && !p.a_kmajor && !p.a_rgather && !p.a_block && !p.b_kgather &&
                          !p.c_scatter && !p.add1 && !p.add2 && p.splits <= 1 && p.alpha == 1.f &&
                          (p.beta == 0.f || p.beta == 1.f) && (p.act == CGAT_ACT_NONE || p.act == CGAT_ACT_TANH);
    if (dense128) need(linear128_ws_bytes(p.N));
    if (dry) return CGAT_OK;
    // a few hundred rows (the harness' shipped batch): one wave per 16 x 16 output tile straight from global memory
    // (rowprog.hip, exact fp32) -- the 128-row ring tiles below leave 250 of 256 CUs idle there
    if (rowprog_gemm_ok(p)) return rowprog_gemm(p, s);
    if (dense128 && linear128_fast(p.K, p.N, p.lda, p.ldc, p.A, p.C) && scratch_bytes >= linear128_ws_bytes(p.N)) {
      const long so = p.b_kmajor ? 1 : p.ldb, sk = p.b_kmajor ? p.ldb : 1;
      Linear128Params l = linear128_params(p.A, p.lda, p.B, so, sk, p.C, p.ldc, p.M, p.N);
      l.bias = p.bias; l.act = p.act; l.accumulate = p.beta == 1.f;
      l.prepared = p.N != 128 ? nullptr : (mode_f16() ? wprep_find(p.B, so, sk) : tprep_find(p.B, so, sk));
      return linear128_launch(l, scratch, s);
    }
    return gemm_launch(p, scratch, scratch_bytes, s);
  }
  // weight (and bias) gradients of width-128 dense layers: out_k = G^T X_k, bsum = column sums of G (rowsdw.hip);
  // returns -1 if the shape/alignment is not the fast one (caller falls back to gemm + colsum)
  int dw128(const float* G, long ldg, const float* X1, long ldx1, float* out1, long ldo1, const float* X2, long ldx2,
            float* out2, long ldo2, float* bsum, int rows) {
    need(rows_dw128_ws_bytes(rows, X2 ? 2 : 1));
    if (dry) return CGAT_OK;
    if (!rows_dw128_fast(G, ldg, X1, ldx1, X2, ldx2) || scratch_bytes < rows_dw128_ws_bytes(rows, X2 ? 2 : 1)) return -1;
    return rows_dw128_launch(G, ldg, X1, ldx1, out1, ldo1, X2, ldx2, out2, ldo2, bsum, rows, scratch, scratch_bytes, s);
  }
  int colsum(const float* x, long ldx, int rows, int cols, float* out, float alpha) {
    need(colsum_ws_bytes(rows, cols));
    if (dry) return CGAT_OK;
    return colsum_launch(x, ldx, rows, cols, out, alpha, scratch, scratch_bytes, s);
  }
  // all predicted layers' dT in one launch (f16x3) on this context's stream
  int wgrad_batch(int n, const float* const* p, const float* const* q, const float* const* r, float* const* out, int rows,
                  int W) {
    need(bilinear_wgrad_batch_ws_bytes(n, rows, W, W, W));
    if (dry) return CGAT_OK;
    return bilinear_wgrad_batch_launch(n, p, W, q, W, r, W, out, rows, W, W, W, scratch, scratch_bytes, s);
  }
  int bilinear(const float* p, long ldp, const float* q, long ldq, const float* T, const float* init, long ldi,
               float* out, long ldo, int rows, int NA, int NB, int NC, float* ln_out = nullptr, float ln_eps = 0.f) {
    need(bilinear_rows_ws_bytes(rows, NA, NB, NC));
    if (dry) return CGAT_OK;
    return bilinear_rows_launch(p, ldp, q, ldq, T, init, ldi, out, ldo, rows, NA, NB, NC, scratch, scratch_bytes, s,
                                ln_out, ln_eps);
  }
  int dual(const float* p, long ldp, const float* q, long ldq, const float* zz, long ldz, const float* T,
           const float* init1, long ldi1, float* out1, long ldo1, const float* init2, long ldi2, float* out2, long ldo2,
           int rows) {
    need(bilinear_dual_ws_bytes(rows));
    if (dry) return CGAT_OK;
    return bilinear_dual_launch(p, ldp, q, ldq, zz, ldz, T, init1, ldi1, out1, ldo1, init2, ldi2, out2, ldo2, rows,
                                scratch, scratch_bytes, s);
  }
  int mix_bwd(const float* g, const float* a, const float* b, const float* d, float* ga, float* gb, float* gd, long n) {
    need(4096);
    if (dry) return CGAT_OK;
    return mix_bwd_launch(g, a, b, d, ga, gb, gd, n, scratch, scratch_bytes, s);
  }
};

#define RUN(expr) do { if (!c.dry) CGAT_TRY(expr); } while (0)

static int check_ws(const Ctx& c, const char* who) {
  if (c.dry) return CGAT_OK;
  if (!c.w.ok || c.scratch_bytes < c.scratch_need) {
    cgat_set_error("%s: workspace too small (have %zu bytes, need %zu)", who, c.w.cap, c.total());
    return CGAT_ERR_WORKSPACE;
  }
  return CGAT_OK;
}

// "Size, check, run": every entry point that runs an orchestrator measures it with a dry pass, refuses a workspace smaller
// than that, and runs the real pass with the dry pass' scratch requirement carried over; the size queries return what the
// dry pass measured.  `impl` is an int(Ctx&) that calls the orchestrator with the entry point's operands.
template <typename Impl>
static Ctx dry_pass(Impl&& impl) {
  Ctx dry(nullptr, 0, true, nullptr);
  impl(dry);
  return dry;
}
template <typename Impl>
static size_t dry_total(Impl&& impl) { return dry_pass(impl).total(); }
template <typename Impl>
static int run_sized(const char* who, void* ws, size_t ws_bytes, void* stream, Impl&& impl) {
  const Ctx dry = dry_pass(impl);
  if (ws_bytes < dry.total()) {
    cgat_set_error("%s: workspace too small (%zu < %zu)", who, ws_bytes, dry.total());
    return CGAT_ERR_WORKSPACE;
  }
  Ctx c(ws, ws_bytes, false, (hipStream_t)stream);
  c.scratch_need = dry.scratch_need;
  return impl(c);
}

// ---- routes: which launches a pass takes, decided once from the dims, the arithmetic mode and the alignment of the
// operands, and read by every step of the pass.  A dry pass takes no route that depends on an operand: it measures the
// generic steps, and the scratch a fast route needs is asked for by dims alone where that route runs (so the real pass
// tests no scratch size: run_sized has refused a workspace smaller than the dry pass measured).
// `ws` stands for a pass' workspace carve-outs in the kernels' 16-byte tests: Workspace::take places every one a multiple
// of 256 bytes behind the caller's base, so any of them passes exactly when all do (aligned16: kernels.h).

// debug: a route as a bit mask (include/cgat_hip.h), bit i = the i-th flag
static uint32_t route_bits(std::initializer_list<bool> on) {
  uint32_t m = 0, i = 0;
  for (bool b : on) m |= (uint32_t)b << i++;
  return m;
}
