// Internal launch interface between the kernel files and the layer orchestrators.
#pragma once
#include "common.h"

#define CGAT_ACT_NONE 0
#define CGAT_ACT_TANH 1
#define CGAT_ACT_LEAKY 2  // LeakyReLU, slope 0.01 (nn.LeakyReLU() default; reference CGAT.py:95)
#define CGAT_ACT_RELU 3

struct GemmParams {
  int M, N, K;
  const float* A;
  long lda;
  int a_kmajor;          // 0: A(m,k)=A[row(m)*lda+k]   1: A(m,k)=A[k*lda+m]
  const int* a_rgather;  // a_kmajor==0 only: row(m)=a_rgather[m]
  long a_block;          // != 0: A is stored in 128-wide column blocks [cols/128][rows][128] with this block
                         // stride (elements); the blocked dimension is k (a_kmajor==0) or m (a_kmajor==1); lda=128
  const float* B;
  long ldb;
  int b_kmajor;          // 0: B(k,n)=B[n*ldb+k] (torch Linear weight)   1: B(k,n)=B[krow(k)*ldb+n]
  const int* b_kgather;  // b_kmajor==1 only: krow(k)=b_kgather[k]
  float* C;
  long ldc;
  const int* c_scatter;  // output row = c_scatter[m]
  float alpha, beta;     // C = act(alpha*acc + bias + adds) + beta*C
  const float* bias;     // [N]
  const float* add1;     // rows gathered by add1_idx[m], leading dim ld_add
  const int* add1_idx;
  const float* add2;
  const int* add2_idx;
  long ld_add;
  int act;
  int splits;            // >1: split the K range, partial slabs in workspace, then reduce
  // Row-wise outer-product (Khatri-Rao) operands: the bilinear contractions at widths other than 128 as plain products
  //   a_outer (a_kmajor == 0, b_kmajor == 1): A(m,k) = a_outer[m*ld_a_outer + k / outer_n] * A[m*lda + k % outer_n]
  //   b_outer (a_kmajor == 1, b_kmajor == 1): B(k,n) = b_outer[k*ld_b_outer + n / outer_n] * B[k*ldb + n % outer_n]
  const float* a_outer;
  long ld_a_outer;
  const float* b_outer;
  long ld_b_outer;
  int outer_n;
  // filled by gemm_launch
  int k_per_split, a_vec, b_vec, c_vec;
  float* slab;
};

static inline GemmParams gemm_params(int M, int N, int K, const float* A, long lda, const float* B, long ldb, float* C,
                                     long ldc) {
  GemmParams p = {};
  p.M = M; p.N = N; p.K = K;
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc;
  p.alpha = 1.f; p.beta = 0.f; p.splits = 1;
  return p;
}

int gemm_launch(GemmParams p, void* ws, size_t ws_bytes, hipStream_t stream);
// the same product on the bf16 matrix cores (exact three-plane split, six passes: gemmsplit.hip); called by gemm_launch
// in the split arithmetic modes with p's derived fields filled in
int gemm_split_launch(const GemmParams& p, unsigned grid, hipStream_t stream);
int gemm_pick_splits(int M, int N, int K);
// split count for products with <= 32 output tiles and K >= 512 (1 otherwise): see gemm.hip
int gemm_pick_splits_skinny(int M, int N, int K);
// C[m*ldc + n] = act(alpha * sum_z slab[z][m][n] + bias[n]) + beta * C   (fixed summation tree)
int splitk_reduce_launch(const float* slab, int splits, int M, int N, float* C, long ldc, hipStream_t stream,
                         float alpha = 1.f, float beta = 0.f, const float* bias = nullptr, int act = 0);
size_t gemm_ws_bytes(const GemmParams& p);

// ---- small-row products as single-op programs of rowprog.hip (exact fp32 MFMA, no workspace) ----
struct cgat_rowprog_op;
int rowprog_max_rows();                       // env CGAT_ROWPROG_MAX_ROWS, default 2048; 0: never
bool rowprog_gemm_ok(const GemmParams& p);    // plain strided product of at most rowprog_max_rows() rows
int rowprog_gemm(const GemmParams& p, hipStream_t s);
int rowprog_launch(const cgat_rowprog_op* ops, int n_ops, uint32_t* sync_words, hipStream_t s);

// ---- the hypernetwork contractions, bilinear.hip ----
// out[n,c] = init[n,c] + sum_{a<NA,b<NB} p[n,a] q[n,b] T3[a,b,c], with T = bilinear_prepare_T(T3 source) (opimage.hip):
// a permuted copy whose columns are interleaved for the MFMA kernel when NB == NC == 128.
// The arithmetic mode of the matrix-core kernels (values: the C ABI's cgat_set/get_bilinear_mode).
//   F32     f32-input MFMA (exact fp32)
//   F16X3   two fp16 planes per operand, three passes (22-bit operands, scaled per row / per tensor)
//   BF16X3  three bf16 planes, three passes (~3e-6; diagnostic, never the default)
//   F16X3C  (default) 24-bit operands: the fp16 passes of F16X3 plus three 6-bit correction terms (mfma_bf16.h) in the
//           kernels that have that form (the hypernetwork contractions); every other matrix-core kernel runs its
//           six-pass bf16 form, exactly as in BF16X6
//   BF16X6  three bf16 planes, six passes (24-bit operands)
enum ArithMode : int { MODE_F32 = 0, MODE_F16X3 = 2, MODE_BF16X3 = 3, MODE_F16X3C = 4, MODE_BF16X6 = 6 };
int bilinear_mode();               // the current ArithMode
// The decisions the launchers make on it.  Every mode but F32 runs split operands on the matrix cores.
inline bool mode_split() { return bilinear_mode() != MODE_F32; }
// the 22-bit fp16 family: bilinear_rows128_ring16_kernel<2>, edge_zx_kernel, the f16p weight gradient, the fp16 weight images
inline bool mode_f16() { return bilinear_mode() == MODE_F16X3; }
// the corrected fp16 forms of the hypernetwork contractions: ring16c, dualc, bilinear_wgrad128_f16c_kernel
inline bool mode_f16c() { return bilinear_mode() == MODE_F16X3C; }
inline bool mode_bf16x3() { return bilinear_mode() == MODE_BF16X3; }
// 24-bit operands: the six-pass bf16 per-edge and dense forms (edge_z6w, batched heads, rowprog one-launch paths)
inline bool mode_24bit() { const int m = bilinear_mode(); return m == MODE_F16X3C || m == MODE_BF16X6; }
// T operands as fp16-plane images (prepared and differentiated in batches): f16x3 and f16x3c
inline bool mode_f16_T() { const int m = bilinear_mode(); return m == MODE_F16X3 || m == MODE_F16X3C; }
void bilinear_set_mode(int m);
size_t bilinear_rows_ws_bytes(int nrows, int NA, int NB, int NC);
int bilinear_rows_launch(const float* p, long ldp, const float* q, long ldq, const float* T, const float* init,
                         long ldi, float* out, long ldo, int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes,
                         hipStream_t stream, float* ln_out = nullptr, float ln_eps = 0.f);   // ln_out: tanh(LayerNorm(out))
// fused pair (bilinear_rows128_dual_kernel): T = bilinear_prepare_T of the [128,128,128] operand
bool bilinear_dual_fast(int NA, int NB, int NC);
size_t bilinear_dual_ws_bytes(int nrows);
int bilinear_dual_launch(const float* p, long ldp, const float* q, long ldq, const float* zz, long ldz, const float* T,
                         const float* init1, long ldi1, float* out1, long ldo1, const float* init2, long ldi2,
                         float* out2, long ldo2, int nrows, void* ws, size_t ws_bytes, hipStream_t stream);

// ---- the contractions' weight gradient, bilwgrad.hip ----
// out[(a*NB+b)*NC + c] = sum_n p[n,a] q[n,b] r[n,c]      (workspace: slabs)
size_t bilinear_wgrad_ws_bytes(int nrows, int NA, int NB, int NC);
int bilinear_wgrad_launch(const float* p, long ldp, const float* q, long ldq, const float* r, long ldr, float* out,
                          int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream,
                          int force_splits = 0);
// the same for n_layers (<= 8) operand triples in ONE launch (f16x3 mode: batched, software-pipelined kernel; other
// modes: one launch per layer).  max_wgs: grid size (0 = one workgroup per CU; 128 = half of the chip)
size_t bilinear_wgrad_batch_ws_bytes(int n_layers, int nrows, int NA, int NB, int NC);
// host predicate of the batched kernel: q / r = the first n_given layers' operands of an n_layers batch
bool bilinear_wgrad_batch_takes(int n_layers, int n_given, const float* const* q, long ldq, const float* const* r, long ldr,
                                int nrows, int NA, int NB, int NC);
int bilinear_wgrad_batch_launch(int n_layers, const float* const* p, long ldp, const float* const* q, long ldq,
                                const float* const* r, long ldr, float* const* out, int nrows, int NA, int NB, int NC,
                                void* ws, size_t ws_bytes, hipStream_t stream, int max_wgs = 0, bool prepared = false);
// one layer's operand preparation for that launch (slot of n_layers), issued separately -- e.g. early, on a side
// stream; CGAT_ERR_UNSUPPORTED when the batched form does not take the operands
int bilinear_wgrad_batch_prep(int slot, int n_layers, const float* p, long ldp, const float* q, long ldq, const float* r,
                              long ldr, int nrows, int NA, int NB, int NC, void* ws, size_t ws_bytes, hipStream_t stream);

// ---- operand images, opimage.hip ----
// The B operand of bilinear_rows for a [n0,n1,n2] tensor viewed with permuted indices
bool bilinear_T_interleaved(int NB, int NC);
size_t bilinear_T_floats(int NA, int NB, int NC);  // workspace floats of the prepared T
size_t bilinear_T_floats_max(int NA, int NB, int NC);   // ... in whichever arithmetic mode needs most (size queries)
// several tensors in two launches (f16x3 mode at width 128; CGAT_ERR_UNSUPPORTED otherwise -> prepare one by one)
#define TPREP_MAX 8
struct TPrepBatch {
  int n;
  const float* src[TPREP_MAX];
  void* dst[TPREP_MAX];
};
size_t bilinear_prepare_T_batch_ws_floats(int n);
// host predicate of the batched form (mode, count, layout, the CGAT_NO_TPREP_BATCH switch, every source 16-byte aligned)
bool bilinear_prepare_T_batch_takes(int n, const float* const* src, int n0, int n1, int n2, int perm1, int perm2);
int bilinear_prepare_T_batch(int n, const float* const* src, float* const* dst, int n0, int n1, int n2, int perm0,
                             int perm1, int perm2, float* part, hipStream_t stream, int alternate = 1);
int bilinear_prepare_T(const float* src, float* dst, int n0, int n1, int n2, int perm0, int perm1, int perm2,
                       hipStream_t stream);
// Planes of sgn(a) * src[a*sa + b*sb + c*sc] (a < NA; b, c < 128) in the ring kernels' fragment order: three bf16 planes,
// or with tmax (device memory, tmax[0] = max |src|) the two fp16 planes of 2^k src.  heads > 1: head h of a multi-head
// layer reads src + h * s_head and writes (float*)dst + h * image_floats, all in one launch.
int prepare_T_planes_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, int alternate,
                            hipStream_t stream, const float* tmax = nullptr, int heads = 1, long s_head = 0,
                            long image_floats = 0);
// the alternate = 1 image whose first H * Hd / 128 blocks hold wA[b] * src[b][c], and cs[h][c] = the signed column sums
// of head h's scaled rows (the bit-plane form of edge_ge_kernel, edgebwd.hip); one launch
int prepare_T_bf16_attn_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, const float* wA, int H,
                               int Hd, float* cs, hipStream_t stream);
int absmax_launch(const float* src, long n, float* out, hipStream_t stream);   // zeroes out[0] first
int absmax_rows128_launch(const float* t, long ld, int rows, float* out, hipStream_t stream);  // folds into out[0]
// ... on `wgs` workgroups, operands unchecked (t 16-byte aligned, ld % 4 == 0, rows > 0)
int absmax_rows128_wgs_launch(const float* t, long ld, int rows, float* out, int wgs, hipStream_t stream);
// fp16 form for weight operands: planes of 2^k(a) W[a], max |W[a]| in ((float*)dst)[NA * 16384 + a].  heads > 1: that
// many weights of NA blocks each in ONE launch, head h reads src + h * s_head and writes the image (NA planes blocks,
// then NA maxima) at (float*)dst + h * image_floats
int prepare_W_f16_launch(const float* src, void* dst, int NA, long sa, long sb, long sc, hipStream_t stream, int heads = 1,
                         long s_head = 0, long image_floats = 0);
// dst[(a*d1 + b)*d2 + c] = src[...] under an index permutation of a [n0,n1,n2] tensor
int permute3_launch(const float* src, float* dst, int n0, int n1, int n2, int perm0, int perm1, int perm2,
                    int interleave, hipStream_t stream);
// (the batched weight images of the dense layers: below, beside WPrepBatch)

// ---- fused edge pre-activations + attention logits, edgez.hip ----
// 16-byte test of a caller's own pointers (null passes); the dims / leading-dimension / mode half of each predicate is
// a function of its own below
template <typename... P>
static inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }
enum ZStore : int { Z_F32 = 0, Z_BF16 = 1, Z_BITS = 2 };
// Operands of the per-edge family: edge_z_launch, edge_zx_launch, edge_logits_launch, edge_msg_wsum_launch.
//     Z[t, :] = act(We e[perm[t]] + Pi[dsti[t]] + Pj[srci[t]]),   a_out[t, h] = bA[h] + sum_j leaky(Z[t, h Hd + j]) wA[h Hd + j]
struct EdgeZParams {
  const float* e;        // the rows operand [rows, 128], row stride lde
  long lde;
  const int* perm;       // row t reads e[perm[t]] (null: e[t])
  int rows;
  const float* We;       // weight, element (out, k) at We[out * ldw + k]; null: Wq already holds the current mode's image
  long ldw;              //   (prepare_T_planes_launch / prepare_W_f16_launch with edge_z_launch's strides) and is only read
  float* Wq;             // the weight image: edge_z_wq_floats(W2) (edge_zx_launch: edge_zx_wq_floats(W2))
  int W2;                // output columns
  const float* Pi;       // first addend, gathered by dsti; with Pj == null: a bias vector [W2] or null (the plain product)
  const int* dsti;
  const float* Pj;       // second addend, gathered by srci
  const int* srci;
  long ld_add;           // row stride of Pi and Pj
  int n_add_rows;        // rows of Pi / Pj.  0 = unknown: never the 256-row kernel, which addresses them by 32-bit offsets
  float* Z;              // output, row stride ldz in elements whatever the storage; null: logits only (edge_logits_launch)
  long ldz;
  ZStore store;          // Z_BF16: Z stored as bf16; Z_BITS: the attention columns leave sign words in the holes of rows
                         // 2 n_add_rows + g of Z instead of values (edge_z6w_kernel<false, 3>; layers.hip attn_z_form)
  const float* wA;       // the logits: fc_out_A's weight [H * Hd] and bias [H] (nullable), a_out [rows, H] (null: none)
  const float* bA;
  int H, Hd;
  float* a_out;
  int act;               // CGAT_ACT_*
  float* omax;           // max |Z| folded into omax[0] (not zeroed here)
  // edge_zx_launch: the x_j projection folded in (f16x3 mode, C == Ce == 128)
  const float* x;        // [N, 128], row stride ldx, gathered by srci
  long ldx;
  const float* Wj;       // the x_j slice of the stacked weight (row stride ldw)
  // edge_msg_wsum_launch: S[n, :] = sum over the rows of segment n of alpha[t, h] leaky(z_M[t, :])
  int N;
  const float* alpha;    // [rows, H]
  const int* rowptr;     // [N + 1]
  float* S;              // [N, H * Hd]
};
// Which kernel a launch of this family runs, with its template arguments and its grid: decided once per launch by
// edge_z_form (host only; DESIGN.md lists the forms) and read by the launcher, the predicates below and the debug query.
enum EdgeZKernel : int { EZK_NONE = 0, EZK_ROWS128 = 1, EZK_ROWS256 = 2, EZK_MSG_WSUM = 3 };
struct EdgeZForm {
  EdgeZKernel kernel;    // edge_z_kernel (128-row workgroups) / edge_z6w_kernel (256-row) / edge_msg_wsum_kernel; none: no rows
  int passes;            // 2 (two fp16 planes), 3 or 6 (three bf16 planes)
  bool adds;             // edge_z_kernel<., ADDS, .>: gathered addends
  bool zb;               // Z stored (edge_msg_wsum_kernel: rounded) as bf16
  int z6w_mode;          // edge_z6w_kernel<., MODE>: 0 training forward, 3 its bit form, 1 logits only
  int G, ncb_g;          // grid.y column groups and the column blocks of each (G == 1: no groups)
  int grid_x, tile_rows; // row tiles, and the rows of each: 128, 256, or edge_msg_wsum_kernel's R
};
EdgeZForm edge_z_form(const EdgeZParams& p);
// the kernels' dims, leading dimensions and mode: K == 128 inputs, whole 128-column blocks, float4 rows
bool edge_z_dims(int K, int W2, long lde, long ld_add, long ldz);
// ... of a launch over the two stacked networks of H heads: a head is whole column blocks
static inline bool edge_z_heads(int W2, int H, int Hd) { return Hd % 128 == 0 && H * Hd * 2 == W2; }
size_t edge_ge_cs_offset(int W2);  // floats in front of those column sums
size_t edge_z_wq_floats(int W2);   // the three-plane image, then W2 floats for the column sums of edge_ge's bit-plane form
// per-edge launch with the x_j projection folded in (f16x3 mode, C == Ce == 128): edgez.hip edge_zx_kernel
size_t edge_zx_wq_floats(int W2);
bool edge_zx_dims(int C, int Ce, int W2, long ld_add, long ldz);
int edge_zx_launch(const EdgeZParams& p, hipStream_t stream);   // reads We, Wj, x; stores fp32 or bf16
// With Pj == null the kernel computes the plain product Z = e We^T + bias: the per-node projections of the operand split
int edge_z_launch(const EdgeZParams& p, hipStream_t stream);
// would the fp32 training forward of a scalar-attention layer run edge_z6w_kernel (mode, switches, shape; host only)
bool edge_z6w_takes(int N, int E, int H, int Hd);
// Per-head offsets of a launch whose grid.y runs over the heads of a multi-head second layer (elements of each operand;
// w in 16-byte pieces): all zero = the single-operand launch
struct HeadBatch {
  long in, w, bias, out, dact;
  long add2;   // edge_z_kernel: offset of the second gathered table (column groups of the per-edge first layer)
  long ks0;    // edge_ge_kernel<., RC>: k-steps in front of a K group (the rebuilt rows are indexed by k-step, not by pointer);
               // edge_z_kernel with logits: column blocks in front of a column group (head index, fc_out_A's weight)
};
// column blocks of a [rows, 128 ncb] product dealt to grid.y groups when the row tiles alone leave CUs idle: the number
// of groups (a divisor of ncb; 1 = no split)
// (unit: column blocks that must stay in one group -- a head's blocks when the launch also forms that head's logits)
static inline int z_col_groups(int row_tiles, int ncb, int unit = 1) {
  int G = 1;
  if (row_tiles >= 512 || unit < 1) return 1;
  for (int g = 2; g <= ncb; ++g)
    if (ncb % g == 0 && (ncb / g) % unit == 0) { G = g; if ((long)row_tiles * G >= 512) break; }
  return G;
}
// The forward without grad at the shapes of the six-pass per-edge launch (edgez.hip): the logits alone (attention column
// blocks, no Z) and the message blocks reduced straight into S[N, H * Hd] = the softmax-weighted segment sums that
// seg_wsum_launch forms from Z, bit-identical.  edge_infer_fused: the host-only predicate of shapes, mode and storage.
bool edge_infer_fused(int N, int E, int C, int Ce, int H, int Hd);
int edge_logits_launch(const EdgeZParams& p, hipStream_t stream);    // Z == null; makes the whole W2 image in Wq
int edge_msg_wsum_launch(const EdgeZParams& p, hipStream_t stream);  // Wq: that image; Pi / Pj: [N, W2]; store Z_BF16: z rounded
// ---- the same per-edge phase for edge_attr = table[idx] of R rows (shell-indexed edge features), edgeidx.hip ----
// Te [R, W2] = table W_e^T (no bias); idx [E] int64 in original edge order, reached through perm; Pi / Pj [N, W2].
// Gathers and fp32 VALU only: any arithmetic mode, any E.  edge_idx_ok: the host-only predicate of the shapes.
#define EDGE_IDX_MAX_ROWS 256
bool edge_idx_ok(int H, int Hd, int R);
int edge_idx_logits_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                           const int* srci, int W2, const float* wA, const float* bA, int H, int Hd, const int* rowptr,
                           int N, int E, float* a_out, hipStream_t stream);
int edge_idx_wsum_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                         const int* srci, int W2, const float* alpha, int H, int Hd, const int* rowptr, int N, int E,
                         float* S, hipStream_t stream);
// ---- the training form of that route, edgeidx.hip: no Z is stored, the backward forms z again from the three rows ----
// edge_idx_train_ok: edge_idx_ok plus whole 32-column mask words per half (H * Hd % 32 == 0).  Host only.
bool edge_idx_train_ok(int H, int Hd, int R);
int edge_idx_bwd_chunks(int N);                 // rows of partialW [chunks][H * Hd]
// the segment backward (segbwd.hip's three steps on recomputed z): tt, ga [E, H]; mask [E][W2 / 32] in EdgeRC's layout;
// Gi [N, W2]; partialW: the partial rows of grad fc_out_A.weight = sum ga leaky(z_A)
int edge_idx_bwd_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                        const int* srci, int W2, const float* alpha, const float* gS, const float* gs, const float* wA,
                        int H, int Hd, const int* rowptr, int N, int E, float* tt, float* ga, unsigned* mask, float* Gi,
                        float* partialW, hipStream_t stream);
int seg_bwd_soft_launch(const float* alpha, const float* tt, const int* rowptr, int N, int H, float* ga,
                        hipStream_t stream);    // segbwd.hip: seg_bwd_soft_kernel alone
// the class sum gT [R, W2] of the rebuilt gZ rows: slots grouped by class in ascending slot order (cls_pos [E]), classes
// cut into fixed pieces (piece_start [R + 1], piece_rowptr [edge_idx_class_pieces(E, R) + 1]) -- all three made by
// edge_idx_class_plan_launch from index and the plan's slot order, once per batch;
// partials: [edge_idx_class_pieces(E, R)][W2] floats of workspace
struct EdgeRC;
int edge_idx_class_pieces(int E, int R);
size_t edge_idx_class_plan_ws_bytes(int E, int R);
int edge_idx_class_plan_launch(const int64_t* idx, const int* perm, int E, int R, int* cls_pos, int* piece_start,
                               int* piece_rowptr, void* ws, size_t ws_bytes, hipStream_t stream);
int edge_idx_class_sum_launch(const EdgeRC& rc, const int* piece_rowptr, const int* piece_start, const int* cls_pos, int R,
                              int E, int W2, float* partials, float* gT, hipStream_t stream);
// ... over a STORED gZ [E, W2] (row-major, destination-sorted slots): level 1 sums each piece's rows, gathered through
// cls_pos, in ascending order in fp64 and rounds once; level 2 is the same fp64 reduction in piece order.  Same tag.
int edge_idx_class_sum_launch(const float* gZ, const int* piece_rowptr, const int* piece_start, const int* cls_pos, int R,
                              int E, int W2, float* partials, float* gT, hipStream_t stream);
// ---- the vector-attention first layer on the lookup: hidden[t, :] = leaky(Te[idx[perm[t]]] + Pi[dst[t]] + Pj[src[t]]) over
// all W2 columns, z through the same idx_z; hmax (optional, zeroed by a fill kernel before): max |hidden| by one integer
// atomic max per workgroup (order-free).  Flat over the E * W2 / 4 column quads: any W2 % 4 == 0, any degree.  Tag
// "edge_idx_hidden".  edge_idx_hidden_ok: the host-only predicate of the shapes.
bool edge_idx_hidden_ok(int W2, int R);
int edge_idx_hidden_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                           const int* srci, const int* dsti, int W2, int E, float* hidden, float* hmax, hipStream_t stream);
// debug: mask[perm[t]][c] = (z[t][c] > 0) for z formed as the route forms it (uint8 [E, W2], original edge order)
int edge_idx_signs_launch(const float* Te, int R, const int64_t* idx, const int* perm, const float* Pi, const float* Pj,
                          const int* srci, const int* dsti, int W2, long E, uint8_t* mask, hipStream_t stream);
size_t linear128_heads_image_floats(int n_out);
// batched form for 128 x 128 dense-layer weights W(o, k) = src[o * so + k * sk]: image i at dst + i * WPREP_IMAGE_FLOATS
#define WPREP_MAX 48
#define WPREP_IMAGE_FLOATS (16384 + 4)
#define WPREP_IMAGE_FLOATS_X6 24576             // the six-pass bf16 chain's image: three 2-byte planes (chain.hip)
#define WPREP_IMAGE_FLOATS_MAX 24576
size_t wprep_image_floats();                    // ... of the current arithmetic mode (0: it has no fused chain)
struct WPrepBatch {
  const float* src[WPREP_MAX];
  long sb[WPREP_MAX], sc[WPREP_MAX];   // strides of the k index and of the output index
  int n;
};
int prepare_W_f16_batch_launch(const WPrepBatch& b, float* dst, hipStream_t stream);
// three-bf16-plane images (the dense-layer kernel's operand in the 24-bit modes) of b.n 128 x 128 weights, 24576 floats each
int prepare_T_bf16_batch_launch(const WPrepBatch& b, float* dst, hipStream_t stream);
int prepare_T_bf16_rows_launch(const float* rows, long ld, const int* gather, int nrows, void* dst, int NA,
                               hipStream_t stream, const float* emax = nullptr);   // emax: fp16 form scaled by max |rows|
// dense layer at width 128 on the split-bf16 kernel: out = act(in W^T + bias) (+ out),  W(o, k) = W[o*so + k*sk]
bool linear128_fast(int K, int N, long ldi, long ldo, const void* in, const void* out);
size_t linear128_ws_bytes(int n_out = 128);
struct Linear128Params {
  const float* in;       // [rows, 128], row stride ldi
  long ldi;
  const float* W;        // element (o, k) at W[o * so + k * sk]
  long so, sk;
  const float* bias;     // [n_out] or null
  int act;               // CGAT_ACT_*
  int accumulate;        // out += result
  float* out;            // [rows, n_out], row stride ldo
  long ldo;
  int rows, n_out;
  const void* prepared;  // the mode's image of W made ahead (prepare_W_f16_batch_launch / prepare_T_bf16_batch_launch), n_out == 128
  const float* dact;     // out *= LeakyReLU'(sign of dact[row, col]), row stride ld_dact; null: none
  long ld_dact;
  float* omax;           // max |out| folded into omax[0] (not zeroed here)
  // linear128_heads_launch: `heads` independent (in, W, bias, out, dact) in one launch pair, head h at + h * s_*
  // (elements).  heads == 1 with zero strides: the single-operand launch
  int heads;
  long s_in, s_w, s_bias, s_out, s_dact;
};
static inline Linear128Params linear128_params(const float* in, long ldi, const float* W, long so, long sk, float* out,
                                               long ldo, int rows, int n_out = 128) {
  Linear128Params p = {};
  p.in = in; p.ldi = ldi; p.W = W; p.so = so; p.sk = sk; p.out = out; p.ldo = ldo; p.rows = rows; p.n_out = n_out;
  p.heads = 1;
  return p;
}
int linear128_launch(const Linear128Params& p, void* ws, hipStream_t stream);
// ws: heads * linear128_heads_image_floats(n_out) floats; the f16x3 and 24-bit modes
int linear128_heads_launch(const Linear128Params& p, void* ws, hipStream_t stream);
// ---- a chain of width-128 dense layers in one launch (f16x3 mode), chain.hip ----
#define CHAIN_MAX 5
struct ChainLayer {
  const uint4* W;        // prepared image (prepare_W_f16_batch_launch: 8 chunks of 8 KB, its scale behind them)
  const float* bias;     // [128] or null
  const float* dact;     // null, or saved activation values y [rows,128]: the layer's result is multiplied by act'(y)
  const float* resid;    // null, or [rows,128] added to the (activated) result
  float* out;            // null, or where the result goes
  long ld_dact, ld_resid, ld_out;
  int act;               // activation of the layer (CGAT_ACT_*)
  int dact_type;         // activation whose derivative `dact` stands for
  int accumulate;        // out += result
};
struct ChainDesc {
  ChainLayer layer[CHAIN_MAX];
  int n_layers, rows;
  const float* x;        // input rows [rows,128]
  long ldx;
  const float* in_dact;  // null, or the input rows are multiplied by act'(in_dact) first (backward of an activation)
  long ld_in_dact;
  int in_dact_type;
  float* in_store;       // null, or where the (multiplied) input rows are stored
  long ld_in_store;
};
int prepare_W_batch_launch(const WPrepBatch& b, float* dst, hipStream_t stream);   // the current mode's chain images
bool mlp_chain128_fast(const ChainDesc& d);
int mlp_chain128_launch(const ChainDesc& d, hipStream_t stream);
#define CHAIN_BATCH_MAX 4
// n independent chains over the same rows in one launch (24-bit modes; otherwise one launch each)
int mlp_chain128_batch_launch(const ChainDesc* d, int n, hipStream_t stream);
// ---- segment backward of the scalar-attention layer, segbwd.hip ----
// partialW: [edge_seg_bwd_chunks(N)][H * Hd].  The caller has decided the route: vec (16-byte aligned, Hd % 4 == 0), zb_6 /
// zb (Z stored as bf16 by the six-pass per-edge kernel / at all), rc_shape (sign bits in `mask` instead of gZ),
// have_scales (f16x3 maxima: gzmax[0..7] zeroed here first) -- one launch, or three small kernels at Hd == 256 with sign bits.
int edge_seg_bwd_chunks(int N);
int edge_seg_bwd_launch(const float* Z, float* gZ, long gz_block, const float* alpha, const float* gS, const float* gs,
                        const int* rowptr, const float* wA_out, int N, int H, int Hd, float* tt, float* ga, float* Gi,
                        float* partialW, float* gzmax, unsigned* mask, float* gimax, bool vec, bool zb_6, bool zb,
                        bool rc_shape, bool have_scales, hipStream_t stream,
                        const int* bits_src = nullptr);   // the bit form of the saved buffer (segbwd.hip seg_bwd_attb_kernel):
                                                          // the source node of every slot; Z holds no attention values
// debug: mask[perm[t]][c] = (Z[t][c] > 0), the saved pre-activations' signs in original edge order
// (zbits: the attention half from the stored sign words of the bit form)
int attn_signs_launch(const float* Z, const int* perm, long E, int W2, uint8_t* mask, hipStream_t stream,
                      const unsigned* zbits = nullptr);
// ---- split-bf16 backward products over gZ, edgebwd.hip ----
// The pre-activation gradient of the scalar-attention layer is never stored when its consumers can rebuild it
// (edge_seg_bwd_kernel step 3, segbwd.hip): for destination-sorted slot t and column col of the stacked hidden layer
//     gZ[t, col] = (ga[t,h]    * wA[col])                 * d      col <  HHd  (attention network, h = col / Hd)
//                = (alpha[t,h] * gS[dst[t], col - HHd])   * d      col >= HHd  (message network,  h = (col-HHd) / Hd)
// with d = 1 if Z[t,col] > 0 else 0.01 (LeakyReLU').  Per edge that is 2 H scalars, one bit per column and a row of a
// per-NODE matrix shared by all edges of the destination: 216 bytes + cache hits instead of 6 KB of HBM per read.
struct EdgeRC {
  const unsigned* mask;   // [E][W2 / 32]: bit (col & 31) of word (col >> 5) = (Z[t, col] > 0)
  const float* ga;        // [E][H]
  const float* alpha;     // [E][H]
  const float* gS;        // [N][HHd]
  const float* wA;        // [HHd]
  const int* dst;         // [E] destination node of slot t
  int H, Hd, HHd, nw;     // nw = W2 / 32
  const float* cs;        // [H][128], set by the launchers of edge_ge_kernel's bit-plane form (prepare_T_bf16_attn_launch)
};
// edge storage mode 3 ("bf16-mma", layers.hip): the per-edge products over the rebuilt gZ rows run ONE bf16 pass
bool edge_mma_bf16();
// shapes the rebuilding kernels take: whole 128-column blocks inside one head, 256-column groups in the mask writer
static inline bool edge_rc_shape(int Ce, int H, int Hd) { return Ce == 128 && H > 0 && Hd > 0 && Hd % 128 == 0; }
// operand element (t, 128 a + j) at gZ[t * ldg + a * gzb + j]: (128, E*128) = column-blocked, (W2, 128) = row-major;
// with rc != null the operand is rebuilt from *rc instead (gZ, ldg, gzb unused)
// The edge part of grad fc_out_A under the bit form of the saved buffer: the reducer of the
// bit-plane form adds sum_k We[col, k] u[col, k] (We: the edge_attr slice of the stacked weight, leading dimension ldw)
// to out[col] -- through part, 4 H Hd doubles of scratch, in a fixed order
struct GwTe {
  const float* We;
  long ldw;
  double* part;
  float* out;
};
// Operands of the K = W2 -> 128 product (edge_ge_kernel): out[scatter[t], :] (+)= rows[t, :] @ W + bias.  One record for the
// plain launch, the K-split launch (slabs != null), the launch on a prepared image (We == null) and the heads launch
// (heads > 0); edge_ge_launch tells them apart by those fields.
struct EdgeGeParams {
  const float* gZ;       // the rows operand, element (t, 128 a + j) at gZ[t * ldg + a * gzb + j] (see above); unused with rc
  long ldg, gzb;
  const EdgeRC* rc;      // non-null: the rows are rebuilt from *rc (the per-edge launch of the scalar-attention backward)
  const float* We;       // weight, element (col, k) at We[col * s_col + k * s_out] (col < W2 inputs, k < 128 outputs);
  long s_col, s_out;     //   null: Wq already holds the six-pass image (prepare_T_planes_launch, alternate = 1) and is only read
  float* Wq;             // the weight image: edge_z_wq_floats(W2) floats; heads: heads * edge_ge_heads_image_floats(W2) +
                         //   bilinear_prepare_T_batch_ws_floats(heads)
  int W2;                // input columns (K)
  int rows;
  float* out;            // [rows, 128], row stride ldo; row t goes to scatter[t] (null: t)
  long ldo;
  const int* scatter;
  int accumulate;        // out += result
  const float* bias;     // [128] or null: added to the product, before any accumulation into `out`
  const float* amax;     // f16x3 mode only: device max |rows| -> the fp16 form; without it the six-pass form runs
  // the K-split launch: group s of S multiplies its column blocks into slab s ([rows, 128] each at slabs + s * rows * 128,
  // scattered rows as `out` would be); the caller adds the slabs in group order.  out / accumulate / bias / amax unused.
  float* slabs;
  int S;                 // edge_ge_ksplit_groups(rows, W2, rc != null)
  // the heads launch: `heads` products y_h = x_h W_h^T + b_h in one launch pair, head h's operands at + h * s_* (elements);
  // W_h [128, W2] row-major and contiguous (s_col == 1, s_out == W2)
  int heads;
  long s_x, s_w, s_bias, s_y;
};
// the plain launch on row-major or column-blocked rows (everything else: set the field)
static inline EdgeGeParams edge_ge_params(const float* gZ, long ldg, long gzb, const float* We, long s_col, long s_out,
                                          float* Wq, int W2, float* out, long ldo, int rows) {
  EdgeGeParams p = {};
  p.gZ = gZ; p.ldg = ldg; p.gzb = gzb; p.We = We; p.s_col = s_col; p.s_out = s_out; p.Wq = Wq; p.W2 = W2;
  p.out = out; p.ldo = ldo; p.rows = rows;
  return p;
}
// Which edge_ge_kernel a launch runs, on which image and grid: decided once per launch by edge_ge_form (host only;
// DESIGN.md lists the forms) and read by the launcher, edge_ge_ksplit_groups' callers and the debug query.
enum EdgeGePrep : int {
  GE_PREP_NONE = 0,      // the caller's image
  GE_PREP_PLANES = 1,    // three bf16 planes, odd blocks negated (all heads' in one launch)
  GE_PREP_F16_TMAX = 2,  // two fp16 planes scaled by the weight's maximum, which is formed first
  GE_PREP_ATTN = 3,      // three planes with the attention blocks scaled by wA, and their column sums (the bit-plane body)
  GE_PREP_HEADS_F16 = 4  // the heads' maxima and fp16 planes by the contractions' batched preparation (opimage.hip)
};
struct EdgeGeForm {
  int passes;            // edge_ge_kernel<PASSES, ., .>: 1 (one bf16 plane), 2 (two fp16 planes), 3 or 6 (three bf16 planes); 0: no rows
  bool rc;               // <., RC, .>: rebuilt rows
  bool bitplane;         // <6, true, BP>: the attention half on the stored bit
  EdgeGePrep prep;
  int grid_x;            // row tiles of 256
  int groups, ncb_g;     // K groups over grid.y (1: none) and the column blocks of each
  int heads;             // heads over grid.y (0: not the heads launch)
};
EdgeGeForm edge_ge_form(const EdgeGeParams& p);
// the kernel's dims, leading dimensions and mode: 128 outputs, whole 128-column blocks, float4 rows (callers add aligned16)
bool edge_ge_dims(int Ce, int W2, long ldg, long gzb, long ldo);
// ... of the heads launch: x_h / y_h as edge_ge_dims, weights [128, W2] with ldw == W2, a mode that batches its heads
bool edge_ge_heads_dims(int heads, int W2, long ldx, long ldy, long ldw, bool have_amax);
size_t edge_ge_heads_image_floats(int W2);
// K-split form for few row tiles beside a long K: the groups a launch of this shape takes (1: the plain launch).  rebuilt:
// the rows come from an EdgeRC
int edge_ge_ksplit_groups(int rows, int W2, bool rebuilt);
int edge_ge_launch(const EdgeGeParams& p, hipStream_t stream);

// Operands of the K = E -> W2 x 128 product (edge_gw_kernel): out[col, :] = sum_t rows[t, col] * e[perm[t], :]
struct EdgeGwParams {
  const float* gZ;       // the rows operand as EdgeGeParams'; unused with rc
  long ldg, gzb;
  const EdgeRC* rc;      // non-null: the rows are rebuilt from *rc
  const float* e;        // [., 128], row stride lde; slot t reads e[perm[t]] (null: e[t])
  long lde;
  const int* perm;
  int E;                 // rows of gZ (the reduction index)
  int W2;                // columns of gZ = rows of out
  float* ws;             // edge_gw_ws_floats(E, W2) floats
  float* out;            // [W2, 128], row stride ldo
  long ldo;
  const float* gmax;     // f16x3 mode only: device max |gZ| and max |e| -> the fp16 form; without them the six-pass form
  const float* emax;
  bool force_six;        // debug: this launch keeps the six-pass form on every column
  const GwTe* te;        // non-null: the bit-plane form's reducer also adds the edge part of grad fc_out_A (above)
};
static inline EdgeGwParams edge_gw_params(const float* gZ, long ldg, long gzb, const float* e, long lde, const int* perm,
                                          int E, int W2, float* ws, float* out, long ldo) {
  EdgeGwParams p = {};
  p.gZ = gZ; p.ldg = ldg; p.gzb = gzb; p.e = e; p.lde = lde; p.perm = perm; p.E = E; p.W2 = W2; p.ws = ws;
  p.out = out; p.ldo = ldo;
  return p;
}
// Which edge_gw_kernel a launch runs and how it carves its workspace: decided once per launch by edge_gw_form (host only)
struct EdgeGwForm {
  int passes;            // edge_gw_kernel<PASSES, ., .> of the plain form: 1, 2, 3 or 6; 0: no rows (out is zero-filled)
  bool rc;               // <., RC, .>
  bool bit_shape;        // mode and shape admit the bit-plane form -- what no debug switch changes (the bit form of the layer's
                         // saved buffer rests on this alone)
  bool bitplane;         // edge_gw_kernel<6, true, true> and its reducer write `out`; the plain form does not run
  bool te_only;          // ... run for te alone (the debug switches keep the six-pass form), then the plain form writes `out`
  int S, grid_x;         // the plain form: k-ranges, and workgroups = S * column-block pairs
  int SA, SM, npm;       // the bit-plane form: k-ranges per attention pair / per message pair, message pairs
  int bit_grid_x;        //   its workgroups: SM * npm + SA * H <= 256
  size_t slab;           // floats from ws: the slabs (either form), behind the planes of e
  size_t slabA, csl;     //   the bit-plane form's attention slabs and column sums
  size_t ws_end;         //   the end of what the launch touches
};
EdgeGwForm edge_gw_form(const EdgeGwParams& p);
// mode and shape of the bit-plane form for a scalar-attention layer of H heads of Hd (edge_gw_form's bit_shape)
bool edge_gw_bitplane_layer(int H, int Hd);
// the kernel's dims, leading dimensions and mode: 128 outputs, whole column-block pairs (callers add aligned16)
bool edge_gw_dims(int Ce, int W2, long ldg, long gzb);
size_t edge_gw_ws_floats(int E, int W2);
bool edge_gw_force_six(bool on);   // debug: the process-wide switch; returns the previous setting
int edge_gw_launch(const EdgeGwParams& p, hipStream_t stream);
// Gj[n, :] = sum over the edges leaving n of the rebuilt gZ rows (src_rowptr / src_pos: slots grouped by source)
int edge_gj_launch(const EdgeRC& rc, const int* src_rowptr, const int* src_pos, int N, int W2, float* Gj, long ldo,
                   hipStream_t stream, float* gjmax = nullptr);   // gjmax: max |Gj| folded in (zeroed by the caller)

// ---- width-128 weight gradients over rows, rowsdw.hip: out_k[o][i] = sum_n G[n,o] X_k[n,i], bsum[o] = sum_n G[n,o] ----
bool rows_dw128_fast(const float* G, long ldg, const float* X1, long ldx1, const float* X2, long ldx2);
size_t rows_dw128_ws_bytes(int rows, int nx);
int rows_dw128_launch(const float* G, long ldg, const float* X1, long ldx1, float* out1, long ldo1, const float* X2,
                      long ldx2, float* out2, long ldo2, float* bsum, int rows, void* ws, size_t ws_bytes,
                      hipStream_t stream);
// many such products in one launch (every item: one right operand; common row count and leading dimensions)
#define DW_BATCH_MAX 32
struct DwBatchItem {
  const float* G;    // [rows, 128], row stride ldg
  const float* X;    // [rows, 128], row stride ldx
  float* out;        // [128][ldo]: G^T X
  float* bsum;       // [128] column sums of G, or null
};
struct DwBatchDesc {
  int n, rows, splits, rows_per_unit;   // splits / rows_per_unit are set by the launch
  long ldg, ldx, ldo;
  DwBatchItem it[DW_BATCH_MAX];
};
size_t rows_dw128_batch_ws_bytes(int n_items, int rows);
bool rows_dw128_batch_fast(const DwBatchDesc& d);
int rows_dw128_batch_launch(DwBatchDesc d, void* ws, size_t ws_bytes, hipStream_t stream);

// ---- elementwise / row kernels, rowops.hip ----
int layernorm_tanh_fwd_launch(const float* u, float* y, int rows, int W, float eps, hipStream_t s);
int layernorm_tanh_bwd_launch(const float* u, const float* y, const float* gy, float* gu, int rows, int W, float eps,
                              hipStream_t s);
int act_bwd_launch(const float* y, const float* gy, float* gpre, long n, int act, hipStream_t s);  // in terms of post-activation y
bool act_bwd_leaky_max_fast(const void* y, const void* gy, const void* gpre, long n);   // the vector form applies
int act_bwd_leaky_max_launch(const float* y, const float* gy, float* gpre, long n, float* gmax, hipStream_t s);
int colsum_launch(const float* x, long ldx, int rows, int cols, float* out, float alpha, void* ws, size_t ws_bytes,
                  hipStream_t s);
size_t colsum_ws_bytes(int rows, int cols);
int mix_launch(const float* a, const float* b, const float* d, float* out, long n, hipStream_t s);  // out = d*a + (1-d)*b
int mix_bwd_launch(const float* g, const float* a, const float* b, const float* d, float* ga, float* gb_accum,
                   float* gd, long n, void* ws, size_t ws_bytes, hipStream_t s);
int scale_launch(const float* x, float alpha, float* out, long n, hipStream_t s);   // out = alpha * x
int axpy_launch(float* y, const float* x, float alpha, long n, hipStream_t s);  // y += alpha*x
int sum_slabs_launch(const float* slabs, int n, long stride, float* out, long count, hipStream_t s);   // out = 0.f + slab 0 + slab 1 + ...
// the same for `items` slab sets item_stride apart, item t into out[t] (rows of 128 at row stride ldo)
#define SLAB_SUM_MAX 8
struct SlabSumOut { float* out[SLAB_SUM_MAX]; };
int sum_slabs_batch_launch(const float* slabs, int n, long stride, long count, int items, long item_stride,
                           float* const* out, long ldo, hipStream_t s);
int copy2d_launch(const float* src, long lds, float* dst, long ldd, int rows, int cols, hipStream_t s);
struct Copy2DJob { const float* src; long lds; float* dst; long ldd; int rows, cols; };
struct Copy2DJobs { Copy2DJob job[4]; int n; };
int copy2d_multi_launch(const Copy2DJobs& j, hipStream_t s);   // n <= 4 copies in one launch
int fill_launch(float* p, float v, long n, hipStream_t s);

// ---- segment kernels (rows sorted by segment, rowptr[S+1]), segment.hip ----
#define SEG_LONG 256   // segments of more rows go to the *_long kernels (segment.hip) -- and keep their order in edgez.hip
int seg_softmax_fwd_launch(const float* a, const float* mult, const int* rowptr, int S, int F, float eps, float* alpha,
                           float* ssum, hipStream_t s);
int seg_softmax_bwd_launch(const float* alpha, const float* galpha, const float* gssum, const float* mult,
                           const int* rowptr, int S, int F, float* ga, float* gmult, hipStream_t s);
// out[s, f] = sum_{r in seg s} w[r, f / fw] * act(x[r or ridx[r], f])      (w nullable, fw = features per weight)
int seg_wsum_launch(const float* x, long ldx, const int* ridx, const float* w, int wF, int fw, const int* rowptr, int S,
                    int F, int act, float* out, long ldo, hipStream_t s, long xblock = 0, int x_bf16 = 0);   // x_bf16: x holds bf16 (ldx, xblock in elements)
// softmax-weighted segment sum (attention pooling) in one pass per direction, see segment.hip
bool seg_attnpool_fast(int aF, int F, long ldm, const void* a, const void* m, const void* out);
int seg_attnpool_fwd_launch(const float* a, int aF, const float* mult, const float* m, long ldm, const int* rowptr,
                            const int* ridx, int S, int F, float eps, float* out, float* mx, float* inv, hipStream_t s,
                            float* out_lo = nullptr);     // out_lo: low part of the fp64 sum, for backward (may be null)
int seg_attnpool_bwd_launch(const float* a, int aF, const float* mult, const float* m, long ldm, const int* rowptr,
                            const int* ridx, int S, int F, const float* out, const float* mx, const float* inv, const float* g_out, float* g_a,
                            float* g_m, long ldgm, float* g_mult, hipStream_t s, const float* out_lo = nullptr);
// the same with an attention-dropout keep-mask: m' = keep * m, keep [R, aF] scaled by 1 / (1 - p); the keep row of CSR
// position t is keep_idx[t] (nullable: the operand row).  `mult` must be null: the combination is refused, not built.
int seg_attnpool_drop_fwd_launch(const float* a, int aF, const float* mult, const float* keep, const int* keep_idx,
                                 const float* m, long ldm, const int* rowptr, const int* ridx, int S, int F, float eps,
                                 float* out, float* mx, float* inv, float* out_lo, hipStream_t s);
int seg_attnpool_drop_bwd_launch(const float* a, int aF, const float* mult, const float* keep, const int* keep_idx,
                                 const float* m, long ldm, const int* rowptr, const int* ridx, int S, int F,
                                 const float* out, const float* mx, const float* inv, const float* out_lo,
                                 const float* g_out, float* g_a, float* g_m, long ldgm, hipStream_t s);
// per-row, per-head dot:  out[r,h] = sum_j act(x[r, h*Hd+j]) * v[(vrow(r)) * ldv + h*Hd + j] + bias[h] (+ addv[vrow(r)*H + h])
int rowdot_launch(const float* x, long ldx, int act, const float* v, long ldv, const int* vrow, const float* bias,
                  const float* addv, int rows, int H, int Hd, float* out, hipStream_t s);

// ---- head combination of the per-edge hypernetwork edge update, edgecomb.hip ----
// out[perm ? perm[t] : t, c] = (sum_h softmax_h(sa[t, ., c'])[h] * keep[t,h,c'] * sm[t,h,c]) / H with c' = c (aF == Co)
// or 0 (aF == 1); the softmax over the heads has no max-subtraction (CGAT.py:214-223).  keep / perm may be null; backward
// recomputes the softmax from sa, g_sa / g_sm may be null.  No workspace, no atomics.
bool edge_combine_ok(int H, int aF, int Co);   // Co % 4 == 0, Co <= 256, 1 <= H <= 8, aF in {1, Co}
int edge_combine_fwd_launch(const float* sa, int aF, const float* sm, const float* keep, const int* perm, long E, int H,
                            int Co, float* out, hipStream_t s);
int edge_combine_bwd_launch(const float* sa, int aF, const float* sm, const float* keep, const int* perm,
                            const float* g_out, long E, int H, int Co, float* g_sa, float* g_sm, hipStream_t s);

// ---- CSR plan, plan.hip ----
size_t plan_ws_bytes(int E, int N);
int plan_build_launch(const int64_t* edge_index, int E, int N, int* dst_rowptr, int* dst_perm, int* dst_sorted,
                      int* src_sorted, int* src_rowptr, int* src_pos, void* ws, size_t ws_bytes, hipStream_t s);
int csr_from_keys_launch(const int* keys, int n, int S, int* rowptr, int* perm, void* ws, size_t ws_bytes, hipStream_t s);
