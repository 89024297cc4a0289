/* libcgat_hip -- C ABI of the MI355X (gfx950) edge-attention hot path of hyllios/CGAT.
 *
 * Every pointer is a DEVICE pointer to contiguous fp32 / int32 / int64 data unless stated
 * otherwise; `stream` is a hipStream_t passed as void*.  Functions return 0 on success; on
 * failure cgat_last_error() describes the problem.  No function allocates device memory or
 * synchronises the host: outputs, saved-for-backward buffers and workspaces are provided by
 * the caller (size queries below), so every call is hipGraph-capturable.
 *
 * The reference (pure Python) has no FFI; each entry point names the reference operator it
 * replaces (paths relative to the reference repository root).
 */
#ifndef CGAT_HIP_H
#define CGAT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CGAT_ABI_VERSION 3   /* 2: cgat_linear_forward / cgat_edge_hidden_forward / _backward carry tensor maxima (round 3)
                              * 3: cgat_segment_attention_pool_* carry out_lo; arithmetic mode 4 = "f16x3c" (round 4) */
#define CGAT_MAX_FC 8      /* Linear+Tanh layers per hypernetwork trunk */
#define CGAT_MAX_HYPER 8   /* predicted layers per hypernetwork */

int cgat_abi_version(void);
const char* cgat_last_error(void);

/* ---- launch timing (HIP events on the launch stream) --------------------------------- */
void cgat_prof_enable(int on);
void cgat_prof_reset(void);
/* sums all recorded launches of kernels tagged `tag` ("bilinear_rows", "bilinear_wgrad",
 * "gemm_f32", ...); synchronises the recorded events. */
int cgat_prof_get(const char* tag, int* count, float* total_ms);
/* kernel launches issued by the library since the process started (every launch is counted, on any stream) */
uint64_t cgat_prof_launches(void);

/* ---- CSR plan: PyG propagate's implicit segment structure, built once per batch --------
 * replaces the index handling of torch_geometric MessagePassing.propagate / utils.softmax /
 * torch_scatter.scatter_add as used at CGAT/CGAT.py:313-326 (aggregation keyed by
 * edge_index[1]).  dst_perm: edge ids sorted (stably) by edge_index[1]; dst_rowptr[N+1];
 * dst_sorted/src_sorted: endpoints in that order; (src_rowptr, src_pos): sorted positions
 * grouped by edge_index[0]. */
typedef struct cgat_plan {
  int32_t N, E;
  const int32_t* dst_rowptr;
  const int32_t* dst_perm;
  const int32_t* dst_sorted;
  const int32_t* src_sorted;
  const int32_t* src_rowptr;
  const int32_t* src_pos;
} cgat_plan;
size_t cgat_plan_workspace_bytes(int32_t E, int32_t N);
int cgat_plan_build(const int64_t* edge_index /* [2,E] */, int32_t E, int32_t N, int32_t* dst_rowptr /* [N+1] */,
                    int32_t* dst_perm /* [E] */, int32_t* dst_sorted /* [E] */, int32_t* src_sorted /* [E] */,
                    int32_t* src_rowptr /* [N+1] */, int32_t* src_pos /* [E] */, void* ws, size_t ws_bytes,
                    void* stream);
/* generic CSR from int32 keys in [0,S): rowptr[S+1], perm[n] (ids ascending inside a segment) */
size_t cgat_csr_workspace_bytes(int32_t S);
int cgat_csr_from_keys(const int32_t* keys, int32_t n, int32_t S, int32_t* rowptr, int32_t* perm, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- batch collation on the device (the step before the hot path) -----------
 * replaces, per training step, CGAT/data.py:61-144 (CompositionData.__getitem__ for every crystal of the batch),
 * PyG Batch.from_data_list (CGAT/lightning_module.py:200) and CGAT/roost_message.py:400-458 (collate_batch).
 * The dataset lives on the device in packed int32 form (built once): per-atom element ids into the embedding table,
 * the neighbour tables already sliced to max_nbr columns, the per-crystal composition (unique elements in
 * first-appearance order and their weights) and y = target * n_atoms (or the plain target for 'volume'). */
typedef struct cgat_packed_dataset {
  int32_t n_graphs, fea, max_nbr, n_elem;
  const float* table;        /* [n_elem, fea] element embedding */
  const int32_t* atom_ptr;   /* [n_graphs+1] */
  const int32_t* atom_elem;  /* [atoms] row of `table` */
  const int32_t* shell;      /* [atoms, max_nbr] edge_attr ids */
  const int32_t* self_idx;   /* [atoms, max_nbr] crystal-local centre atom */
  const int32_t* nbr_idx;    /* [atoms, max_nbr] crystal-local neighbour atom */
  const int32_t* comp_ptr;   /* [n_graphs+1] */
  const int32_t* comp_elem;  /* [unique elements] row of `table` */
  const float* comp_weight;  /* [unique elements] count / n_atoms */
  const float* y_val;        /* [n_graphs] */
} cgat_packed_dataset;
typedef struct cgat_collated {   /* outputs, caller-allocated; dtypes as the reference's tensors */
  float* x;                  /* [N, fea] */
  int64_t* edge_index;       /* [2, E], E = N * max_nbr */
  int64_t* edge_attr;        /* [E] */
  float* y;                  /* [B] */
  int64_t* batch;            /* [N] */
  float* comp_weight;        /* [Nc] (the reference views it as [Nc,1]) */
  float* comp_fea;           /* [Nc, fea] */
  int64_t* comp_self;        /* [Ec] */
  int64_t* comp_nbr;         /* [Ec] */
  int64_t* comp_crystal;     /* [Nc] */
} cgat_collated;
/* ids[B]: crystals of the batch in order; node_off/comp_off/cedge_off[B]: exclusive prefix sums of their atom
 * counts, unique-element counts and u*(u-1) composition edges (all device pointers). */
int cgat_collate_batch(const cgat_packed_dataset* ds, const int32_t* ids, const int32_t* node_off,
                       const int32_t* comp_off, const int32_t* cedge_off, int32_t B, int64_t E_total, int64_t Ec_total,
                       const cgat_collated* out, void* stream);

/* ---- neighbour tables from lattice + fractional coordinates (the stage before packing) -----------
 * replaces CGAT/prepare_data.py:146-169 (pymatgen's get_all_neighbors(radius), a Python sort and a Python loop per
 * atom): the tables a cgat_packed_dataset is packed from.  All geometry in fp64.  For every crystal g (atoms
 * atom_ptr[g] .. atom_ptr[g+1], lattice rows a, b, c in lattice[g]): f_j = frac_j - floor(frac_j), r_j = f_j . L; the
 * candidates of atom i are all (j, R in Z^3) with 1e-8 < d = |r_j + R.L - r_i| <= radius; sorted by d, shell ids by the
 * reference's chain rule (a candidate opens the next shell iff d exceeds the FIRST distance of the current shell by more
 * than 1e-8); the row keeps the first K, the shell holding the K-th place taken in ascending j, and is ordered by
 * (shell, j).  status[g]: 0 built; 1 some atom has fewer than K candidates within radius (the reference drops the
 * crystal); 2 beyond the kernel's limits (more than 1024 atoms in the crystal, a lattice without volume, more than 2^26
 * (image, j) pairs in one search, or a shell holding the K-th place that does not fit the 2048-entry candidate list).
 * Rows of crystals with status != 0 are zero-filled; no wrong row is ever written.  Outputs: shell (1..K), self_idx
 * (crystal-local i), nbr_idx (crystal-local j), all int32 [N, K]; dist fp64 [N, K] or NULL; passes int32 [N] or NULL
 * (searches the atom needed: 1 = the first working radius was accepted).  1 <= K <= 64, N * K < 2^31, atom_ptr
 * non-decreasing from 0 to N.  All pointers are device pointers; bitwise deterministic; caller's stream, no allocation,
 * no synchronisation. */
int cgat_neighbor_tables(const double* lattice /* [G,3,3] */, const double* frac /* [N,3] */,
                         const int32_t* atom_ptr /* [G+1] */, int32_t G, int32_t N, int32_t K, double radius, int32_t* shell,
                         int32_t* self_idx, int32_t* nbr_idx, double* dist, int32_t* status /* [G] */, int32_t* passes,
                         void* stream);
/* The same with the candidate capacity (K .. 2048) and the first working radius (0 = from the number density) given by
 * the caller: the tests drive the shrink / grow / does-not-fit paths with it. */
int cgat_debug_neighbor_tables(const double* lattice, const double* frac, const int32_t* atom_ptr, int32_t G, int32_t N,
                               int32_t K, double radius, int32_t cap, double first_radius, int32_t* shell,
                               int32_t* self_idx, int32_t* nbr_idx, double* dist, int32_t* status, int32_t* passes,
                               void* stream);

/* ---- packing a dataset on the device (between the neighbour tables and the first batch) -----------
 * replaces the per-crystal host loop of cgat_amd/collate.py:72-95 (PackedDataset.from_dict) and, in the reference,
 * CGAT/data.py:61-103 and 140-141 (CompositionData.__getitem__: element rows, composition, tables sliced to
 * max_neighbor_number, y = target * n_atoms) with the slicing into per-crystal arrays before it
 * (cgat_amd/neighbors.py dataset_dict_from_structures; CGAT/prepare_data.py:146-169).  Inputs, all device pointers:
 * atom_ptr [G+1] (non-decreasing from 0 to N), atom_elem [N] rows of the embedding table, shell / self_idx / nbr_idx
 * [N, Ks] as cgat_neighbor_tables writes them, status [G] or NULL (a crystal is kept iff its status is 0; NULL keeps all),
 * target [G] fp64 per-cell values or NULL (y = 0).  Outputs are the arrays of a cgat_packed_dataset for the kept crystals
 * in input order, bit-identical to the host loop's: atom_ptr' [Gk+1], atom_elem' [Nk], the first K <= Ks columns of every
 * kept row as [Nk, K], comp_ptr' [Gk+1], comp_elem' [Uk] (the crystal's distinct ids in first-appearance order, not
 * sorted), comp_weight' [Uk] = (float)((double)count / (double)n_atoms), y_val [Gk] = (float)(target / (double)n) * (float)n
 * in target_mode 0 and (float)(target / (double)n) in target_mode 1 (the reference's target == "volume"), kept [Gk]
 * (indices into the input crystals).
 *   cgat_pack_dataset_plan   fills the workspace (per-crystal distinct counts and output offsets: exclusive prefix sums
 *       over the crystals, tiled, no atomics) and totals[4] = {Gk, Nk, Uk, bad}: bad counts the element ids outside
 *       [0, n_elem) plus the crystals whose atom_ptr range does not lie inside [0, N] (those read as empty).
 *   cgat_pack_dataset_write  writes the outputs; the caller has read totals, allocated exactly those sizes and passes
 *       them back as Gk, Nk, Uk with the same inputs, workspace and totals.  A write whose sizes differ from the record,
 *       or whose workspace came from other inputs, writes nothing outside the given sizes.
 * Distinct elements are found by comparing ids, nothing is gathered through one: no bound on n_elem or on the atoms of a
 * crystal, and a bad id cannot fault.  1 <= K <= Ks, N * Ks < 2^31.  Rows are copied 16 bytes at a time when K and Ks are
 * multiples of 4 and the tables are 16-byte aligned.  Bitwise deterministic; caller's stream, no allocation, no host
 * synchronisation in either call. */
size_t cgat_pack_dataset_workspace_bytes(int32_t G, int32_t N);
int cgat_pack_dataset_plan(const int32_t* atom_ptr /* [G+1] */, const int32_t* atom_elem /* [N] */,
                           const int32_t* status /* [G] or NULL */, int32_t G, int32_t N, int32_t n_elem,
                           int32_t* totals /* [4] */, void* ws, size_t ws_bytes, void* stream);
int cgat_pack_dataset_write(const int32_t* atom_ptr, const int32_t* atom_elem, const int32_t* shell /* [N,Ks] */,
                            const int32_t* self_idx, const int32_t* nbr_idx, const int32_t* status,
                            const double* target /* [G] or NULL */, int32_t G, int32_t N, int32_t Ks, int32_t K,
                            int32_t n_elem, int32_t target_mode, const int32_t* totals, const void* ws, size_t ws_bytes,
                            int32_t Gk, int32_t Nk, int32_t Uk, int32_t* out_atom_ptr /* [Gk+1] */,
                            int32_t* out_atom_elem /* [Nk] */, int32_t* out_shell /* [Nk,K] */, int32_t* out_self_idx,
                            int32_t* out_nbr_idx, int32_t* out_comp_ptr /* [Gk+1] */, int32_t* out_comp_elem /* [Uk] */,
                            float* out_comp_weight /* [Uk] */, float* out_y_val /* [Gk] */, int32_t* kept /* [Gk] */,
                            void* stream);

/* Gradient of a small embedding table looked up once per edge (reference CGAT/CGAT.py: nbr_embedding =
 * nn.Embedding(neighbor_number + 1, nbr_embedding_size), CGAtNet.forward): g_table[k, :] = sum_{t: idx[t] == k} g[t, :].
 * Deterministic (no atomics).  idx: int64 [rows]; C <= 128, K * C <= 8192. */
size_t cgat_embedding_backward_workspace_bytes(int32_t K, int32_t C);
int cgat_embedding_backward(const float* g, int64_t ldg, const int64_t* idx, int64_t rows, int32_t K, int32_t C,
                            float* g_table, void* ws, size_t ws_bytes, void* stream);

/* ---- fused optimiser steps and losses (after the hot path) -------------------
 * One launch over all parameter tensors.  `table[n_tensors]` (device) holds the tensors; the chunk list cuts them
 * into pieces of cgat_mt_chunk_elems() elements: chunk c covers table[chunk_tensor[c]] from element chunk_off[c];
 * the chunks of a tensor are consecutive and first_chunk[n_tensors+1] indexes them (LAMB's per-tensor norms).
 *   cgat_adamw_step : torch.optim.AdamW as the reference constructs it (CGAT/lightning_module.py:328-331):
 *                     p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;
 *                     p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 *   cgat_adam_step  : torch.optim.Adam as the reference constructs it (CGAT/lightning_module.py:325-327), coupled
 *                     (L2) decay: g' = g + wd*p; moments and bias corrections as cgat_adamw_step, on g'; no p *= ...
 *   cgat_sgd_step   : torch.optim.SGD(lr, weight_decay, momentum) as at CGAT/lightning_module.py:320-323 (dampening
 *                     0, no Nesterov): g' = g + wd*p;  buf = momentum*buf + g';  p -= lr*buf.  table[i].m is the
 *                     momentum buffer (zero-initialised: torch's first-step buf = clone(g') has the same bits),
 *                     table[i].v is unused and may be null.  momentum == 0: p -= lr*g', no buffer is read or
 *                     written and m may be null.
 *   cgat_lamb_step  : CGAT/lambs.py:155-181 lamb_kernel (JITLamb.step 226-262): no bias correction, weight norm
 *                     clamped to [0,10], trust ratio |w|/(|s|+eps) (1 when either norm is 0), p -= lr*ratio*s,
 *                     s = m/(sqrt(v)+eps) + wd*p.  ws: 2*n_chunks + n_tensors floats.
 *   cgat_robust_loss: CGAT/utils.py:30-47 RobustL1 (kind 1) / RobustL2 (kind 2): per-row terms and the gradients
 *                     of the terms wrt output and log_std (the caller takes the mean).
 *   cgat_loss_metrics: criterion, its gradients and the step metrics of CGAT/lightning_module.py:240-243 (276-277,
 *                     297-298) in ONE launch of one 256-thread workgroup (deterministic, no atomics).  `target` is
 *                     the raw target: t_n = (target - mean)/std and pred = output*std + mean (lines 153, 159).
 *                     kind 1 / 2: RobustL1 / RobustL2 on (output, log_std, t_n); kind 3: nn.L1Loss |output - t_n|
 *                     (gradient sign(output - t_n), 0 at equality); kind 4: nn.MSELoss (output - t_n)^2 (lines
 *                     131-142).  g_output[n] / g_log_std[n]: gradients of the MEAN loss (divided by n); for kinds 3
 *                     and 4 log_std and g_log_std may be null and are not touched.  out3 = {mean loss,
 *                     mean |pred - target|, sqrt(mean (pred - target)^2)}, summed in double, rounded to fp32 once.
 *                     n >= 1. */
typedef struct cgat_mt_tensor {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
} cgat_mt_tensor;
int32_t cgat_mt_chunk_elems(void);
int cgat_adamw_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t n_chunks,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int cgat_adam_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t n_chunks,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream);
int cgat_sgd_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t n_chunks,
                  float lr, float momentum, float weight_decay, void* stream);
int cgat_lamb_step(const cgat_mt_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t n_chunks,
                   const int32_t* first_chunk, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                   float weight_decay, float* ws, void* stream);
int cgat_robust_loss(const float* output, const float* log_std, const float* target, int32_t n, int32_t kind,
                     float* loss_terms, float* g_output, float* g_log_std, void* stream);
int cgat_loss_metrics(const float* output, const float* log_std, const float* target, int32_t n, int32_t kind, float mean,
                      float std, float* g_output, float* g_log_std, float* out3, void* stream);

/* ---- GATConvNodes message + softmax + aggregate (scalar attention) ----------------------
 * replaces CGAT/CGAT.py:319-329: m=cat[x_i,edge_attr,x_j]; alpha=softmax_dst(MH_A(m));
 * aggr = scatter_add(MH_M(m)*alpha).mean(heads), with MH_* = MultiHeadNetwork (CGAT.py:65-112).
 * Parameter tensors are exactly the reference state_dict tensors (Conv1d weights
 * [H*Hd, D, 1] / [H*out, Hd, 1] are passed as the same contiguous memory). */
typedef struct cgat_attn_params {
  int32_t C, Ce, H, Hd; /* D = 2C + Ce, columns of *_in_w ordered [x_i | edge_attr | x_j] */
  const float* A_in_w;  /* [H*Hd, D]  MH_A.fc_in.weight  */
  const float* A_in_b;  /* [H*Hd]                         */
  const float* A_out_w; /* [H, Hd]    MH_A.fc_out.weight */
  const float* A_out_b; /* [H]                            */
  const float* M_in_w;  /* [H*Hd, D]  MH_M.fc_in.weight  */
  const float* M_in_b;  /* [H*Hd]                         */
  const float* M_out_w; /* [H*C, Hd]  MH_M.fc_out.weight */
  const float* M_out_b; /* [H*C]                          */
} cgat_attn_params;
typedef struct cgat_attn_grads {
  float *A_in_w, *A_in_b, *A_out_w, *A_out_b, *M_in_w, *M_in_b, *M_out_w, *M_out_b;
} cgat_attn_grads;
/* saved-for-backward: `saved` holds Z[E,2*H*Hd] | alpha[E,H] | S[N,H*Hd] | ssum[N,H] */
size_t cgat_nodes_attention_saved_floats(int32_t N, int32_t E, int32_t H, int32_t Hd);
size_t cgat_nodes_attention_forward_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p);
size_t cgat_nodes_attention_backward_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p);
int cgat_nodes_attention_forward(const cgat_plan* plan, const cgat_attn_params* p, const float* x /* [N,C] */,
                                 const float* edge_attr /* [E,Ce], original edge order */,
                                 float* aggr /* out [N,C] = head-mean of the aggregated messages */, float* saved,
                                 void* ws, size_t ws_bytes, void* stream);
int cgat_nodes_attention_backward(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                  const float* edge_attr, const float* saved, const float* g_aggr /* [N,C] */,
                                  float* g_x /* [N,C] */, float* g_edge_attr /* [E,Ce] */, const cgat_attn_grads* g,
                                  void* ws, size_t ws_bytes, void* stream);

/* The same forward without grad (replaces CGAT/CGAT.py:307-335 where it runs under torch.no_grad(): predictions,
 * graph embeddings): aggr as cgat_nodes_attention_forward computes it, bit-identical, with nothing saved for backward.
 * Where cgat_nodes_attention_infer_fused says 1 -- a host-only predicate of shapes, arithmetic mode and edge storage:
 * the 24-bit split modes (f16x3c, bf16x6), C = Ce = 128, Hd a multiple of 128, H*Hd <= 2048, H <= 8, E*H % 4 == 0,
 * N*8*H*Hd < 2^32, any number of edges -- the per-edge
 * work of CGAT.py:319-329 (MH_A's logits, softmax, MH_M's first layer weighted by alpha and summed per destination) runs
 * as two launches that write no per-edge activation: the workspace holds the node projections, logits, alpha, the
 * per-node sums and weight images, and does not grow with E*H*Hd.  The call then refuses (CGAT_ERR_ARG) inputs those
 * launches cannot take, such as a misaligned edge_attr, instead of taking another route.  Elsewhere it runs the
 * launches of cgat_nodes_attention_forward with the saved buffer carved out of the workspace. */
int32_t cgat_nodes_attention_infer_fused(const cgat_plan* plan, const cgat_attn_params* p);
size_t cgat_nodes_attention_infer_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p);
int cgat_nodes_attention_infer(const cgat_plan* plan, const cgat_attn_params* p, const float* x /* [N,C] */,
                               const float* edge_attr /* [E,Ce], original edge order */, float* aggr /* out [N,C] */,
                               void* ws, size_t ws_bytes, void* stream);

/* The same forward without grad for shell-indexed edge features: edge_attr[e] = table[index[e]] with R rows (replaces
 * CGAT/CGAT.py:319-329 together with the edge features of 569 and 583: in the shipped network nbr_embedding's lookup and
 * every row-wise edge update keep edge_attr a lookup of at most neighbor_number + 1 rows).  Te = table W_e^T [R, 2*H*Hd] is
 * formed once and the per-edge pre-activation is the sum of three gathered rows, Te[index[e]] + Pi[dst] + Pj[src]: no
 * per-edge product, nothing of size E*H*Hd formed; the workspace grows with E by the logits and alpha alone.  Equal to
 * cgat_nodes_attention_infer on table[index] up to fp32 summation order; bitwise deterministic; no allocation, no host
 * synchronisation.  index values must lie in [0, R) (the caller validates; the kernels clamp).
 * cgat_nodes_attention_infer_indexed_ok -- a host-only predicate -- says 1 for fp32 edge storage, every arithmetic mode,
 * N, E > 0, H <= 8, Hd % 4 == 0, H*Hd <= 2048, 1 <= R <= 256 (any C, Ce; any E; 64-bit row offsets); 0 under edge storage
 * "bf16", where the dense route rounds the pre-activations and this one would not.  Where it says 0 the call returns
 * CGAT_ERR_UNSUPPORTED: the caller densifies and calls cgat_nodes_attention_infer. */
int32_t cgat_nodes_attention_infer_indexed_ok(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
size_t cgat_nodes_attention_infer_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
int cgat_nodes_attention_infer_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x /* [N,C] */,
                                       const float* table /* [R,Ce] */, int32_t R,
                                       const int64_t* index /* [E], original edge order, values in [0,R) */,
                                       float* aggr /* out [N,C] */, void* ws, size_t ws_bytes, void* stream);

/* The TRAINING form of the same route (replaces CGAT/CGAT.py:319-329 and its autograd backward on edge_attr =
 * table[index], with the embedding backward of 569 / 583 folded in).  The forward runs the launches of
 * cgat_nodes_attention_infer_indexed -- bit-identical aggr -- and keeps alpha [E,H] and ssum [N,H] in `saved`
 * (cgat_nodes_attention_indexed_saved_floats floats, on a 256-byte boundary): E*H + N*H floats plus alignment padding, no
 * pre-activations and no S.  The backward forms Pi, Pj, Te and S [N,H*Hd] again with the forward's launches on the same
 * inputs (the same bits), forms z[t] = Te[index[perm[t]]] + Pi[dst[t]] + Pj[src[t]] where the dense backward reads Z, and
 * replaces grad edge_attr / grad W_e by the class sum gT[r,:] = sum of the pre-activation gradients of class r:
 * g_table = gT W_e [R,Ce] (the gradient wrt table, embedding backward included), grad W_e = gT^T table.  No g_edge_attr
 * [E,Ce] exists.  The class grouping is the caller's, built once per (index, plan) by cgat_indexed_class_plan: cls_pos [E]
 * lists the destination-sorted slots of class 0, 1, ... in ascending slot order (a stable counting sort for few classes of
 * many rows) and every class is cut into pieces of 256 rows: piece_start [R+1], piece_rowptr
 * [cgat_indexed_class_pieces(E,R) + 1], where cgat_indexed_class_pieces(E,R) = ceil(E/256) + R bounds the piece count.  Pieces are summed in ascending order, the
 * partial rows of a class in piece order in fp64, rounded once: bitwise deterministic, no atomics.
 * cgat_nodes_attention_train_indexed_ok -- host only -- says 1 where cgat_nodes_attention_infer_indexed_ok does and
 * H*Hd % 32 == 0 (whole mask words per half), in every arithmetic mode, under fp32 edge storage ("f32") alone; where it says
 * 0 the calls return CGAT_ERR_UNSUPPORTED and the caller densifies.  Under "f16x3" the node-side products of the backward
 * run in the bf16x6 form (this route folds no tensor maxima).  No allocation, no host synchronisation; workspace sizes
 * from N, E, R and the dims alone. */
int32_t cgat_nodes_attention_train_indexed_ok(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
size_t cgat_nodes_attention_indexed_saved_floats(int32_t N, int32_t E, int32_t H, int32_t Hd);
size_t cgat_nodes_attention_forward_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
int cgat_nodes_attention_forward_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x /* [N,C] */,
                                         const float* table /* [R,Ce] */, int32_t R, const int64_t* index /* [E] */,
                                         float* aggr /* out [N,C] */, float* saved, void* ws, size_t ws_bytes,
                                         void* stream);
size_t cgat_nodes_attention_backward_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
int cgat_nodes_attention_backward_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                          const float* table, int32_t R, const int64_t* index, const int32_t* cls_pos,
                                          const int32_t* piece_rowptr, const int32_t* piece_start, const float* saved,
                                          const float* g_aggr /* [N,C] */, float* g_x /* out [N,C] */,
                                          float* g_table /* out [R,Ce] */, const cgat_attn_grads* g, void* ws,
                                          size_t ws_bytes, void* stream);
int32_t cgat_indexed_class_pieces(int32_t E, int32_t R);
size_t cgat_indexed_class_plan_workspace_bytes(int32_t E, int32_t R);
int cgat_indexed_class_plan(const cgat_plan* plan, const int64_t* index /* [E] */, int32_t R, int32_t* cls_pos /* out [E] */,
                            int32_t* piece_start /* out */, int32_t* piece_rowptr /* out */, void* ws, size_t ws_bytes,
                            void* stream);
/* Debug (tests only): the derivative pattern of that route, mask[e, c] = (z[slot(e), c] > 0) as uint8 [E, 2*H*Hd] in
 * original edge order, from x, table, index and the parameters through the forward's projections and the one function
 * that forms z for the forward and the backward (CGAT/CGAT.py:95-96,105-108). */
size_t cgat_debug_nodes_attention_signs_indexed_workspace_bytes(const cgat_plan* plan, const cgat_attn_params* p, int32_t R);
int cgat_debug_nodes_attention_signs_indexed(const cgat_plan* plan, const cgat_attn_params* p, const float* x,
                                             const float* table, int32_t R, const int64_t* index,
                                             uint8_t* mask /* out [E, 2*H*Hd] */, void* ws, size_t ws_bytes, void* stream);

/* Debug (tests only): the routes cgat_nodes_attention_forward (backward == 0) or cgat_nodes_attention_backward
 * (backward != 0) takes for this layer in the current arithmetic and edge-storage modes, for 16-byte aligned operands --
 * host only, a predicate of the shapes like cgat_nodes_attention_infer_fused.  One bit per route, from bit 0:
 *   forward:  fused_infer (what cgat_nodes_attention_infer would take; the others describe the training forward),
 *             zx, fused_z, z_bf16, proj_fast, out_fast, out_one
 *   backward: rc, vec, have_scales, z_bf16, z_bf16_six, out_fast, out_heads_one,
 *             node_ksplit, node_small_rows, node_launches, node_gemm (exactly one), node_scales,
 *             ge_ksplit, ge_launch, ge_gemm (exactly one), gw_launch, gw_gemm (exactly one)
 * named as the route structs of csrc/layers.hip, which say what each stands for.  0 for a layer attn_check refuses. */
uint32_t cgat_debug_nodes_attention_route(const cgat_plan* plan, const cgat_attn_params* p, int32_t backward);

/* Debug (tests only): WHICH KERNEL a launch of the per-edge family (csrc/edgez.hip) runs, and in what shape, in the
 * current arithmetic mode -- host only, no device call.  The forms of one launch are bit-identical by design, so no
 * result can tell which ran; this names it.
 *   launch 0: the per-edge launch, the per-node projections (adds == 0, logits == 0) and the dense layer at width 128
 *             (the same with W2 = its outputs, H = 1, Hd = 128);
 *          1: the logits launch of the forward without grad;   2: its message / weighted-sum launch (n_add_rows = N).
 *   rows, W2 (output columns), H, Hd; n_add_rows: rows of the gathered addends, 0 = not given (as the first layer of the
 *   vector-attention variants calls it); ld_add: their row stride; store: 0 fp32, 1 bf16, 2 the bit form;
 *   adds / logits / omax: whether the launch has gathered addends (and a slot permutation), forms logits, folds max |Z|;
 *   act: 0 none, 1 tanh, 2 LeakyReLU, 3 ReLU.
 * CGAT_ERR_ARG (1) where the launch itself refuses the combination. */
typedef struct cgat_edge_z_form {
  int32_t kernel;            /* 0 none (no rows), 1 the 128-row kernel, 2 the 256-row kernel, 3 the message / weighted-sum kernel */
  int32_t passes;            /* matrix passes per product: 2 (fp16 planes; three MFMA passes), 3 or 6 (bf16 planes) */
  int32_t adds;              /* the kernel variant with gathered addends */
  int32_t z_bf16;            /* Z stored (kernel 3: rounded) as bf16 */
  int32_t wide_mode;         /* kernel 2: 0 the training forward, 3 its bit form, 1 logits only */
  int32_t groups;            /* grid.y: groups the column blocks are dealt to (1: none) */
  int32_t blocks_per_group;  /* 128-column blocks each group walks */
  int32_t grid_x;            /* row tiles */
  int32_t tile_rows;         /* rows per tile */
} cgat_edge_z_form;
int cgat_debug_edge_z_form(int32_t launch, int32_t rows, int32_t W2, int32_t H, int32_t Hd, int32_t n_add_rows,
                           int64_t ld_add, int32_t store, int32_t adds, int32_t logits, int32_t omax, int32_t act,
                           cgat_edge_z_form* out);

/* Debug (tests only): WHICH FORM a launch of the backward per-edge family (csrc/edgebwd.hip) runs in the current arithmetic
 * and edge-storage modes -- host only, no device call.  The forms of one launch agree within tolerance (the bit-plane and
 * K-split forms re-round), so no parity test can tell which ran; this names it.
 *   product 0: out[t, :] = rows[t, :] @ W (edge_ge_kernel, K = W2 -> 128), launch 0 the plain launch, 1 the K-split launch
 *              with the groups the layers would give it, 2 on a caller-prepared image, 3 the heads launch (H heads);
 *           1: out[col, :] = sum_t rows[t, col] e[perm[t], :] (edge_gw_kernel, K = rows), launch 0.
 *   rows, W2 (columns of the row operand), H, Hd (the heads of a rebuilt row operand);
 *   rebuilt: the rows are rebuilt from sign bits and coefficients (the scalar-attention backward's per-edge launches);
 *   maxima: the f16x3 mode's operand maxima are given; perm: a scatter (product 0) / slot permutation (product 1) is given;
 *   force_six, te (product 1): the launch's debug switch; the edge part of grad fc_out_A is asked for.
 * CGAT_ERR_ARG (1) where the launch itself refuses the combination. */
typedef struct cgat_edge_bwd_form {
  int32_t passes;            /* matrix passes of the product: 1 (one bf16 plane), 2 (fp16 planes), 3 or 6 (bf16 planes); 0: no rows */
  int32_t rc;                /* the kernel variant that rebuilds its rows */
  int32_t bitplane;          /* the attention half runs on the stored bit */
  int32_t prep;              /* product 0, the weight image: 0 the caller's, 1 three bf16 planes, 2 fp16 planes scaled by the tensor
                                maximum, 3 the attention-scaled image with column sums, 4 the batched fp16 images of the heads */
  int32_t grid_x;            /* product 0: row tiles of 256; product 1: workgroups of the plain form */
  int32_t groups;            /* product 0: K groups over grid.y (1: none) */
  int32_t blocks_per_group;  /*            128-column blocks each group walks */
  int32_t heads;             /*            heads over grid.y (0: not the heads launch) */
  int32_t bit_shape;         /* product 1: mode and shape admit the bit-plane form, whatever the debug switches say */
  int32_t te_only;           /*            the bit-plane form runs for the edge part of grad fc_out_A alone, the plain form writes out */
  int32_t ranges;            /*            k-ranges per column-block pair of the plain form */
  int32_t SA, SM;            /*            k-ranges per attention pair / per message pair of the bit-plane form (0: no such shape) */
  int32_t message_pairs;
  int32_t bit_grid_x;        /*            workgroups of the bit-plane form: SM * message_pairs + SA * H */
  int32_t reserved;
  int64_t ws_end;            /*            floats of workspace the launch touches; ws_floats: what the size query returns */
  int64_t ws_floats;
} cgat_edge_bwd_form;
int cgat_debug_edge_bwd_form(int32_t product, int32_t launch, int32_t rows, int32_t W2, int32_t H, int32_t Hd, int32_t rebuilt,
                             int32_t maxima, int32_t perm, int32_t force_six, int32_t te, cgat_edge_bwd_form* out);

/* Debug / parity instrumentation (tests only, not on the hot path): the LeakyReLU derivative pattern the backward of
 * cgat_nodes_attention_forward will use -- mask[e, c] = (Z[slot(e), c] > 0) for the pre-activations of MH_A (columns
 * [0, H*Hd)) and MH_M ([H*Hd, 2*H*Hd)) of CGAT/CGAT.py:96,105-108, in ORIGINAL edge order.  LeakyReLU's derivative
 * jumps at 0 (CGAT.py:95, slope 0.01), so two correct fp32 evaluations can disagree on elements with |z| ~ 1e-7 max|z|
 * and then differ in every upstream gradient by a finite amount; the parity tests force the oracle's derivative
 * pattern to THIS one and compare at the flat tolerance.  fp32 edge storage only.  Under the bit form of the saved buffer
 * (cgat_nodes_attention_bit_form) the attention half is read from the stored sign words, the message half from Z_M; which
 * form `saved` is in is what the last cgat_nodes_attention_forward recorded if it filled this buffer, else what a forward
 * on 16-byte aligned x and edge_attr would choose. */
int cgat_debug_nodes_attention_signs(const cgat_plan* plan, const cgat_attn_params* p, const float* saved,
                                     uint8_t* mask /* out [E, 2*H*Hd] */, void* stream);

/* 1 if cgat_nodes_attention_forward keeps this layer's saved buffer in the BIT FORM (for 16-byte aligned operands; host
 * only): no attention pre-activations are stored.  The buffer keeps its size and the places of Z_M, alpha, S and ssum; the
 * H*Hd attention columns of its rows hold the attention halves of the two per-node projections (rows [0, N) and
 * [N, 2N)) and, from row 2N on, the sign words of 32 edge rows each.  Taken in the 24-bit arithmetic modes under edge
 * storage 0 where the forward runs its 256-row per-edge kernel (at least 128 row tiles, H*Hd <= 2048), Hd == 256 and
 * 2N + ceil(E/32) <= E; the backward then forms grad MH_A.fc_out.weight from those and the column sums of grad W_e's
 * product.  Everything else the layer returns keeps its bits.  0 everywhere else, where nothing changes. */
int32_t cgat_nodes_attention_bit_form(const cgat_plan* plan, const cgat_attn_params* p);

/* Debug / parity instrumentation (tests only): grad edge_attr's product  out[t, :] = gZ[t, :] W_e  ALONE, with the rows of
 * gZ rebuilt from caller-supplied ingredients exactly as the backward of cgat_nodes_attention_forward rebuilds them,
 *     gZ[t, (h, c)]          = ga[t, h]    * wA[h, c]           * d      (attention half, columns [0, H*Hd))
 *     gZ[t, H*Hd + (h, c)]   = alpha[t, h] * gS[dst[t], (h, c)] * d      (message half)
 * d = 1 where bit (col & 31) of mask[t, col >> 5] is set, 0.01 elsewhere -- through the launches the backward takes for
 * this product (K groups at few row tiles).  Its error against an fp64 product of the SAME inputs is that of the kernel.
 * mask [E, 2*H*Hd / 32], ga / alpha [E, H], gS [N, H*Hd], wA [H*Hd], dst [E] (< N), We [2*H*Hd, 128], out [E, 128]
 * (slot order, no scatter).  24-bit arithmetic modes, Hd a multiple of 128. */
size_t cgat_debug_edge_ge_rebuilt_workspace_bytes(int32_t E, int32_t H, int32_t Hd);
int cgat_debug_edge_ge_rebuilt(const uint32_t* mask, const float* ga, const float* alpha, const float* gS,
                               const float* wA, const int32_t* dst, const float* We, int32_t H, int32_t Hd, int32_t E,
                               float* out, void* ws, size_t ws_bytes, void* stream);

/* Debug / parity instrumentation (tests only): grad W_e's product  out[col, :] = sum_t gZ[t, col] e[perm[t], :]  ALONE, with
 * gZ rebuilt from the same caller-supplied ingredients as above, through the launch the backward takes for it.
 * e [E, 128] (original edge order), perm [E] (slot -> edge), out [2*H*Hd, 128].  force_six != 0: the six-pass form on
 * every column, whatever the route would be; *took_bitplane (host, may be null) = 1 when the attention half ran on the
 * stored bit (24-bit modes, fp32 / bf16 edge storage, Hd == 256).  Every split arithmetic mode, Hd a multiple of 128.
 * cgat_debug_edge_gw_force_six: the same switch for every later launch of the process (returns the previous value). */
int32_t cgat_debug_edge_gw_force_six(int32_t on);
size_t cgat_debug_edge_gw_rebuilt_workspace_bytes(int32_t E, int32_t H, int32_t Hd);
int cgat_debug_edge_gw_rebuilt(const uint32_t* mask, const float* ga, const float* alpha, const float* gS,
                               const float* wA, const float* e, const int32_t* perm, const int32_t* dst, int32_t H,
                               int32_t Hd, int32_t E, int32_t force_six, float* out, int32_t* took_bitplane, void* ws,
                               size_t ws_bytes, void* stream);

/* ---- first layer of the message networks alone (vector-attention variants) ---------------
 * hidden[t, :] = LeakyReLU(w_in [x_i ; edge_attr ; x_j] + b_in), t = destination-sorted edge slot (plan.dst_perm),
 * for the stacked first-layer weights w_in [W2, 2C+Ce] of any number of heads / networks: MultiHeadNetwork's
 * repeat + grouped Conv1d + LeakyReLU (CGAT/CGAT.py:96,105-108) on m = cat[x_i, edge_attr, x_j] (CGAT.py:316-318),
 * computed with the operand split and never materialising m.  The channel-wise attention of
 * vector_attention=True (CGAT.py:286-290) applies the second layers and the softmax to `hidden`. */
size_t cgat_edge_hidden_forward_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2);
size_t cgat_edge_hidden_backward_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2);
int cgat_edge_hidden_forward(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in /* [W2,2C+Ce] */,
                             const float* b_in /* [W2] */, const float* x /* [N,C] */, const float* edge_attr /* [E,Ce] */,
                             float* hidden /* [E,W2] */, float* hidden_absmax /* out [1], optional: max |hidden| */,
                             void* ws, size_t ws_bytes, void* stream);
/* g_is_pre != 0: g_hidden already is the gradient of the pre-activation (made by cgat_linear_backward_dact, which folds
 * LeakyReLU' into the product) and gpre_absmax[0] (device, optional) its maximum: no elementwise pass over [E, W2] */
int cgat_edge_hidden_backward(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in, const float* x,
                              const float* edge_attr, const float* hidden, const float* g_hidden, int32_t g_is_pre,
                              const float* gpre_absmax, float* g_x, float* g_edge_attr, float* g_w_in, float* g_b_in,
                              void* ws, size_t ws_bytes, void* stream);

/* The same first layer on SHELL-INDEXED edge features, edge_attr[e] = table[index[e]] with R rows (CGAT/CGAT.py:96,105-108
 * on the message of 316-318 with the lookups of 569 / 583): Te = table W_e^T [R,W2] once, then
 *     hidden[t, :] = LeakyReLU(Te[index[perm[t]], :] + Pi[dst[t], :] + Pj[src[t], :])
 * by a gather of three rows, with max |hidden| folded into the same launch -- no [E,Ce] tensor and no per-edge product.
 * `hidden` [E,W2] is stored as ever: the second layers read every row.  The backward takes the pre-activation gradient gZ
 * as cgat_edge_hidden_backward does (g_is_pre as there; gpre_absmax is accepted for the same call shape and not read:
 * this route runs no product that takes tensor maxima, and under "f16x3" its node-side products run in the bf16x6 form,
 * like cgat_nodes_attention_backward_indexed's), sums it by destination and by source for g_x / grad W_i / grad W_j /
 * g_b_in, and by CLASS -- gT[r,:] = sum of the gZ rows of class r, over the class plan of cgat_indexed_class_plan, every
 * piece's rows in ascending order in fp64 and rounded once, a class' partial rows in fp64 in piece order -- for g_table = gT W_e [R,Ce] (embedding backward
 * included) and grad W_e = gT^T table: the two per-edge products of the dense backward and its g_edge_attr do not exist.
 * Rows of g_table for classes no edge uses are exactly 0.  Bitwise deterministic; the one atomic on memory is the integer
 * maximum behind hidden_absmax.  cgat_edge_hidden_indexed_ok -- host only -- says 1 under fp32 edge storage ("f32") for
 * N > 0, E > 0, W2 % 4 == 0 and 1 <= R <= 256, at any width (the launch is column-wise) and in every arithmetic mode; where
 * it says 0 the calls return CGAT_ERR_UNSUPPORTED before any launch and the caller densifies.  The forward workspace holds
 * Pi, Pj, Te and the weight images: it does not grow with E.  The backward reads the class plan that was built from
 * `index` (cls_pos, piece_rowptr, piece_start), not `index` itself, which only has to be the same non-null array.  No
 * allocation, no host synchronisation. */
int32_t cgat_edge_hidden_indexed_ok(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t R);
size_t cgat_edge_hidden_forward_indexed_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t R);
int cgat_edge_hidden_forward_indexed(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2,
                                     const float* w_in /* [W2,2C+Ce] */, const float* b_in /* [W2] */,
                                     const float* x /* [N,C] */, const float* table /* [R,Ce] */, int32_t R,
                                     const int64_t* index /* [E] */, float* hidden /* out [E,W2] */,
                                     float* hidden_absmax /* out [1], optional */, void* ws, size_t ws_bytes, void* stream);
size_t cgat_edge_hidden_backward_indexed_workspace_bytes(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t R);
int cgat_edge_hidden_backward_indexed(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, const float* w_in,
                                      const float* x, const float* table, int32_t R, const int64_t* index,
                                      const int32_t* cls_pos, const int32_t* piece_rowptr, const int32_t* piece_start,
                                      const float* hidden, const float* g_hidden, int32_t g_is_pre,
                                      const float* gpre_absmax, float* g_x /* out [N,C] */, float* g_table /* out [R,Ce] */,
                                      float* g_w_in /* out [W2,2C+Ce] */, float* g_b_in /* out [W2] */, void* ws,
                                      size_t ws_bytes, void* stream);

/* Debug (tests only): the routes cgat_edge_hidden_forward (backward == 0) or cgat_edge_hidden_backward (backward != 0;
 * g_is_pre as passed to it, has_absmax != 0: with a gpre_absmax) takes at these shapes in the current arithmetic mode, for
 * 16-byte aligned operands -- host only, like cgat_debug_nodes_attention_route.  One bit per route, from bit 0:
 *   forward:  fast (the node projections and the per-edge phase on the split per-edge kernel; else the GEMM engine)
 *   backward: have_scales (the fp16 per-tensor scales of the f16x3 mode),
 *             node_ksplit, node_small_rows, node_launches, node_gemm (exactly one), node_scales,
 *             ge_ksplit, ge_launch, ge_gemm (exactly one), gw_launch, gw_gemm (exactly one)
 * named as the route structs of csrc/layers.hip.  0 for arguments the two calls refuse. */
uint32_t cgat_debug_edge_hidden_route(const cgat_plan* plan, int32_t C, int32_t Ce, int32_t W2, int32_t backward,
                                      int32_t g_is_pre, int32_t has_absmax);

/* ---- H_Net_0 / H_Net: hypernetwork Pooling_NN -------------------------------------------
 * replaces CGAT/Hypernetworksmp.py:257-313 (HyperFC of n_hyper predicted layers, each with its
 * own FCBlock trunk of n_fc Linear+Tanh and a Linear(W -> W*W+W) head; LayerNorm(no affine,
 * eps 1e-5)+Tanh after every predicted layer but the last).  All widths equal W, as
 * CGAT.py:301-305 constructs them.  damping == NULL selects H_Net_0 (hyper input = h0);
 * otherwise hyper input = d*h0 + (1-d)*v with d = *damping (already clamped by the caller,
 * Hypernetworksmp.py:310-311). */
typedef struct cgat_hyperlinear_params {
  const float* fc_w[CGAT_MAX_FC]; /* [W,W]      hypo_params.net.{s}.net.0.weight */
  const float* fc_b[CGAT_MAX_FC]; /* [W]                                          */
  const float* head_w;            /* [W*W+W, W] hypo_params.net.{n_fc}.weight    */
  const float* head_b;            /* [W*W+W]                                      */
} cgat_hyperlinear_params;
typedef struct cgat_hnet_params {
  int32_t W, n_fc, n_hyper;
  cgat_hyperlinear_params layer[CGAT_MAX_HYPER];
  const float* damping; /* device scalar or NULL */
} cgat_hnet_params;
typedef struct cgat_hyperlinear_grads {
  float* fc_w[CGAT_MAX_FC];
  float* fc_b[CGAT_MAX_FC];
  float* head_w;
  float* head_b;
} cgat_hyperlinear_grads;
typedef struct cgat_hnet_grads {
  cgat_hyperlinear_grads layer[CGAT_MAX_HYPER];
  float* damping; /* [1] or NULL */
} cgat_hnet_grads;
size_t cgat_hnet_saved_floats(int32_t rows, const cgat_hnet_params* p);
size_t cgat_hnet_forward_workspace_bytes(int32_t rows, const cgat_hnet_params* p);
size_t cgat_hnet_backward_workspace_bytes(int32_t rows, const cgat_hnet_params* p);
int cgat_hnet_forward(int32_t rows, const cgat_hnet_params* p, const float* h0 /* [rows,W] */,
                      const float* v /* [rows,W] */, float* y /* [rows,W] */, float* saved, void* ws, size_t ws_bytes,
                      void* stream);
int cgat_hnet_backward(int32_t rows, const cgat_hnet_params* p, const float* h0, const float* v, const float* saved,
                       const float* g_y, float* g_h0, float* g_v, const cgat_hnet_grads* g, void* ws, size_t ws_bytes,
                       void* stream);

/* Same backward with the four weight-gradient contractions (grad of head_w[0 : W*W]) issued on `side_stream`: they
 * feed nothing else in the pass and are matrix-core bound, so they can run beside the HBM-bound kernels that follow
 * on `stream`.  The caller owns `side_ws` (cgat_hnet_backward_side_workspace_bytes) and must keep it, `saved`, `v`,
 * `g_y` and the head_w gradient buffers alive -- and must not read those gradients -- until `side_stream` has drained. */
size_t cgat_hnet_backward_side_workspace_bytes(int32_t rows, const cgat_hnet_params* p);
int cgat_hnet_backward_overlapped(int32_t rows, const cgat_hnet_params* p, const float* h0, const float* v,
                                  const float* saved, const float* g_y, float* g_h0, float* g_v, const cgat_hnet_grads* g,
                                  void* ws, size_t ws_bytes, void* stream, void* side_ws, size_t side_ws_bytes,
                                  void* side_stream);

/* Debug (tests only): the route cgat_hnet_forward (backward == 0), cgat_hnet_backward (backward != 0) or
 * cgat_hnet_backward_overlapped (backward != 0 and overlapped != 0) takes at these rows, W, n_fc and n_hyper in the current
 * arithmetic mode, for 16-byte aligned operands -- host only, no device call; the pointers of `p` are not read.  One bit
 * per route, from bit 0:
 *   forward:  t_batched (the re-laid T of every predicted layer in two launches), w_batched (every dense-layer weight
 *             image in one launch per kind), chained (trunks + trunk-side linear term as chains), ln_fused
 *   backward: t_batched, w_batched, dual (one contraction for both bilinear input gradients),
 *             chain (a trunk's backward as one launch, now), chain_queued (... in the batched launch behind the loop;
 *             neither: layer by layer), dw_deferred (dense weight gradients wait for ONE batched launch), head_dw_queued, head_dw_rows (the head's dense weight gradients: queued, the rows kernel now, or
 *             neither: generic products), dT_side (the dT launch on the side stream), early_prep (its operands prepared
 *             per layer on the side stream), dw_side (the batched dense weight gradients on the side stream),
 *             dw_side_ws (on the main stream over the side workspace; neither: main stream and workspace)
 * named as HnetFwdRoute / HnetBwdRoute of csrc/hnet.hip.  0 for arguments the calls refuse. */
uint32_t cgat_debug_hnet_route(int32_t rows, const cgat_hnet_params* p, int32_t backward, int32_t overlapped);

/* Debug (tests only): the library's column sum alone, out[c] = alpha * sum_r x[r * ldx + c] in its fixed order (128-row
 * chunks of four lane sums each, repeated on the partials; csrc/rowops.hip), which every bias gradient goes through with
 * alpha = 1.  ws of at least cgat_debug_colsum_workspace_bytes(rows, cols). */
size_t cgat_debug_colsum_workspace_bytes(int32_t rows, int32_t cols);
int cgat_debug_colsum(const float* x, int64_t ldx, int32_t rows, int32_t cols, float* out, float alpha, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- dense layer y = act(x W^T + b)  (nn.Linear / 1x1 Conv1d group + activation) --------
 * replaces the Linear/LeakyReLU/ReLU/Tanh pairs of CGAT/message_changed.py:58-63,124-130,
 * CGAT/roost_message.py:348-352 and one head of MultiHeadNetwork (CGAT/CGAT.py:103-109).
 * act: 0 none, 1 tanh, 2 LeakyReLU(0.01), 3 ReLU.  ldx/ldw/ldy are row strides in floats. */
size_t cgat_linear_forward_workspace_bytes(int32_t M, int32_t K, int32_t N);
size_t cgat_linear_backward_workspace_bytes(int32_t M, int32_t K, int32_t N);
/* ws may be NULL (then the generic f32 GEMM engine is used for every shape).  x_absmax (optional, device pointer to
 * max |x| over the tensor x is a slice of, e.g. cgat_edge_hidden_forward's hidden_absmax): lets the K > 128 -> 128 route
 * run in the f16x3 form (three matrix passes) instead of the scale-free six-pass bf16 form */
int cgat_linear_forward(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y,
                        int64_t ldy, int32_t M, int32_t K, int32_t N, int32_t act, const float* x_absmax, void* ws,
                        size_t ws_bytes, void* stream);
/* The backward of a bias-free-activation nn.Linear whose INPUT x is itself a LeakyReLU(0.01) output (the hidden layer
 * of MultiHeadNetwork, CGAT/CGAT.py:96-98): g_x = (g_y W) * LeakyReLU'(sign of gx_dact), i.e. the gradient of the
 * pre-activation behind x, with max |g_x| folded into gx_absmax[0] (device, caller-zeroed, optional); g_w, g_b as in
 * cgat_linear_backward.  Needs N == 128 and K a multiple of 128 in a split arithmetic mode (CGAT_ERR_UNSUPPORTED
 * otherwise: use cgat_linear_backward and an elementwise pass). */
int cgat_linear_backward_dact(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* g_y, int64_t ldgy,
                              float* g_x, int64_t ldgx, const float* gx_dact, int64_t ld_dact, float* gx_absmax,
                              float* g_w, int64_t ldgw, float* g_b, int32_t M, int32_t K, int32_t N, void* ws,
                              size_t ws_bytes, void* stream);
/* The H per-head second layers of one MultiHeadNetwork in ONE call (CGAT/CGAT.py:97-98, 103-109: fc_out is a grouped
 * Conv1d = H independent Linear(K, N) on the H column blocks of the hidden matrix): head h works on x + h * s_x,
 * w + h * s_w, bias + h * s_bias, y + h * s_y (strides in elements).  Same results as H calls of cgat_linear_forward /
 * cgat_linear_backward_dact, which is also what runs for shapes the batched kernels do not take; batched (f16x3 mode,
 * N == 128, K a multiple of 128, contiguous per-head weights) the layer is 3 launches instead of 4-5 per head. */
size_t cgat_heads_linear_forward_workspace_bytes(int32_t M, int32_t K, int32_t N, int32_t H);
int cgat_heads_linear_forward(const float* x, int64_t ldx, int64_t s_x, const float* w, int64_t ldw, int64_t s_w,
                              const float* bias, int64_t s_bias, float* y, int64_t ldy, int64_t s_y, int32_t M, int32_t K,
                              int32_t N, int32_t H, const float* x_absmax, void* ws, size_t ws_bytes, void* stream);
size_t cgat_heads_linear_backward_dact_workspace_bytes(int32_t M, int32_t K, int32_t N, int32_t H);
int cgat_heads_linear_backward_dact(const float* x, int64_t ldx, int64_t s_x, const float* w, int64_t ldw, int64_t s_w,
                                    const float* g_y, int64_t ldgy, int64_t s_gy, float* g_x, int64_t ldgx, int64_t s_gx,
                                    const float* gx_dact, int64_t ld_dact, int64_t s_dact, float* gx_absmax, float* g_w,
                                    int64_t ldgw, int64_t s_gw, float* g_b, int64_t s_gb, int32_t M, int32_t K, int32_t N,
                                    int32_t H, void* ws, size_t ws_bytes, void* stream);
/* gpre = g_y * act'(y) is written to `gpre` [M,N] (caller buffer); g_x += or = per accumulate_gx */
int cgat_linear_backward(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* y, int64_t ldy,
                         const float* g_y, int64_t ldgy, float* gpre /* [M,N] dense */, float* g_x, int64_t ldgx,
                         int32_t accumulate_gx, float* g_w, int64_t ldgw, float* g_b, int32_t M, int32_t K, int32_t N,
                         int32_t act, void* ws, size_t ws_bytes, void* stream);

/* ---- segment softmax / segment sums over CSR-ordered rows --------------------------------
 * replaces torch_geometric.utils.softmax (CGAT.py:59,323; eps 1e-16), the weighted softmax of
 * roost_message.py:307-311 (mult = w**pow, eps 1e-13) and torch_scatter.scatter_add
 * (CGAT.py:60, roost_message.py:315).  Rows must be ordered by segment (rowptr[S+1]). */
int cgat_segment_softmax_forward(const float* a /* [R,F] */, const float* mult /* [R] or NULL */,
                                 const int32_t* rowptr, int32_t S, int32_t F, float eps, float* alpha /* [R,F] */,
                                 void* stream);
int cgat_segment_softmax_backward(const float* alpha, const float* g_alpha, const float* mult, const int32_t* rowptr,
                                  int32_t S, int32_t F, float* g_a, float* g_mult /* [R] or NULL, F==1 */,
                                  void* stream);
/* out[s,f] = sum_{r in seg s} x[ridx ? ridx[r] : r, f] */
int cgat_segment_sum(const float* x, int64_t ldx, const int32_t* ridx, const int32_t* rowptr, int32_t S, int32_t F,
                     float* out, int64_t ldo, void* stream);

/* Softmax-weighted segment sum ("attention pooling") in one pass per direction, rows in CSR order:
 *   out[s,f] = sum_{r in seg s} alpha[r, f/fw] * m[r,f],  fw = F / aF,
 *   alpha[r,c] = mult[r] * exp(a[r,c] - max_seg a[.,c]) / (sum_seg mult * exp(..) + eps)      (mult may be NULL)
 * = torch_geometric softmax (+1e-16) -> multiply -> scatter_add of reference CGAT.py:323-329 (vector attention:
 * aF = F), CGAT.py:59-61 (MHAttention: aF = heads) and roost_message.py:305-317 (WeightedAttention: aF = 1,
 * mult = weights ** pow, eps = 1e-13).  mx / inv [S, aF] (segment maximum, the denominator sum + eps: alpha is ONE division, as in the reference) are what backward needs
 * instead of alpha; out_lo [S, F] (may be NULL) receives the low part of the sum, which is accumulated in fp64: backward
 * centres every row on out + out_lo, so that the rounding of `out` does not enter g_a as an error common to all rows of
 * a segment.  Row r of a segment is row ridx[r] of a / mult / m (and of the gradients) when ridx != NULL.  Needs F % 4 == 0 and aF == F (aF % 4 == 0) or F / aF in {4, 8, .., 256} (a power of two). */
int cgat_segment_attention_pool_forward(const float* a, int32_t aF, const float* mult, const float* m, int64_t ldm,
                                        const int32_t* rowptr, const int32_t* ridx, int32_t S, int32_t F, float eps, float* out, float* mx,
                                        float* inv, float* out_lo, void* stream);
/* g_m[r,f] = alpha * g_out[s,f];  g_a[r,c] = sum_{f in c} alpha * g_out * (m - out - out_lo);  g_mult[r] = g_a[r,0] / mult[r]
 * (aF == 1; g_m / g_mult / out_lo may be NULL) */
int cgat_segment_attention_pool_backward(const float* a, int32_t aF, const float* mult, const float* m, int64_t ldm,
                                         const int32_t* rowptr, const int32_t* ridx, int32_t S, int32_t F, const float* out, const float* mx,
                                         const float* inv, const float* out_lo, const float* g_out, float* g_a, float* g_m,
                                         int64_t ldgm, float* g_mult, void* stream);

/* Attention pooling with training-mode attention dropout (reference CGAT.py:323-329: softmax -> F.dropout on the
 * normalised coefficients -> times the message -> scatter_add), one pass per direction:
 *   out[s,f] = sum_{r in seg s} keep[k(r), f/fw] * alpha[r, f/fw] * m[r,f] = sum_r alpha * (keep * m),
 * alpha as above without a multiplier; the maximum, the denominator (mx / inv) and the centre's normalisation do not see
 * the mask.  keep [R, aF] is the keep-mask already scaled by 1 / (1 - p) (values 0 or 1 / (1 - p)), laid out as the
 * logits; the keep row of CSR position t is k = keep_idx[t] (int32 [R]) when keep_idx != NULL -- a mask drawn in the
 * caller's edge order for operands in destination-sorted slot order -- and the operand row (ridx[t], or t) otherwise.
 * Same shape rule as cgat_segment_attention_pool_forward; keep must be 16-byte aligned when aF == F; S == 0 launches
 * nothing.  The mask is an explicit operand (no random numbers are drawn in the kernel).  No atomics, fixed summation
 * order: bitwise reproducible; with keep == 1 everywhere every output equals cgat_segment_attention_pool_* bit for bit. */
int cgat_segment_attention_pool_dropout_forward(const float* a, int32_t aF, const float* keep, const int32_t* keep_idx,
                                                const float* m, int64_t ldm, const int32_t* rowptr, const int32_t* ridx,
                                                int32_t S, int32_t F, float eps, float* out, float* mx, float* inv,
                                                float* out_lo, void* stream);
/* g_m[r,f] = keep * alpha * g_out[s,f];  g_a[r,c] = sum_{f in c} alpha * g_out * ((keep * m - out) - out_lo)
 * (g_m / out_lo may be NULL; keep receives no gradient) */
int cgat_segment_attention_pool_dropout_backward(const float* a, int32_t aF, const float* keep, const int32_t* keep_idx,
                                                 const float* m, int64_t ldm, const int32_t* rowptr, const int32_t* ridx,
                                                 int32_t S, int32_t F, const float* out, const float* mx, const float* inv,
                                                 const float* out_lo, const float* g_out, float* g_a, float* g_m,
                                                 int64_t ldgm, void* stream);

/* Head combination of the per-edge hypernetwork edge update, GATConvEdges(no_hyper=False) (reference CGAT.py:214-223:
 * exp -> sum over the heads -> division -> attention dropout -> times the message -> mean over the heads), one kernel
 * per direction.  sa [E, H, aF] logits, sm [E, H, Co] messages, aF == Co (vector attention, c' = c) or aF == 1 (c' = 0):
 *   alpha[t,h,c']            = exp(sa[t,h,c']) / sum_h' exp(sa[t,h',c'])     (no max-subtraction, ONE division: as the reference)
 *   out[perm ? perm[t] : t, c] = (sum_h alpha[t,h,c'] * keep[t,h,c'] * sm[t,h,c]) / H
 * keep [E, H, aF] is the dropout keep-mask scaled by 1 / (1 - p), NULL = no dropout; perm [E] (the plan's dst_perm when
 * the rows are destination-sorted slots), NULL = rows already in output order.  Needs Co % 4 == 0, Co <= 256,
 * 1 <= H <= 8, 16-byte aligned operands; E == 0 launches nothing.  No workspace, no atomics (bitwise reproducible). */
int cgat_edge_head_combine_forward(const float* sa, int32_t aF, const float* sm, const float* keep, const int32_t* perm,
                                   int64_t E, int32_t H, int32_t Co, float* out /* [E, Co] */, void* stream);
/* alpha is recomputed from sa (nothing but the inputs is saved).  With g = g_out[perm ? perm[t] : t, :] / H:
 *   g_sm[t,h,c]  = g[c] * alpha[t,h,c'] * keep[t,h,c']
 *   q_h[c']      = sum over the channels c that share c' of g[c] * sm[t,h,c] * keep[t,h,c']
 *   g_sa[t,h,c'] = alpha_h * (q_h - sum_h' alpha_h' * q_h')
 * g_sa / g_sm may be NULL when that gradient is not needed.  With aF == 1 the sums over the Co channels run in a fixed
 * order inside the row's lane group, and g_sa (E * H values) is formed in fp64 and rounded once; where the forward's
 * fp32 denominator is not finite or zero, the row's g_sa is NaN as the row of `out` is. */
int cgat_edge_head_combine_backward(const float* sa, int32_t aF, const float* sm, const float* keep, const int32_t* perm,
                                    const float* g_out /* [E, Co] */, int64_t E, int32_t H, int32_t Co, float* g_sa,
                                    float* g_sm, void* stream);

/* A chain of up to 5 dense layers of width 128 in ONE launch (the split arithmetic modes f16x3, f16x3c, bf16x6;
 * CGAT_ERR_UNSUPPORTED in the f32 mode; the workspace holds one prepared weight image of 24576 floats per layer):
 *   r_0 = x                      (times act'(in_dact) if in_dact != NULL; stored to in_store if != NULL)
 *   r_(l+1) = act_l(r_l W_l^T + bias_l) (+ resid_l) (* dact_type_l'(dact_l)),   W_l(o,k) = W[o*w_so + k*w_sk]
 * every r_(l+1) is written to out_l when out_l != NULL (+= when accumulate).  Forward of the hypernetwork trunks
 * (reference Hypernetworksmp.py:36-83: four Linear+Tanh, then the linear terms of the predicted layer), their backward
 * (the same chain on the transposed weights with the tanh derivatives as in_dact / dact), and the edge update's
 * two-layer network with its residual (CGAT.py:226-229, 580-585).  Rows stay in registers between layers; only the
 * requested outputs touch HBM.  All row pointers 16-byte aligned, leading dimensions multiples of 4. */
typedef struct cgat_chain_layer {
  const float* W;
  int64_t w_so, w_sk;
  const float* bias;      /* [128] or NULL */
  const float* dact;      /* NULL, or saved activation values [rows,128]: result *= act'(dact) with act = dact_type */
  int64_t ld_dact;
  const float* resid;     /* NULL, or [rows,128] added to the activated result */
  int64_t ld_resid;
  float* out;             /* NULL, or destination [rows,128] */
  int64_t ld_out;
  int32_t act;            /* 0 none, 1 tanh, 2 LeakyReLU(0.01), 3 ReLU */
  int32_t dact_type;
  int32_t accumulate;
} cgat_chain_layer;
typedef struct cgat_chain_desc {
  int32_t n_layers, rows;
  const float* x;
  int64_t ldx;
  const float* in_dact;
  int64_t ld_in_dact;
  int32_t in_dact_type;
  float* in_store;
  int64_t ld_in_store;
  cgat_chain_layer layer[5];
} cgat_chain_desc;
size_t cgat_mlp_chain_workspace_bytes(int32_t n_layers);
int cgat_mlp_chain(const cgat_chain_desc* d, void* ws, size_t ws_bytes, void* stream);

/* Weight (and bias) gradients of many width-128 dense layers in ONE launch: for item i < n
 *     out[i][o][k] = sum_r G[i][r,o] X[i][r,k]   (128 x 128, row stride ldo),   bsum[i][o] = sum_r G[i][r,o]  (or NULL)
 * i.e. what autograd accumulates into nn.Linear.weight / .bias of the hypernetwork's trunk layers and linear terms
 * (Hypernetworksmp.py:24-60, 77-83) and of the per-head second layers (CGAT.py:103-109): exact fp32 products
 * (f32-input MFMA), fixed summation order.  All items share rows, ldg, ldx, ldo; n <= 32; G, X 16-byte aligned. */
size_t cgat_dense_wgrad_batch_workspace_bytes(int32_t n, int32_t rows);
int cgat_dense_wgrad_batch(int32_t n, const float* const* G, int64_t ldg, const float* const* X, int64_t ldx,
                           float* const* out, int64_t ldo, float* const* bsum, int32_t rows, void* ws, size_t ws_bytes,
                           void* stream);

/* ---- small-row dense-layer programs: a whole G-row / Nc-row network per launch ------------------------------------
 * At the batch the reference harness ships (--batch-size 64, CGAT/lightning_module.py:468-473) the output head
 * (ResidualNetwork, CGAT/message_changed.py:81-138: per layer act(fc(x)) + res_fc(x), then fc_out), Roost's gate and
 * message networks (SimpleNetwork, CGAT/roost_message.py:137-153, 324-355) and the per-crystal networks of MHAttention
 * (CGAT/CGAT.py:14-62) are products over 64 ... 2 048 rows: bound by kernel boundaries, not by flops.  A program is a
 * list of products
 *     out[m,n] = act( alpha sum_k A'(m,k) B0(n,k) + bias[n] ) [-> h_out[m,n]]  +  sum_k A(m,k) B1(n,k)  +  resid[m,n]  +  beta out[m,n]
 *     A'(m,k)  = A(m,k) * dact_type'(dact(m,k))     (dact = saved activation VALUES; NULL: A' = A)
 *     rowsum[m] = sum_k A'(m,k)                       (optional: a bias gradient)
 * with X(r,k) = X[r * x_rs + k * x_ks] for A, dact, B0, B1 -- so one op is a forward layer with its residual product
 * (A = x, B0 = fc.weight, B1 = res_fc.weight), an input gradient (A = g_y, dact = h, B0 = W^T, B1 = R^T) or a weight
 * gradient (A = g_y^T, dact = h^T, B0 = x^T, rowsum = the bias gradient) -- run by ONE persistent launch phase by
 * phase: the ops of a phase must not depend on each other, phase p may read what phases < p wrote (a grid barrier with
 * device-scope release / acquire separates them).  Exact fp32 products with fp32 accumulation (f32-input MFMA), fixed
 * summation order; no workspace, no operand images.  act / dact_type: 0 none, 1 tanh, 2 LeakyReLU(0.01), 3 ReLU.
 * B1, bias, resid, h_out, rowsum, dact may be NULL.  Meant for M, N <= a few thousand.
 * sync_words: CGAT_ROWPROG_SYNC_WORDS uint32 of device memory, 64-byte aligned, zero-filled by the caller ONCE and then
 * left to the library for the life of the process (barrier counters that every launch returns to zero, and one sticky
 * word -- index CGAT_ROWPROG_SYNC_WORDS - 16 -- that is set to 1 if a barrier ever gave up instead of hanging: the
 * results of that launch are void). */
#define CGAT_ROWPROG_MAX_OPS 24
#define CGAT_ROWPROG_SYNC_WORDS ((1024 + 1) * 16)
typedef struct cgat_rowprog_op {
  int32_t phase;            /* non-decreasing over the op list, starting at 0, no gaps */
  int32_t M, N, K;
  const float* A;     int64_t a_rs, a_ks;
  const float* dact;  int64_t d_rs, d_ks;  int32_t dact_type;
  const float* B0;    int64_t b0_rs, b0_ks;
  const float* B1;    int64_t b1_rs, b1_ks;
  const float* bias;  /* [N] */
  int32_t act;
  const float* resid; int64_t ld_resid;
  float* out;         int64_t ldo;
  float alpha, beta;  /* beta == 0: out is not read */
  float* h_out;       int64_t ld_h;
  float* rowsum;      /* [M] */
} cgat_rowprog_op;
typedef struct cgat_rowprog {
  int32_t n_ops;
  cgat_rowprog_op op[CGAT_ROWPROG_MAX_OPS];
} cgat_rowprog;
int cgat_rowprog_run(const cgat_rowprog* prog, uint32_t* sync_words, void* stream);

/* Storage of the per-edge intermediates of cgat_nodes_attention_*: the pre-activations Z saved by forward, and their
 * gradient gZ inside backward -- which at the benchmark widths is NOT stored at all but rebuilt by its consumers from
 * one sign bit per element and per-node rows (same values to fp32 rounding).
 *   0 = fp32 Z (default);
 *   1 = bf16 Z ("bf16 activations" of BASELINE configs[4]): halves the bytes of the Z-sized passes; attention logits,
 *       softmax statistics, sums and every matrix product stay as they are (fp32 accumulation); tolerance of that mode
 *       1e-2 max-norm relative.  Exists for the scalar-attention node layer at C = Ce = 128, Hd a multiple of 128, in every
 *       split arithmetic mode (f16x3c, bf16x6, f16x3); cgat_nodes_attention_forward / _backward return
 *       CGAT_ERR_UNSUPPORTED for a layer without that form (other widths, the f32 mode) instead of running it in fp32
 *       storage under the bf16 label (round 4's library ignored the switch there);
 *   2 = fp32 Z with gZ stored in backward (round 1's path, 6 KB more workspace per edge): the A/B reference of the tests.
 *   4 = fp32 with the attention pre-activations stored at every shape ("f32+za"): mode 0 without the bit form of the saved
 *       buffer (cgat_nodes_attention_bit_form), its A/B reference; identical to mode 0 wherever that form is not taken.
 * A backward call must run under the mode its forward ran under.  Env CGAT_EDGE_STORAGE = bf16 | f32+gz | bf16-mma |
 * f32+za sets the start value. */
void cgat_set_edge_storage(int32_t mode);
int32_t cgat_get_edge_storage(void);

/* ---- kernel-level primitives (what the layer entry points above are composed of) --------- */
/* C = act(alpha * A.B + bias + add1[add1_idx[m]] + add2[add2_idx[m]]) + beta * C on the fp32 matrix
 * cores.  A(m,k) = A[row(m)*lda + k] (a_kmajor=0, row(m)=a_rgather?a_rgather[m]:m) or A[k*lda + m]
 * (a_kmajor=1); B(k,n) = B[n*ldb + k] (b_kmajor=0, i.e. a torch Linear weight) or
 * B[krow(k)*ldb + n] (b_kmajor=1, krow(k)=b_kgather?b_kgather[k]:k); output row = c_scatter?c_scatter[m]:m.
 * splits > 1 splits K over workgroups (deterministic slab reduction; needs workspace). */
typedef struct cgat_gemm_desc {
  int32_t M, N, K;
  const float* A;
  int64_t lda;
  int32_t a_kmajor;
  const int32_t* a_rgather;
  const float* B;
  int64_t ldb;
  int32_t b_kmajor;
  const int32_t* b_kgather;
  float* C;
  int64_t ldc;
  const int32_t* c_scatter;
  float alpha, beta;
  const float* bias;
  const float* add1;
  const int32_t* add1_idx;
  const float* add2;
  const int32_t* add2_idx;
  int64_t ld_add;
  int32_t act;
  int32_t splits; /* 0 = choose automatically */
  int64_t a_block; /* != 0: A stored as 128-wide column blocks [cols/128][rows][128], block stride in floats;
                      the blocked dimension is k (a_kmajor=0) or m (a_kmajor=1); lda must be 128 */
} cgat_gemm_desc;
size_t cgat_gemm_workspace_bytes(const cgat_gemm_desc* d);
int cgat_gemm(const cgat_gemm_desc* d, void* ws, size_t ws_bytes, void* stream);
/* out[n,c] = init[n,c] + sum_{a<NA,b<NB} p[n,a] q[n,b] T[(a*NB+b)*NC + c]   (init may be NULL or == out).
 * The workspace holds the kernel-side re-layout of T and the partial slabs of the a-split. */
size_t cgat_bilinear_rows_workspace_bytes(int32_t rows, int32_t NA, int32_t NB, int32_t NC);
int cgat_bilinear_rows(const float* p, int64_t ldp, const float* q, int64_t ldq, const float* T, const float* init,
                       int64_t ldi, float* out, int64_t ldo, int32_t rows, int32_t NA, int32_t NB, int32_t NC,
                       void* ws, size_t ws_bytes, void* stream);
/* Two gradients of the hypernetwork's trilinear form from ONE contraction (backward of reference
 * Hypernetworksmp.py:77-83, HyperLinear.forward; widths fixed at 128):
 *   out1[n,c] = init1[n,c] + sum_{a,b} p[n,a] q[n,b] T[(a*128+b)*128 + c]
 *   out2[n,a] = init2[n,a] + sum_{b,c} zz[n,c] q[n,b] T[(a*128+b)*128 + c]
 * (init1/init2 may be NULL or alias their outputs).  In the f32 arithmetic mode it runs as two contractions. */
size_t cgat_bilinear_dual_workspace_bytes(int32_t rows);
int cgat_bilinear_dual(const float* p, int64_t ldp, const float* q, int64_t ldq, const float* zz, int64_t ldz,
                       const float* T, const float* init1, int64_t ldi1, float* out1, int64_t ldo1, const float* init2,
                       int64_t ldi2, float* out2, int64_t ldo2, int32_t rows, void* ws, size_t ws_bytes, void* stream);
/* Arithmetic of the width-128 matrix-core kernels: 2 (default, "f16x3") = operands scaled by a power of two and
 * split into two fp16 pieces, three fp16-MFMA passes with fp32 accumulation (measured at the error of an fp32 product
 * chain); 6 ("bf16x6") = three bf16 pieces, six bf16-MFMA passes (same accuracy, twice the matrix work); 3 = three bf16
 * passes (~4e-6 relative, fails the parity tests: diagnostic only); 0 = f32-input MFMA (exact fp32 fmaf chains) and the
 * f32 GEMM engine for the edge products.  Env CGAT_BILINEAR_MODE = f16x3 | bf16x6 | bf16x3 | f32 sets the start value. */
void cgat_set_bilinear_mode(int32_t mode);
int32_t cgat_get_bilinear_mode(void);
/* out[(a*NB+b)*NC + c] = sum_n p[n,a] q[n,b] r[n,c] */
size_t cgat_bilinear_wgrad_workspace_bytes(int32_t rows, int32_t NA, int32_t NB, int32_t NC);
int cgat_bilinear_wgrad(const float* p, int64_t ldp, const float* q, int64_t ldq, const float* r, int64_t ldr,
                        float* out, int32_t rows, int32_t NA, int32_t NB, int32_t NC, void* ws, size_t ws_bytes,
                        void* stream);
/* y = tanh(LayerNorm(u)) without affine, biased variance (Hypernetworksmp.py:103-107) and its backward */
int cgat_layernorm_tanh_forward(const float* u, float* y, int32_t rows, int32_t W, float eps, void* stream);
int cgat_layernorm_tanh_backward(const float* u, const float* y, const float* g_y, float* g_u, int32_t rows, int32_t W,
                                 float eps, void* stream);

/* ---- sparse variational GP head on graph embeddings (prediction with uncertainty) -----------------------
 * The prediction side of the reference's screening flow: CGAT/gaussian_process.py:45-66 (ScaleKernel(RBFKernel) with one
 * lengthscale, ConstantMean / ZeroMean, whitened VariationalStrategy + CholeskyVariationalDistribution) as evaluated at
 * :247-268 (latent distribution, no likelihood noise; confidence region mean +- 2 stddev; denorm by std, mean) and used
 * by Utilities/gp_predict.py:29 (uncertainty = upper - prediction).  With k_x[m] = s exp(-max(|x - z_m|^2, 0) inv_two_l2),
 * L = chol(K_zz + jitter I), a = L^-T m, W1 = L^-1, W2 = L_S^T L^-1:
 *   mean_f = c + k_x . a        var_f = max(s - |W1 k_x|^2 + |W2 k_x|^2, 0)
 *   pred = mean_f tgt_std + tgt_mean        lower / upper = (mean_f -+ 2 sqrt(var_f)) tgt_std + tgt_mean
 * One launch over tiles of 32 rows of X on the f32-input matrix cores; the tile of the G x M cross-kernel matrix stays in
 * LDS (32 x M x 4 B), hence M <= 1024: a larger M returns 4 (unsupported) with a message.  G = 0 launches nothing.
 * Operands (device, fp32; Mp = M rounded up to 32, Dp = D rounded up to 64; padding is zero):
 *   X [G, D] rows ldx apart;  centroid [D] of Z;  znorm [Mp] = |z_m - centroid|^2;
 *   Zimg: the packed image of Z - centroid as [Mp, Dp];  factors: a [Mp], then the packed image of [W1; W2] as
 *   [2 Mp, Mp] (W1 in rows 0 .., W2 in rows Mp ..).  W1 must be lower triangular: its column blocks past the diagonal
 *   are not read.  Packed image of P [R, Kd]: img[((c Kd/8 + k8) 64 + lane) 4 + q] = P[32 c + (lane & 31)][8 k8 + 2 q +
 *   (lane >> 5)]; both images 16-byte aligned.
 * Outputs [G]: mean_f, var_f; pred, lower, upper each or NULL.  No workspace is needed (the query returns 0).  No
 * atomics: bitwise deterministic; caller's stream, no allocation, no synchronisation. */
size_t cgat_gp_predict_workspace_bytes(int32_t G, int32_t M, int32_t D);
int cgat_gp_predict(const float* X, int64_t ldx, int32_t G, int32_t D, const float* Zimg, int32_t M,
                    const float* centroid, const float* znorm, const float* factors, float c, float s, float inv_two_l2,
                    float tgt_mean, float tgt_std, float* mean_f, float* var_f, float* pred, float* lower, float* upper,
                    void* ws, size_t ws_bytes, void* stream);

/* ---- sufficient statistics of the collapsed sparse-GP bound (fitting the head above) ---------------------
 * The reference trains the GP of CGAT/gaussian_process.py:45-66 by minibatch AdamW on gpytorch's VariationalELBO with a
 * GaussianLikelihood (:59, :233), targets normalised by torch.mean / torch.std (:200-204), Z a random batch of training
 * embeddings (:223-226).  For a Gaussian likelihood that bound has a closed-form maximiser in the variational
 * distribution (Titsias' collapsed bound), and the data enter only through
 *   gram = sum_n a~_n a~_n^T,   a~_n = [W1 k(Z, x_n), y_norm[n], 1],   k as in cgat_gp_predict,   W1 = L^-1
 * which this entry accumulates in one pass over X (cgat_amd/gp.py solves the rest on the host in fp64).
 * gram [(M+2) x (M+2)], fp64, row-major, symmetric (both triangles are written, bit-equal):
 *   gram[i][j], i, j < M : Psi = sum_n a_n a_n^T        gram[i][M] : sum_n a_n y_n        gram[i][M+1] : sum_n a_n
 *   gram[M][M] : sum_n y_n^2        gram[M][M+1] : sum_n y_n        gram[M+1][M+1] : N (exactly)
 * Operands as for cgat_gp_predict (X [N, D] rows ldx apart, Zimg, centroid, znorm); W1img is the packed image of W1 as
 * [Mp, Mp], lower triangular, zero padded, 16-byte aligned; y_norm [N] fp32.  X is processed in chunks of chunk_rows rows
 * (a positive multiple of 32; 32768 is the intended value; more than N rounded up to 32 counts as that): per chunk the
 * whitened rows go to a chunk buffer in the workspace, their Gram product is formed on the f32-input matrix cores in
 * fp32 over slabs of 1024 rows, and the slabs are added in fp64 in a fixed order.  M > 1024 returns 4 (unsupported) with
 * a message, as cgat_gp_predict does.  The workspace (query below; 0 for arguments the entry refuses) must be 16-byte
 * aligned.  No atomics: bitwise deterministic; caller's stream, no allocation, no synchronisation. */
size_t cgat_gp_fit_stats_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows);
int cgat_gp_fit_stats(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D, const float* Zimg, int32_t M,
                      const float* centroid, const float* znorm, const float* W1img, float s, float inv_two_l2,
                      int32_t chunk_rows, double* gram, void* ws, size_t ws_bytes, void* stream);

/* ---- data part of the gradient of the collapsed bound in (Z, log l, log s) ------------------------------
 * With (m, L_S, c, sigma^2) at their maximisers the derivative of the bound with respect to the kernel's parameters is the
 * partial derivative at fixed (c, sigma^2).  Its dependence on the data is a second pass over X with the adjoints of the
 * statistics, G2 = 2 dF/dPsi [M x M] (symmetric) and g = dF/dbeta [M], computed on the host in fp64 (cgat_amd/gp.py):
 *   a_n = W1 k_n,  q_n = G2 a_n + g (y_norm[n] - c),  u_n = W1^T q_n,  r_nm = u_nm k_nm,  k as in cgat_gp_predict
 *   colsum[m] = sum_n r_nm    d2sum[m] = sum_n r_nm max(|x_n - z_m|^2, 0)    P[m][d] = sum_n r_nm (x_n[d] - centroid[d])
 * from which dF/dlog l = sum_m d2sum[m] / l^2 and dF/dZ = (P - colsum o (Z - centroid)) / l^2 (data parts).
 * Outputs fp64: colsum [M], d2sum [M], P [M, D] row-major.  Operands as for cgat_gp_fit_stats, plus W1timg and G2img, the
 * packed images of W1^T (upper triangular: its column blocks before the diagonal are not read) and of G2 as [Mp, Mp], zero
 * padded, 16-byte aligned; g [M] and c in fp32.  The three products are formed one after the other on the f32-input matrix
 * cores per tile of 32 rows (never as one M x M factor), the intermediates pass through a chunk buffer in the workspace,
 * the distances are recomputed next to k; the sums over rows are fp32 per tile of 32 rows (colsum, d2sum) or per slab of
 * 1024 rows (P) and added in fp64 in a fixed order.  chunk_rows, M > 1024, the workspace and its query as for
 * cgat_gp_fit_stats.  No atomics: bitwise deterministic; caller's stream, no allocation, no synchronisation. */
size_t cgat_gp_fit_grad_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows);
int cgat_gp_fit_grad(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D, const float* Zimg, int32_t M,
                     const float* centroid, const float* znorm, const float* W1img, const float* W1timg,
                     const float* G2img, const float* g, float c, float s, float inv_two_l2, int32_t chunk_rows,
                     double* colsum, double* d2sum, double* P, void* ws, size_t ws_bytes, void* stream);

/* ---- the same pass with the gradient of the bound in the embeddings (deep-kernel learning) ---------------
 * The reference fits its GP (CGAT/gaussian_process.py:45-66, bound at :233) on the embeddings of a frozen network; to train
 * the network under that bound one needs dF/dX.  The RBF kernel's k(x, x) = s is constant, so the bound depends on X only
 * through k_nm, and with r of cgat_gp_fit_grad and rho_n = sum_m r_nm (at fixed (m, L_S, c, sigma^2): the envelope theorem)
 *   dX[n][d] = (sum_m r_nm (Z - centroid)[m][d] - rho_n (x_n[d] - centroid[d])) 2 inv_two_l2 = dF/dx_n[d]
 * one more product per tile of 32 rows on the f32-input matrix cores, from the r the pass leaves in its chunk buffer, with
 * rho added over m in a fixed order.  Everything else is cgat_gp_fit_grad: both entries run one implementation, colsum,
 * d2sum and P are bit-equal between them, and cgat_gp_fit_grad_workspace_bytes serves both (dX is written directly).
 * Ztimg: the packed image of (Z - centroid)^T as [Dq, Mp], Dq = D rounded up to 32, zero padded, 16-byte aligned.
 * dX [N, D] fp32, rows lddx >= D apart; columns at or past D of a row and rows at or past N are never written; 16-byte
 * stores are used where dX and lddx allow them.  A null Ztimg or dX, lddx < D or a misaligned Ztimg return 1 (argument)
 * before any launch.  No atomics: bitwise deterministic, and a row's dX does not depend on chunk_rows. */
int cgat_gp_fit_grad_inputs(const float* X, int64_t ldx, const float* y_norm, int32_t N, int32_t D, const float* Zimg,
                            int32_t M, const float* centroid, const float* znorm, const float* W1img, const float* W1timg,
                            const float* G2img, const float* g, float c, float s, float inv_two_l2, int32_t chunk_rows,
                            double* colsum, double* d2sum, double* P, const float* Ztimg, float* dX, int64_t lddx,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- derivative of the head's prediction in its input: the backward of cgat_gp_predict -------------------
 * The reference evaluates its GP at CGAT/gaussian_process.py:247-268 on the embeddings of a frozen network; a loss of the
 * prediction (held-out error, predictive density, an acquisition value) that is to reach the network needs dL/dX.  With
 * alpha = W1 k_x, S = L_S L_S^T and k as in cgat_gp_predict, mean_f = c + alpha . m and var_f = s + alpha^T (S - I) alpha,
 * so per row n with the upstream gradients gm[n] = dL/dmean_f and gv[n] = dL/dvar_f and G2 = 2 (S - I)
 *   q_n = gv[n] G2 alpha_n + gm[n] m,   u_n = W1^T q_n,   r_nm = u_nm k_nm,   rho_n = sum_m r_nm
 *   dX[n][d] = (sum_m r_nm (Z - centroid)[m][d] - rho_n (x_n[d] - centroid[d])) 2 inv_two_l2 = dL/dx_n[d]
 * the chain of cgat_gp_fit_grad_inputs with a per-row coefficient on the G2 product and without its sums over the rows.
 * Operands as there: X [G, D] rows ldx apart, Zimg / centroid / znorm, the packed images W1img (lower triangular), W1timg
 * (upper), G2img (symmetric) as [Mp, Mp] and Ztimg as [Dq, Mp], zero padded, 16-byte aligned; m [M] the variational mean;
 * gm, gv [G] fp32, finite.  A null gv means "mean only" (alpha is then not formed), a null gm "variance only"; both null is
 * an argument error.  The clamp of var_f at 0 is the caller's: pass gv = 0 for such a row.  Per chunk of chunk_rows rows the
 * three products are formed one after the other on the f32-input matrix cores through a chunk buffer in the workspace; the
 * last kernel recomputes the distances, keeps the tile of r in LDS, adds rho over m in a fixed order and forms dX, so r never
 * reaches memory.  dX [G, D] fp32, rows lddx >= D apart; columns at or past D of a row are never written.  G < 1, lddx < D, a
 * null or misaligned operand return 1 (argument), M > 1024 returns 4 (unsupported), a short workspace 3, each with a message
 * and before any launch.  The workspace (query below; 0 for arguments the entry refuses) is the chunk buffer alone,
 * 16-byte aligned.  No atomics: bitwise deterministic, and a row's dX does not depend on chunk_rows; caller's stream, no
 * allocation, no synchronisation. */
size_t cgat_gp_predict_backward_workspace_bytes(int32_t G, int32_t M, int32_t D, int32_t chunk_rows);
int cgat_gp_predict_backward(const float* X, int64_t ldx, int32_t G, int32_t D, const float* Zimg, int32_t M,
                             const float* centroid, const float* znorm, const float* W1img, const float* W1timg,
                             const float* G2img, const float* m, const float* gm, const float* gv, float s,
                             float inv_two_l2, int32_t chunk_rows, const float* Ztimg, float* dX, int64_t lddx, void* ws,
                             size_t ws_bytes, void* stream);

/* ---- one Lloyd step of k-means over the embeddings: inducing points at the centres of the data ----------
 * The reference normalises the targets and starts its inducing points from one random batch of training embeddings
 * (CGAT/gaussian_process.py:208-226); the usual recipe for a sparse GP moves such a start by k-means.  Per row n of X
 *   a_n = argmin_{m < M} max(|x_n - z_m|^2, 0), a tie to the smaller m;   d_n = that minimum
 *   counts[m] = #{n : a_n = m}     wss[m] = sum_{a_n = m} d_n     P[m][d] = sum_{a_n = m} (x_n[d] - centroid[d])
 * so the next centre is centroid + P[m] / counts[m] (an empty cluster has counts[m] = 0 and P[m] = 0) and sum_m wss[m] is
 * the inertia of the assignment.  Outputs: assign [N] int32; fp64 counts [M] (exact integers), wss [M], P [M, D]
 * row-major.  Operands as for cgat_gp_fit_stats: X [N, D] rows ldx apart, Zimg / centroid / znorm of the centres Z (a
 * padded centre never receives a row).  The distances are formed as in cgat_gp_predict on the f32-input matrix cores; the
 * one-hot assignment of a chunk passes through the chunk buffer and P is formed by the slab product of cgat_gp_fit_grad;
 * the sums are fp32 per tile of 32 rows (counts, wss) or per slab of 1024 rows (P) and added in fp64 in a fixed order.
 * chunk_rows, M > 1024, the workspace and its query (equal to cgat_gp_fit_grad_workspace_bytes) as for cgat_gp_fit_stats.
 * No atomics: bitwise deterministic; caller's stream, no allocation, no synchronisation. */
size_t cgat_gp_kmeans_step_workspace_bytes(int32_t N, int32_t M, int32_t D, int32_t chunk_rows);
int cgat_gp_kmeans_step(const float* X, int64_t ldx, int32_t N, int32_t D, const float* Zimg, int32_t M,
                        const float* centroid, const float* znorm, int32_t chunk_rows, int32_t* assign, double* counts,
                        double* wss, double* P, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CGAT_HIP_H */
