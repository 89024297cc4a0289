// Dataset packing on the device: from the finished neighbour tables (csrc/neighbors.hip) and flat per-atom
// element ids to the arrays of a cgat_packed_dataset, for the crystals whose status is 0, in input order.  Replaces the
// per-crystal host loop of cgat_amd/collate.py PackedDataset.from_dict (and of the reference's
// CompositionData.__getitem__, CGAT/data.py:61-103, 140-141): element ids per atom, the composition (distinct elements
// in first-appearance order, weight = count / n_atoms), the tables sliced to their first K columns, y = target * n_atoms.
// Integer work plus two fp32 roundings, so the arrays are bit-identical to the host loop's.
//
//   plan : (a) pack_count_kernel   per crystal: distinct elements, ids outside [0, n_elem)
//          (b) pack_scan_kernel<0> sums per tile of PACK_SCAN_TILE crystals of (keep, keep*atoms, keep*distinct, bad)
//              pack_tiles_kernel   one workgroup: exclusive scan of the tile sums, totals record
//              pack_scan_kernel<1> exclusive scan inside every tile + tile offset -> per-crystal output offsets
//   write: (c) pack_write_kernel   one wave per kept crystal of <= 64 atoms, the workgroup for a wider one
//
// "Distinct" is decided by comparing ids (atom i opens an element iff no atom j < i carries the same id), never by
// indexing with an id: any n_elem and any id is safe, and a crystal of n atoms costs n compares per atom -- 64 shuffles
// inside a wave for the usual crystal, n broadcast LDS reads per atom for a wide one (1024 atoms: about 4 k reads per
// thread).  The scans use no atomics: the same inputs give the same bits.
#include "../../include/cgat_hip.h"
#include "common.h"

#define PACK_THREADS 256
#define PACK_WAVES 4           // crystals per workgroup of (a) and (c): one per wave
#define PACK_SCAN_TILE 1024    // crystals per workgroup of (b): 4 per thread
#define PACK_ELEM_TILE 1024    // element ids of a wide crystal staged in LDS per pass

struct PackWs {                // views into the caller's workspace, all [G] but tile_sum [4 * tiles]
  int32_t *nuniq, *bad, *off_g, *off_a, *off_u, *tile_sum;
};
static inline int pack_tiles(int G) { return cdiv(G, PACK_SCAN_TILE); }
static size_t pack_ws_bytes(int G) { return 5 * ws_round((size_t)G, 4) + ws_round((size_t)4 * pack_tiles(G), 4) + 256; }
static bool pack_ws_take(void* ws, size_t bytes, int G, PackWs* v) {
  Workspace w(ws, bytes);
  v->nuniq = w.take<int32_t>(G); v->bad = w.take<int32_t>(G);
  v->off_g = w.take<int32_t>(G); v->off_a = w.take<int32_t>(G); v->off_u = w.take<int32_t>(G);
  v->tile_sum = w.take<int32_t>((size_t)4 * pack_tiles(G));
  return w.ok;
}

// atoms [a0, a0 + n) of crystal g; a range that is not inside [0, N] reads as empty and is counted with the bad ids
__device__ inline bool pack_range(const int32_t* __restrict__ atom_ptr, int g, int N, int& a0, int& n) {
  a0 = atom_ptr[g];
  const int a1 = atom_ptr[g + 1];
  const bool ok = a0 >= 0 && a1 >= a0 && a1 <= N;
  n = ok ? a1 - a0 : 0;
  if (!ok) a0 = 0;
  return ok;
}
__device__ inline bool pack_keep(const int32_t* __restrict__ status, int g) { return status == nullptr || status[g] == 0; }

// ---- distinct elements of one crystal -----------------------------------------------------------------------------
// wave form, n <= 64: lane = atom.  cnt = atoms of the crystal with this lane's id; returns the lanes that open an element
__device__ inline unsigned long long pack_wave_distinct(int e, bool valid, int n, int lane, int& cnt) {
  bool first = valid;
  cnt = 0;
  for (int j = 0; j < n; ++j) {
    const bool eq = __shfl(e, j) == e;
    cnt += eq;
    first = first && !(eq && j < lane);
  }
  return __ballot(first);
}
// workgroup form: every thread takes atom i (i >= n: idle) and compares it with all n ids, staged through `tile`
__device__ inline bool pack_block_distinct(const int32_t* __restrict__ elem, int n, int i, int e, bool valid,
                                           int32_t* tile, int& cnt) {
  bool first = valid;
  cnt = 0;
  for (int j0 = 0; j0 < n; j0 += PACK_ELEM_TILE) {
    const int m = min(PACK_ELEM_TILE, n - j0);
    __syncthreads();
    for (int t = threadIdx.x; t < m; t += PACK_THREADS) tile[t] = elem[j0 + t];
    __syncthreads();
    for (int j = 0; j < m; ++j) {
      const bool eq = tile[j] == e;
      cnt += eq;
      first = first && !(eq && j0 + j < i);
    }
  }
  return first;
}

// ---- (a) ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PACK_THREADS) void pack_count_kernel(const int32_t* __restrict__ atom_ptr,
                                                                  const int32_t* __restrict__ atom_elem, int G, int N,
                                                                  int n_elem, int32_t* __restrict__ nuniq,
                                                                  int32_t* __restrict__ bad) {
  __shared__ int32_t tile[PACK_ELEM_TILE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  {
    const int g = blockIdx.x * PACK_WAVES + w;
    int a0, n = 0;
    const bool ok = g < G && pack_range(atom_ptr, g, N, a0, n);
    if (g < G && n <= 64) {
      const int e = lane < n ? atom_elem[a0 + lane] : -1;
      const bool valid = lane < n && e >= 0 && e < n_elem;
      int cnt;
      const unsigned long long firsts = pack_wave_distinct(e, valid, n, lane, cnt);
      const unsigned long long bads = __ballot(lane < n && !valid);
      if (lane == 0) { nuniq[g] = __popcll(firsts); bad[g] = __popcll(bads) + (ok ? 0 : 1); }
    }
  }
  for (int c = 0; c < PACK_WAVES; ++c) {           // the wide crystals of this group, by all four waves (uniform branch)
    const int g = blockIdx.x * PACK_WAVES + c;
    if (g >= G) break;
    int a0, n;
    pack_range(atom_ptr, g, N, a0, n);
    if (n <= 64) continue;
    int nu = 0, nb = 0;
    for (int i0 = 0; i0 < n; i0 += PACK_THREADS) {
      const int i = i0 + tid;
      const int e = i < n ? atom_elem[a0 + i] : -1;
      const bool valid = i < n && e >= 0 && e < n_elem;
      int cnt;
      const bool first = pack_block_distinct(atom_elem + a0, n, i, e, valid, tile, cnt);
      nu += __syncthreads_count(first);
      nb += __syncthreads_count(i < n && !valid);
    }
    if (tid == 0) { nuniq[g] = nu; bad[g] = nb; }
  }
}

// ---- (b) ----------------------------------------------------------------------------------------------------------
struct Pack3 { int g, a, u; };
__device__ inline Pack3 operator+(Pack3 x, Pack3 y) { return {x.g + y.g, x.a + y.a, x.u + y.u}; }
// exclusive scan of one Pack3 per thread over the workgroup, in thread order; *total = the sum of all
__device__ inline Pack3 pack_block_scan(Pack3 v, Pack3* total, Pack3* wave_sum /* LDS [PACK_WAVES] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Pack3 inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const Pack3 t = {__shfl_up(inc.g, d), __shfl_up(inc.a, d), __shfl_up(inc.u, d)};
    if (lane >= d) inc = inc + t;
  }
  __syncthreads();
  if (lane == 63) wave_sum[w] = inc;
  __syncthreads();
  Pack3 before = {0, 0, 0}, all = {0, 0, 0};
  for (int k = 0; k < PACK_WAVES; ++k) {
    if (k < w) before = before + wave_sum[k];
    all = all + wave_sum[k];
  }
  *total = all;
  return {before.g + inc.g - v.g, before.a + inc.a - v.a, before.u + inc.u - v.u};
}
__device__ inline Pack3 pack_crystal_sizes(const int32_t* __restrict__ atom_ptr, const int32_t* __restrict__ status,
                                           const int32_t* __restrict__ nuniq, int g, int G, int N) {
  if (g >= G || !pack_keep(status, g)) return {0, 0, 0};
  int a0, n;
  pack_range(atom_ptr, g, N, a0, n);
  return {1, n, nuniq[g]};
}
// APPLY = 0: the tile's sums (and its count of bad ids) into tile_sum[4 * tile ..]; APPLY = 1: tile_sum holds the tile's
// offsets, every crystal gets its own
template <int APPLY>
__global__ __launch_bounds__(PACK_THREADS) void pack_scan_kernel(const int32_t* __restrict__ atom_ptr,
                                                                 const int32_t* __restrict__ status, int G, int N,
                                                                 PackWs ws) {
  __shared__ Pack3 wave_sum[PACK_WAVES];
  __shared__ int bad_sum[PACK_WAVES];
  const int tid = threadIdx.x, g0 = blockIdx.x * PACK_SCAN_TILE + tid * 4;
  Pack3 v[4], mine = {0, 0, 0};
  for (int q = 0; q < 4; ++q) {
    v[q] = pack_crystal_sizes(atom_ptr, status, ws.nuniq, g0 + q, G, N);
    mine = mine + v[q];
  }
  Pack3 total;
  Pack3 off = pack_block_scan(mine, &total, wave_sum);
  if (APPLY) {
    const int32_t* base = ws.tile_sum + 4 * blockIdx.x;
    off = off + Pack3{base[0], base[1], base[2]};
    for (int q = 0; q < 4 && g0 + q < G; ++q) {
      ws.off_g[g0 + q] = off.g; ws.off_a[g0 + q] = off.a; ws.off_u[g0 + q] = off.u;
      off = off + v[q];
    }
  } else {
    int nb = 0;                                    // bad ids of every crystal, kept or not
    for (int q = 0; q < 4 && g0 + q < G; ++q) nb += ws.bad[g0 + q];
    for (int d = 32; d > 0; d >>= 1) nb += __shfl_down(nb, d);
    if ((tid & 63) == 0) bad_sum[tid >> 6] = nb;
    __syncthreads();
    if (tid == 0) {
      int32_t* o = ws.tile_sum + 4 * blockIdx.x;
      o[0] = total.g; o[1] = total.a; o[2] = total.u;
      o[3] = bad_sum[0] + bad_sum[1] + bad_sum[2] + bad_sum[3];
    }
  }
}
// one workgroup: tile sums -> exclusive tile offsets (in place), totals = {Gk, Nk, Uk, bad ids}
__global__ __launch_bounds__(PACK_THREADS) void pack_tiles_kernel(int32_t* __restrict__ tile_sum, int tiles,
                                                                  int32_t* __restrict__ totals) {
  __shared__ Pack3 wave_sum[PACK_WAVES];
  __shared__ int bad_sum[PACK_WAVES];
  const int tid = threadIdx.x;
  Pack3 carry = {0, 0, 0};
  int nb = 0;
  for (int t0 = 0; t0 < tiles; t0 += PACK_THREADS) {
    const int t = t0 + tid;
    Pack3 v = {0, 0, 0};
    if (t < tiles) { v = {tile_sum[4 * t], tile_sum[4 * t + 1], tile_sum[4 * t + 2]}; nb += tile_sum[4 * t + 3]; }
    Pack3 total;
    const Pack3 off = pack_block_scan(v, &total, wave_sum) + carry;
    if (t < tiles) { tile_sum[4 * t] = off.g; tile_sum[4 * t + 1] = off.a; tile_sum[4 * t + 2] = off.u; }
    carry = carry + total;
  }
  for (int d = 32; d > 0; d >>= 1) nb += __shfl_down(nb, d);
  if ((tid & 63) == 0) bad_sum[tid >> 6] = nb;
  __syncthreads();
  if (tid == 0) {
    totals[0] = carry.g; totals[1] = carry.a; totals[2] = carry.u;
    totals[3] = bad_sum[0] + bad_sum[1] + bad_sum[2] + bad_sum[3];
  }
}

// ---- (c) ----------------------------------------------------------------------------------------------------------
struct PackIn {
  const int32_t *atom_ptr, *atom_elem, *shell, *self_idx, *nbr_idx, *status;
  const double* target;
  int G, N, Ks, K, n_elem, mode;
};
struct PackOut {
  int32_t *atom_ptr, *atom_elem, *shell, *self_idx, *nbr_idx, *comp_ptr, *comp_elem;
  float *comp_weight, *y_val;
  int32_t* kept;
  int Gk, Nk, Uk;
};
// first K of Ks columns of rows [a0, a0 + n) -> rows [o0, o0 + n) of a [., K] table; thread t of `step`
template <bool VEC>
__device__ inline void pack_copy_rows(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int a0, int o0, int n,
                                      int Ks, int K, int t, int step) {
  if (VEC) {
    const int K4 = K >> 2, Ks4 = Ks >> 2;
    const int4* s = reinterpret_cast<const int4*>(src) + (long)a0 * Ks4;
    int4* d = reinterpret_cast<int4*>(dst) + (long)o0 * K4;
    for (int i = t; i < n * K4; i += step) {
      const int r = i / K4, c = i - r * K4;
      d[i] = s[(long)r * Ks4 + c];
    }
  } else {
    const int32_t* s = src + (long)a0 * Ks;
    int32_t* d = dst + (long)o0 * K;
    for (int i = t; i < n * K; i += step) {
      const int r = i / K, c = i - r * K;
      d[i] = s[(long)r * Ks + c];
    }
  }
}
template <bool VEC>
__device__ inline void pack_copy_crystal(const PackIn& in, const PackOut& out, int a0, int o0, int n, int t, int step) {
  pack_copy_rows<VEC>(in.shell, out.shell, a0, o0, n, in.Ks, in.K, t, step);
  pack_copy_rows<VEC>(in.self_idx, out.self_idx, a0, o0, n, in.Ks, in.K, t, step);
  pack_copy_rows<VEC>(in.nbr_idx, out.nbr_idx, a0, o0, n, in.Ks, in.K, t, step);
}
// where crystal g goes, or false: dropped, or outside the planned sizes (a plan of other inputs: nothing is written)
__device__ inline bool pack_place(const PackIn& in, const PackOut& out, const PackWs& ws, int g, int& a0, int& n, int& og,
                                  int& o0, int& u0, int& nu) {
  if (g >= in.G || !pack_keep(in.status, g)) return false;
  pack_range(in.atom_ptr, g, in.N, a0, n);
  og = ws.off_g[g]; o0 = ws.off_a[g]; u0 = ws.off_u[g]; nu = ws.nuniq[g];
  return og >= 0 && og < out.Gk && o0 >= 0 && n <= out.Nk - o0 && u0 >= 0 && nu >= 0 && nu <= out.Uk - u0;
}
__device__ inline void pack_crystal_head(const PackIn& in, const PackOut& out, int g, int n, int og, int o0, int u0) {
  out.kept[og] = g;
  out.atom_ptr[og] = o0;
  out.comp_ptr[og] = u0;
  float y = 0.f;
  if (in.target != nullptr) {
    y = (float)(in.target[g] / (double)n);       // the stored target: per-cell value over the atom count, fp64, rounded once
    if (in.mode == 0) y = y * (float)n;          // data.py:140-141: times n_atoms in fp32 unless target == "volume"
  }
  out.y_val[og] = y;
}

template <bool VEC>
__global__ __launch_bounds__(PACK_THREADS) void pack_write_kernel(PackIn in, PackOut out, PackWs ws,
                                                                  const int32_t* __restrict__ totals) {
  __shared__ int32_t tile[PACK_ELEM_TILE];
  __shared__ int wave_firsts[PACK_WAVES];
  // the outputs were sized from the totals of the plan this workspace holds, or nothing is written
  if (totals[0] != out.Gk || totals[1] != out.Nk || totals[2] != out.Uk) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) { out.atom_ptr[out.Gk] = out.Nk; out.comp_ptr[out.Gk] = out.Uk; }
  {
    const int g = blockIdx.x * PACK_WAVES + w;
    int a0, n, og, o0, u0, nu;
    if (pack_place(in, out, ws, g, a0, n, og, o0, u0, nu) && n <= 64) {
      if (lane == 0) pack_crystal_head(in, out, g, n, og, o0, u0);
      const int e = lane < n ? in.atom_elem[a0 + lane] : -1;
      if (lane < n) out.atom_elem[o0 + lane] = e;
      const bool valid = lane < n && e >= 0 && e < in.n_elem;
      int cnt;
      const unsigned long long firsts = pack_wave_distinct(e, valid, n, lane, cnt);
      const int rank = __popcll(firsts & ((1ull << lane) - 1ull));
      if (((firsts >> lane) & 1ull) && rank < nu) {
        out.comp_elem[u0 + rank] = e;
        out.comp_weight[u0 + rank] = (float)((double)cnt / (double)n);
      }
      pack_copy_crystal<VEC>(in, out, a0, o0, n, lane, 64);
    }
  }
  for (int c = 0; c < PACK_WAVES; ++c) {           // the wide crystals of this group, by all four waves (uniform branch)
    const int g = blockIdx.x * PACK_WAVES + c;
    int a0, n, og, o0, u0, nu;
    if (!pack_place(in, out, ws, g, a0, n, og, o0, u0, nu) || n <= 64) continue;
    if (tid == 0) pack_crystal_head(in, out, g, n, og, o0, u0);
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += PACK_THREADS) {
      const int i = i0 + tid;
      const int e = i < n ? in.atom_elem[a0 + i] : -1;
      if (i < n) out.atom_elem[o0 + i] = e;
      const bool valid = i < n && e >= 0 && e < in.n_elem;
      int cnt;
      const bool first = pack_block_distinct(in.atom_elem + a0, n, i, e, valid, tile, cnt);
      const unsigned long long firsts = __ballot(first);
      __syncthreads();
      if (lane == 0) wave_firsts[w] = __popcll(firsts);
      __syncthreads();
      int rank = base + __popcll(firsts & ((1ull << lane) - 1ull));
      for (int k = 0; k < PACK_WAVES; ++k) {
        if (k < w) rank += wave_firsts[k];
        base += wave_firsts[k];
      }
      if (first && rank < nu) {
        out.comp_elem[u0 + rank] = e;
        out.comp_weight[u0 + rank] = (float)((double)cnt / (double)n);
      }
    }
    pack_copy_crystal<VEC>(in, out, a0, o0, n, tid, PACK_THREADS);
  }
}

// ---- entry points -------------------------------------------------------------------------------------------------
extern "C" size_t cgat_pack_dataset_workspace_bytes(int32_t G, int32_t N) {
  (void)N;
  return G < 0 ? 0 : pack_ws_bytes(G);
}

extern "C" int cgat_pack_dataset_plan(const int32_t* atom_ptr, const int32_t* atom_elem, const int32_t* status, int32_t G,
                                      int32_t N, int32_t n_elem, int32_t* totals, void* ws, size_t ws_bytes,
                                      void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CGAT_CHECK_ARG(G >= 0 && N >= 0 && n_elem >= 0, "pack_dataset_plan: bad sizes");
  CGAT_CHECK_ARG(atom_ptr && totals && (atom_elem || N == 0), "pack_dataset_plan: null atom_ptr/atom_elem/totals");
  PackWs v;
  if (!ws || !pack_ws_take(ws, ws_bytes, G, &v)) {
    cgat_set_error("pack_dataset_plan: workspace too small (cgat_pack_dataset_workspace_bytes)");
    return CGAT_ERR_WORKSPACE;
  }
  CGAT_PROF("pack_plan", s);
  const int tiles = pack_tiles(G);
  if (G > 0) {
    hipLaunchKernelGGL(pack_count_kernel, dim3(cdiv(G, PACK_WAVES)), dim3(PACK_THREADS), 0, s, atom_ptr, atom_elem, G, N,
                       n_elem, v.nuniq, v.bad);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(pack_scan_kernel<0>, dim3(tiles), dim3(PACK_THREADS), 0, s, atom_ptr, status, G, N, v);
    CGAT_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pack_tiles_kernel, dim3(1), dim3(PACK_THREADS), 0, s, v.tile_sum, tiles, totals);
  CGAT_LAUNCH_CHECK();
  if (G > 0) {
    hipLaunchKernelGGL(pack_scan_kernel<1>, dim3(tiles), dim3(PACK_THREADS), 0, s, atom_ptr, status, G, N, v);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}

extern "C" int cgat_pack_dataset_write(const int32_t* atom_ptr, const int32_t* atom_elem, const int32_t* shell,
                                       const int32_t* self_idx, const int32_t* nbr_idx, const int32_t* status,
                                       const double* target, int32_t G, int32_t N, int32_t Ks, int32_t K, int32_t n_elem,
                                       int32_t target_mode, const int32_t* totals, const void* ws, size_t ws_bytes,
                                       int32_t Gk, int32_t Nk, int32_t Uk, int32_t* out_atom_ptr, int32_t* out_atom_elem,
                                       int32_t* out_shell, int32_t* out_self_idx, int32_t* out_nbr_idx,
                                       int32_t* out_comp_ptr, int32_t* out_comp_elem, float* out_comp_weight,
                                       float* out_y_val, int32_t* kept, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CGAT_CHECK_ARG(G >= 0 && N >= 0 && n_elem >= 0 && K >= 1 && K <= Ks, "pack_dataset_write: needs 1 <= K <= Ks");
  CGAT_CHECK_ARG(target_mode == 0 || target_mode == 1, "pack_dataset_write: target_mode is 0 (times n_atoms) or 1 (as stored)");
  CGAT_CHECK_ARG(Gk >= 0 && Gk <= G && Nk >= 0 && Nk <= N && Uk >= 0 && Uk <= Nk, "pack_dataset_write: planned sizes out of range");
  CGAT_CHECK_ARG((long)N * Ks < (1l << 31) && (long)Nk * K < (1l << 31), "pack_dataset_write: N * Ks needs 32-bit row offsets");
  CGAT_CHECK_ARG(atom_ptr && totals && out_atom_ptr && out_comp_ptr, "pack_dataset_write: null atom_ptr/totals/outputs");
  CGAT_CHECK_ARG(N == 0 || (atom_elem && shell && self_idx && nbr_idx), "pack_dataset_write: null input tables");
  CGAT_CHECK_ARG(Gk == 0 || (out_y_val && kept), "pack_dataset_write: null y_val/kept");
  CGAT_CHECK_ARG(Nk == 0 || (out_atom_elem && out_shell && out_self_idx && out_nbr_idx), "pack_dataset_write: null output tables");
  CGAT_CHECK_ARG(Uk == 0 || (out_comp_elem && out_comp_weight), "pack_dataset_write: null composition outputs");
  PackWs v;
  if (!ws || !pack_ws_take(const_cast<void*>(ws), ws_bytes, G, &v)) {
    cgat_set_error("pack_dataset_write: workspace too small (cgat_pack_dataset_workspace_bytes)");
    return CGAT_ERR_WORKSPACE;
  }
  CGAT_PROF("pack_write", s);
  const PackIn in = {atom_ptr, atom_elem, shell, self_idx, nbr_idx, status, target, G, N, Ks, K, n_elem, target_mode};
  const PackOut out = {out_atom_ptr, out_atom_elem, out_shell, out_self_idx, out_nbr_idx, out_comp_ptr, out_comp_elem,
                       out_comp_weight, out_y_val, kept, Gk, Nk, Uk};
  const uintptr_t align = (uintptr_t)shell | (uintptr_t)self_idx | (uintptr_t)nbr_idx | (uintptr_t)out_shell |
                          (uintptr_t)out_self_idx | (uintptr_t)out_nbr_idx;
  const bool vec = (K & 3) == 0 && (Ks & 3) == 0 && (align & 15) == 0;   // 16-byte row copies, else one int at a time
  const dim3 grid(G > 0 ? cdiv(G, PACK_WAVES) : 1);                      // G == 0: the closing pointer entries alone
  if (vec)
    hipLaunchKernelGGL(pack_write_kernel<true>, grid, dim3(PACK_THREADS), 0, s, in, out, v, totals);
  else
    hipLaunchKernelGGL(pack_write_kernel<false>, grid, dim3(PACK_THREADS), 0, s, in, out, v, totals);
  CGAT_LAUNCH_CHECK();
  return CGAT_OK;
}
