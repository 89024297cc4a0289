// Neighbour tables on the device: the three integer tables a PackedDataset is packed from -- shell id, centre
// index and neighbour index per atom, [n_atoms, K] -- straight from lattice + fractional coordinates.  Replaces the
// reference's offline stage CGAT/prepare_data.py:146-169 (pymatgen's get_all_neighbors(radius), a Python sort and a Python
// loop per atom).  All geometry is fp64.
//
// Definition (shared with tests/neighbor_cases.py): wrapped f_j = frac_j - floor(frac_j), r_j = f_j . L; the candidates
// of atom i are all (j, R in Z^3) with 1e-8 < d = |r_j + R.L - r_i| <= radius; sorted by d, shell ids by the chain rule
// of prepare_data.py:163-169 (a candidate opens the next shell iff d > first distance of the current shell + 1e-8); the
// row keeps the first K, the shell holding the K-th place taken in ascending j; the row is ordered by (shell, j).
//
// One workgroup per atom.  A pass searches a working radius r_w <= radius (first guess from the number density: about
// 3K candidates): lanes stride over (image, j), survivors go to an LDS list through one LDS counter, the list is sorted
// on (d, j) by a bitonic network.  The pass is accepted only when it provably is the full-radius answer:
//   d_K + 1e-8 < r_w   (every member of the shell holding the K-th place, and everything before it, lies inside r_w)
// or r_w == radius.  Otherwise r_w grows (to d_K + 1e-6, which the next pass must accept, or by a factor when fewer than K
// were found); a list that would overflow the LDS buffer shrinks r_w instead, bisecting once both bounds are known.  An
// atom that finds neither within NB_MAX_PASSES, a crystal of more than NB_MAX_ATOMS atoms, a lattice without volume and a
// search of more than NB_MAX_EVALS (image, j) pairs mark the crystal status 2; fewer than K candidates at the full
// radius mark it status 1.  The compaction order is not deterministic; both sorts use total orders, so the output is.
#include "../../include/cgat_hip.h"
#include "common.h"
#include "kernels.h"

#define NB_THREADS 256
#define NB_MAX_ATOMS 1024          // atoms per crystal: their Cartesian positions live in LDS (24 KB)
#define NB_CAP 2048                // candidate list: 8-byte distance + 4-byte key each (24 KB)
#define NB_MAX_PASSES 24
#define NB_MAX_EVALS 67108864.0    // 2^26 (image, j) pairs per pass
#define NB_SHELL_EPS 1e-8
#define NB_FAIL_FEW 1              // bits collected in status[] by the row kernel; nb_finalize_kernel maps them to 1 / 2
#define NB_FAIL_LIMIT 2

typedef unsigned long long nb_u64;

// MODE 0: by (distance, j); MODE 1: by (shell << 11 | j, distance).  Distances are positive doubles: their bit patterns
// order as unsigned integers.
template <int MODE>
__device__ __forceinline__ bool nb_less(nb_u64 a1, unsigned b1, nb_u64 a2, unsigned b2) {
  if (MODE == 0) return a1 < a2 || (a1 == a2 && b1 < b2);
  return b1 < b2 || (b1 == b2 && a1 < a2);
}

// bitonic sort of the first P (a power of two, <= NB_CAP) entries, ascending; every thread of the block calls it
template <int MODE>
__device__ void nb_bitonic(nb_u64* A, unsigned* B, int P, int tid) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += NB_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool up = (i & k) == 0;
        const nb_u64 ai = A[i], al = A[l];
        const unsigned bi = B[i], bl = B[l];
        if (nb_less<MODE>(al, bl, ai, bi) == up) {
          A[i] = al; A[l] = ai;
          B[i] = bl; B[l] = bi;
        }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int nb_pow2_at_least(int m) {
  int p = 1;
  while (p < m) p <<= 1;
  return p;
}

__global__ __launch_bounds__(NB_THREADS) void nb_rows_kernel(const double* __restrict__ lattice,
                                                             const double* __restrict__ frac,
                                                             const int32_t* __restrict__ atom_ptr, int G, int N, int K,
                                                             double radius, int cap, double first_radius,
                                                             int32_t* __restrict__ shell, int32_t* __restrict__ self_idx,
                                                             int32_t* __restrict__ nbr_idx, double* __restrict__ dist,
                                                             int32_t* __restrict__ status, int32_t* __restrict__ passes) {
// the distances are the plain IEEE sums of the definition: no contraction into fma, so a host restatement of the same
// expressions gives the same bits
#pragma clang fp contract(off)
  __shared__ double pos[3][NB_MAX_ATOMS];
  __shared__ nb_u64 A[NB_CAP];
  __shared__ unsigned B[NB_CAP];
  __shared__ int s_cnt, s_p1;
  const int tid = threadIdx.x;
  const int row = blockIdx.x;
  // crystal of this atom: the largest g with atom_ptr[g] <= row
  int g = 0;
  {
    int lo = 0, hi = G;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (atom_ptr[mid] <= row) lo = mid; else hi = mid;
    }
    g = lo;
  }
  const int a0 = atom_ptr[g], n = atom_ptr[g + 1] - a0;
  const int il = row - a0;
  if (a0 < 0 || n <= 0 || il < 0 || il >= n || (long)a0 + n > (long)N) return;   // atom_ptr not a partition of the rows
  if (passes && tid == 0) passes[row] = 0;
  double L[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) L[q] = lattice[(long)g * 9 + q];
  // interplanar spacings h_a = V / |b x c| (and cyclic): |R_a| <= floor(r / h_a) + 1 covers radius r for wrapped coordinates
  const double bcx = L[4] * L[8] - L[5] * L[7], bcy = L[5] * L[6] - L[3] * L[8], bcz = L[3] * L[7] - L[4] * L[6];
  const double cax = L[7] * L[2] - L[8] * L[1], cay = L[8] * L[0] - L[6] * L[2], caz = L[6] * L[1] - L[7] * L[0];
  const double abx = L[1] * L[5] - L[2] * L[4], aby = L[2] * L[3] - L[0] * L[5], abz = L[0] * L[4] - L[1] * L[3];
  const double V = fabs(L[0] * bcx + L[1] * bcy + L[2] * bcz);
  const double ha = V / sqrt(bcx * bcx + bcy * bcy + bcz * bcz);
  const double hb = V / sqrt(cax * cax + cay * cay + caz * caz);
  const double hc = V / sqrt(abx * abx + aby * aby + abz * abz);
  const bool geom_ok = V > 0.0 && V < 1e300 && ha > 0.0 && hb > 0.0 && hc > 0.0 && ha < 1e300 && hb < 1e300 && hc < 1e300;
  if (n > NB_MAX_ATOMS || !geom_ok) {
    if (tid == 0) atomicOr(&status[g], NB_FAIL_LIMIT);
    return;
  }
  for (int j = tid; j < n; j += NB_THREADS) {
    const double* f = frac + (long)(a0 + j) * 3;
    const double f0 = f[0] - floor(f[0]), f1 = f[1] - floor(f[1]), f2 = f[2] - floor(f[2]);
    pos[0][j] = f0 * L[0] + f1 * L[3] + f2 * L[6];
    pos[1][j] = f0 * L[1] + f1 * L[4] + f2 * L[7];
    pos[2][j] = f0 * L[2] + f1 * L[5] + f2 * L[8];
  }
  __syncthreads();
  const double rix = pos[0][il], riy = pos[1][il], riz = pos[2][il];

  // first working radius: a sphere expected to hold 3K + 16 candidates at the crystal's number density
  double r_w = first_radius > 0.0 ? first_radius : cbrt((3.0 * K + 16.0) * V * 0.2387324146378430 / (double)n);
  if (!(r_w < radius)) r_w = radius;
  double lo_r = 0.0, hi_r = -1.0;      // largest radius known too small, smallest radius known to overflow (none yet)
  int fail = 0, M = 0, pass = 0;
  for (;;) {
    ++pass;
    const double xa = floor(r_w / ha * (1.0 + 1e-12)) + 1.0, xb = floor(r_w / hb * (1.0 + 1e-12)) + 1.0,
                 xc = floor(r_w / hc * (1.0 + 1e-12)) + 1.0;
    const double evals = (2.0 * xa + 1.0) * (2.0 * xb + 1.0) * (2.0 * xc + 1.0) * (double)n;
    if (!(evals <= NB_MAX_EVALS)) { fail = NB_FAIL_LIMIT; break; }
    const int ma = (int)xa, mb = (int)xb, mc = (int)xc;
    const unsigned nb = 2 * mb + 1, nc = 2 * mc + 1, tot = (unsigned)evals;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (unsigned t = tid; t < tot; t += NB_THREADS) {
      unsigned c = t / (unsigned)n;
      const int j = (int)(t - c * (unsigned)n);
      const unsigned c2 = c / nc;
      const int Rc = (int)(c - c2 * nc) - mc;
      const unsigned c3 = c2 / nb;
      const int Rb = (int)(c2 - c3 * nb) - mb;
      const int Ra = (int)c3 - ma;
      const double fa = (double)Ra, fb = (double)Rb, fc = (double)Rc;
      const double dx = (pos[0][j] + (fa * L[0] + fb * L[3] + fc * L[6])) - rix;
      const double dy = (pos[1][j] + (fa * L[1] + fb * L[4] + fc * L[7])) - riy;
      const double dz = (pos[2][j] + (fa * L[2] + fb * L[5] + fc * L[8])) - riz;
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      if (d > NB_SHELL_EPS && d <= r_w) {
        const int slot = atomicAdd(&s_cnt, 1);
        if (slot < cap) {
          A[slot] = (nb_u64)__double_as_longlong(d);
          B[slot] = (unsigned)j;
        }
      }
    }
    __syncthreads();
    M = s_cnt;
    double next;
    if (M > cap) {                       // the list overflowed: a smaller radius
      hi_r = r_w;
      next = lo_r > 0.0 ? 0.5 * (lo_r + hi_r) : 0.7 * r_w;
    } else if (M >= K) {
      const int P = nb_pow2_at_least(M);
      for (int t = M + tid; t < P; t += NB_THREADS) { A[t] = ~(nb_u64)0; B[t] = ~0u; }
      __syncthreads();
      nb_bitonic<0>(A, B, P, tid);
      const double dK = __longlong_as_double((long long)A[K - 1]);
      if (r_w >= radius || dK + NB_SHELL_EPS < r_w) break;     // accepted: the list holds the full-radius prefix
      lo_r = r_w;
      next = dK + 1e-6;                  // the K-th distance can only shrink as the radius grows: this one is accepted
    } else {
      if (r_w >= radius) { fail = NB_FAIL_FEW; break; }
      lo_r = r_w;
      next = 1.4 * r_w;
    }
    if (pass >= NB_MAX_PASSES) { fail = NB_FAIL_LIMIT; break; }
    if (hi_r > 0.0 && next >= hi_r) next = 0.5 * (lo_r + hi_r);
    if (!(next < radius)) next = radius;
    r_w = next;
    __syncthreads();                     // everyone has read s_cnt and the list before the next pass resets them
  }
  if (passes && tid == 0) passes[row] = pass;
  if (fail) {
    if (tid == 0) atomicOr(&status[g], fail);
    return;                              // the crystal's rows are zero-filled by nb_finalize_kernel
  }
  // shell ids by the chain rule, up to the end of the shell that holds the K-th place
  if (tid == 0) {
    double first = __longlong_as_double((long long)A[0]);
    unsigned sh = 1;
    int p = 0;
    for (; p < M; ++p) {
      const double d = __longlong_as_double((long long)A[p]);
      if (d > first + NB_SHELL_EPS) {
        if (p >= K) break;
        first = d;
        ++sh;
      }
      B[p] = (sh << 11) | B[p];
    }
    s_p1 = p;
  }
  __syncthreads();
  const int p1 = s_p1;
  const int P2 = nb_pow2_at_least(p1);
  for (int t = p1 + tid; t < P2; t += NB_THREADS) { A[t] = ~(nb_u64)0; B[t] = ~0u; }
  __syncthreads();
  nb_bitonic<1>(A, B, P2, tid);          // by (shell, j): the first K are the row, the cut shell in ascending j
  if (tid < K) {
    const unsigned key = B[tid];
    const long o = (long)row * K + tid;
    shell[o] = (int32_t)(key >> 11);
    self_idx[o] = il;
    nbr_idx[o] = (int32_t)(key & 2047u);
    if (dist) dist[o] = __longlong_as_double((long long)A[tid]);
  }
}

// one workgroup per crystal: failure bits -> status (too few neighbours wins over a limit: it is a statement about the
// crystal, not about this kernel), and the rows of a crystal that was not built are zero-filled
__global__ __launch_bounds__(NB_THREADS) void nb_finalize_kernel(const int32_t* __restrict__ atom_ptr, int N, int K,
                                                                 int32_t* __restrict__ shell, int32_t* __restrict__ self_idx,
                                                                 int32_t* __restrict__ nbr_idx, double* __restrict__ dist,
                                                                 int32_t* __restrict__ status, int32_t* __restrict__ passes) {
  const int g = blockIdx.x, tid = threadIdx.x;
  const int bits = status[g];
  if (bits == 0) return;
  __syncthreads();
  if (tid == 0) status[g] = (bits & NB_FAIL_FEW) ? 1 : 2;
  const long a0 = atom_ptr[g], a1 = atom_ptr[g + 1];
  if (a0 < 0 || a1 > (long)N || a1 <= a0) return;
  for (long o = a0 * K + tid; o < a1 * K; o += NB_THREADS) {
    shell[o] = 0;
    self_idx[o] = 0;
    nbr_idx[o] = 0;
    if (dist) dist[o] = 0.0;
  }
  (void)passes;
}

static int nb_launch(const double* lattice, const double* frac, const int32_t* atom_ptr, int32_t G, int32_t N, int32_t K,
                     double radius, int32_t cap, double first_radius, int32_t* shell, int32_t* self_idx, int32_t* nbr_idx,
                     double* dist, int32_t* status, int32_t* passes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CGAT_CHECK_ARG(G >= 0 && N >= 0, "neighbor_tables: negative sizes");
  CGAT_CHECK_ARG(K >= 1 && K <= 64, "neighbor_tables: K = %d outside 1..64", (int)K);
  CGAT_CHECK_ARG(radius > 0.0 && radius < 1e300, "neighbor_tables: radius must be positive and finite");
  CGAT_CHECK_ARG(cap >= K && cap <= NB_CAP, "neighbor_tables: candidate capacity outside K..%d", NB_CAP);
  CGAT_CHECK_ARG(first_radius >= 0.0 && first_radius < 1e300, "neighbor_tables: bad first working radius");
  CGAT_CHECK_ARG((long)N * K < 2147483647L, "neighbor_tables: N * K needs 32-bit row offsets");
  if (G == 0) {
    CGAT_CHECK_ARG(N == 0, "neighbor_tables: atoms without crystals");
    return CGAT_OK;
  }
  CGAT_CHECK_ARG(lattice && atom_ptr && status, "neighbor_tables: null lattice / atom_ptr / status");
  CGAT_CHECK_ARG(N == 0 || (frac && shell && self_idx && nbr_idx), "neighbor_tables: null coordinates or tables");
  CGAT_PROF("neighbor_tables", s);
  CGAT_HIP(hipMemsetAsync(status, 0, (size_t)G * sizeof(int32_t), s));
  if (N > 0) {
    hipLaunchKernelGGL(nb_rows_kernel, dim3(N), dim3(NB_THREADS), 0, s, lattice, frac, atom_ptr, (int)G, (int)N, (int)K, radius,
                       (int)cap, first_radius, shell, self_idx, nbr_idx, dist, status, passes);
    CGAT_LAUNCH_CHECK();
    hipLaunchKernelGGL(nb_finalize_kernel, dim3(G), dim3(NB_THREADS), 0, s, atom_ptr, (int)N, (int)K, shell, self_idx, nbr_idx,
                       dist, status, passes);
    CGAT_LAUNCH_CHECK();
  }
  return CGAT_OK;
}

extern "C" int cgat_neighbor_tables(const double* lattice, const double* frac, const int32_t* atom_ptr, int32_t G, int32_t N,
                                    int32_t K, double radius, int32_t* shell, int32_t* self_idx, int32_t* nbr_idx,
                                    double* dist, int32_t* status, int32_t* passes, void* stream) {
  return nb_launch(lattice, frac, atom_ptr, G, N, K, radius, NB_CAP, 0.0, shell, self_idx, nbr_idx, dist, status, passes,
                   stream);
}

extern "C" int cgat_debug_neighbor_tables(const double* lattice, const double* frac, const int32_t* atom_ptr, int32_t G,
                                          int32_t N, int32_t K, double radius, int32_t cap, double first_radius,
                                          int32_t* shell, int32_t* self_idx, int32_t* nbr_idx, double* dist, int32_t* status,
                                          int32_t* passes, void* stream) {
  return nb_launch(lattice, frac, atom_ptr, G, N, K, radius, cap, first_radius, shell, self_idx, nbr_idx, dist, status,
                   passes, stream);
}
