// What the one-workgroup TT rounding kernels (ttk_randorth.hip, ttk_nystroem.hip, ttk_retract.hip) and the
// one-workgroup splits of a local solve (ttk_split_kick.hip, ttk_trunc_kick.hip) share:
//   device   products and loads, the right-to-left sketch step, the Householder QR, the one-sided
//            Jacobi round and the Jacobi SVD built on it, the kept rank of a truncation;
//   host     the planners' constants, extents check, saturating sizes and region allocator, and the
//            entry points' scratch block, LDS attribute and plan-status mapping.
// Each .hip file keeps its plan struct, its region sizes and its kernels' phase structure.
// The summation order is part of the contract: one ascending-k fma chain per output element.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "ttk_common.h"
#include "ttk_internal.h"

// The team: every helper below exists in two forms.  The one with a trailing (tid, nt) works with nt threads, the
// caller's thread being number tid of them; the one without is the whole workgroup, (threadIdx.x, blockDim.x).
// nt is a multiple of 64 and uniform.  A workgroup launched wider than its team (the batched rounding,
// ttk_retract.hip) passes TT_IDLE as the tid of its surplus waves: every loop over elements, columns, pairs
// or rows is then empty, every `tid == 0` and `wid == ...` test false, and such a thread only follows the
// uniform control flow to the barriers.  Which thread owns an element and how a reduction is ordered depend on
// nt alone, never on blockDim.x, so a team gives the same bits in a wider workgroup.
constexpr int TT_IDLE = 1 << 30;  // above every element count (those stay below 2^31 / 2) and, >> 6, every wave id

// C(i, j) = sum_k a(i, k) b(k, j), k ascending in one fma chain from 0; element e = i N + j goes to
// thread e mod nt.
template <class FA, class FB, class FC>
__device__ __forceinline__ void ro_gemm(int M, int N, int K, FA a, FB b, FC store, int tid, int nt) {
  for (int e = tid; e < M * N; e += nt) {
    const int i = e / N, j = e - i * N;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = fma(a(i, k), b(k, j), acc);
    store(i, j, acc);
  }
}
template <class FA, class FB, class FC>
__device__ __forceinline__ void ro_gemm(int M, int N, int K, FA a, FB b, FC store) {
  ro_gemm(M, N, K, a, b, store, threadIdx.x, blockDim.x);
}

__device__ __forceinline__ void ro_load(double *dst, const double *src, int n, int tid, int nt) {
  for (int e = tid; e < n; e += nt) dst[e] = src[e];
}
__device__ __forceinline__ void ro_load(double *dst, const double *src, int n) {
  ro_load(dst, src, n, threadIdx.x, blockDim.x);
}

__host__ __device__ inline int64_t tt_even(int64_t v) { return (v + 1) & ~(int64_t)1; }  // 16-byte aligned regions

// One step of the right-to-left sketch chain, W_k (rk x sk) = unfold(A_k W_{k+1}) unfold(B_k)^T, with
// A_k (rk, n, r1) at `core`, B_k (sk, n, s1) at `sketch` and W_{k+1} (r1 x s1) in W on entry: loads
// both cores into C and Z, forms T = A_k W_{k+1} (rk n x s1) in Y, then W_k into W and into wk.
// direct: the last core meets its sketch core as it lies (T = A_k, r1 == s1; W and Y are not read).
// Ends with a barrier.
__device__ __forceinline__ void tt_sketch_step(const double *core, const double *sketch, int rk, int n, int r1, int sk,
                                               int s1, bool direct, double *C, double *Z, double *Y, double *W,
                                               double *wk) {
  ro_load(C, core, rk * n * r1);
  ro_load(Z, sketch, sk * n * s1);
  __syncthreads();
  const double *T = C;
  if (!direct) {
    ro_gemm(rk * n, s1, r1, [&](int i, int c) { return C[i * r1 + c]; }, [&](int c, int j) { return W[c * s1 + j]; },
            [&](int i, int j, double v) { Y[i * s1 + j] = v; });
    __syncthreads();
    T = Y;
  }
  const int K = n * s1;
  ro_gemm(rk, sk, K, [&](int i, int c) { return T[i * K + c]; }, [&](int c, int j) { return Z[j * K + c]; },
          [&](int i, int j, double v) {
            W[i * sk + j] = v;
            wk[i * sk + j] = v;
          });
  __syncthreads();
}

namespace {

constexpr int NY_SWEEPS = 30;                // hard cap of the Jacobi sweeps (they converge in under 10)
constexpr int NY_FLAGS = 16;                 // doubles that hold the NY_SWEEPS per-sweep rotation flags
constexpr double NY_EPS = 2.220446049250313e-16;

// Householder QR of Y (m x n, column-major, in LDS) in place, any m and n: k = min(m, n) reflectors
// v_j = [1; Y[j+1:, j]] with tau[j], R in the upper trapezoid.  LAPACK's sign convention (dlarfg):
// beta = -sign(alpha) ||x||, tau = (beta - alpha) / beta, and a column that is zero below the
// diagonal gives tau = 0 (H = I).  Every wave forms reflector j itself (the same wave-tree sum of the
// same lane partials, so the same bits in every wave) and applies it to the columns it owns: one
// workgroup barrier per column.  Ends with a barrier.
__device__ void ro_householder(double *Y, int m, int n, double *tau, int tid, int nt) {
  const int lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  const int k = m < n ? m : n;
  for (int j = 0; j < k; ++j) {
    double *wj = Y + j * m;
    double part = 0.0;
    for (int i = j + 1 + lane; i < m; i += 64) part = fma(wj[i], wj[i], part);
    const double s2 = ttk::wave_sum(part);
    const double alpha = wj[j];
    double tj, sc, beta;
    if (s2 == 0.0) {
      tj = 0.0;
      beta = alpha;
      sc = 0.0;
    } else {
      const double nrm = sqrt(alpha * alpha + s2);
      beta = (alpha >= 0.0) ? -nrm : nrm;
      tj = (beta - alpha) / beta;
      sc = 1.0 / (alpha - beta);
    }
    if (tj != 0.0) {
      for (int c = j + 1 + wid; c < n; c += nw) {
        double *wc = Y + c * m;
        double dp = (lane == 0) ? wc[j] : 0.0;
        for (int i = j + 1 + lane; i < m; i += 64) dp = fma(wj[i] * sc, wc[i], dp);
        const double dd = ttk::wave_sum(dp) * tj;
        if (lane == 0) wc[j] -= dd;
        for (int i = j + 1 + lane; i < m; i += 64) wc[i] -= dd * (wj[i] * sc);
      }
    }
    __syncthreads();
    if (wid == j % nw) {  // every wave has read column j; nobody reads it again before the loop ends
      for (int i = j + 1 + lane; i < m; i += 64) wj[i] *= sc;
      if (lane == 0) {
        wj[j] = beta;
        tau[j] = tj;
      }
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void ro_householder(double *Y, int m, int n, double *tau) {
  ro_householder(Y, m, n, tau, threadIdx.x, blockDim.x);
}

// Qc (m x k, column-major, in LDS) = H_0 ... H_{k-1} [I_k; 0] from the reflectors ro_householder left
// in Y.  Column c only meets the reflectors j = c, c-1, ..., 0, so a wave takes whole columns through
// all their reflectors with no workgroup barrier in between.  Ends with a barrier.
__device__ void ro_form_q(const double *Y, const double *tau, int m, int k, double *Qc, int tid, int nt) {
  const int lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  for (int e = tid; e < m * k; e += nt) {
    const int c = e / m, i = e - c * m;
    Qc[e] = (i == c) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int c = wid; c < k; c += nw) {
    double *qc = Qc + c * m;
    for (int j = c; j >= 0; --j) {
      const double tj = tau[j];
      if (tj == 0.0) continue;
      const double *v = Y + j * m;
      double dp = (lane == 0) ? qc[j] : 0.0;
      for (int i = j + 1 + lane; i < m; i += 64) dp = fma(v[i], qc[i], dp);
      const double dd = ttk::wave_sum(dp) * tj;
      if (lane == 0) qc[j] -= dd;
      for (int i = j + 1 + lane; i < m; i += 64) qc[i] -= dd * v[i];
      __threadfence_block();  // one wave's LDS accesses stay in program order behind the fence
    }
  }
  __syncthreads();
}
__device__ __forceinline__ void ro_form_q(const double *Y, const double *tau, int m, int k, double *Qc) {
  ro_form_q(Y, tau, m, k, Qc, threadIdx.x, blockDim.x);
}

// One sweep-round of the one-sided Jacobi on the rows of A (p x n) with the rotations accumulated in
// G (p x p): the round's disjoint pairs (circle method over m = p rounded up to even players, the
// last one fixed) go to the waves in turn.  A pair (i, j) is rotated when |<a_i, a_j>| exceeds
// tol ||a_i|| ||a_j||.  Returns after a workgroup barrier.
__device__ void ny_jacobi_round(double *A, double *G, int p, int n, int m, int round, double tol2, int *flag, int tid,
                                int nt) {
  const int lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  for (int t = wid; t < m / 2; t += nw) {
    int i = t == 0 ? m - 1 : (round + t) % (m - 1);
    int j = (round - t + (m - 1)) % (m - 1);
    if (i > j) {
      const int x = i;
      i = j, j = x;
    }
    if (j >= p) continue;  // the bye of an odd p
    double *ai = A + i * n, *aj = A + j * n;
    double pa = 0.0, pb = 0.0, pg = 0.0;
    for (int c = lane; c < n; c += 64) {
      const double x = ai[c], y = aj[c];
      pa = fma(x, x, pa);
      pb = fma(y, y, pb);
      pg = fma(x, y, pg);
    }
    const double al = ttk::wave_sum(pa), be = ttk::wave_sum(pb), ga = ttk::wave_sum(pg);
    if (!(ga * ga > tol2 * al * be)) continue;  // |ga| <= tol sqrt(al be): orthogonal already
    const double zeta = (be - al) / (2.0 * ga);
    const double tn = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double cs = 1.0 / sqrt(1.0 + tn * tn), sn = cs * tn;
    for (int c = lane; c < n; c += 64) {
      const double x = ai[c], y = aj[c];
      ai[c] = cs * x - sn * y;
      aj[c] = sn * x + cs * y;
    }
    double *gi = G + i * p, *gj = G + j * p;
    for (int c = lane; c < p; c += 64) {
      const double x = gi[c], y = gj[c];
      gi[c] = cs * x - sn * y;
      gj[c] = sn * x + cs * y;
    }
    if (lane == 0) *flag = 1;
  }
  __syncthreads();
}

// One-sided Jacobi SVD of the rows of A (p x n, in LDS; the caller gives whichever of its matrix and
// the transpose has fewer rows): on return A = diag(S) W^T with the rotations accumulated in G
// (p x p, G A_in = A_out), sv[j] = ||row j|| and perm[position] = row, descending (ties by index).
// sv holds 2 tt_even(p) doubles and NY_FLAGS more: the values, perm (returned) and the sweep flags.
// Contract: call it once A is written, with no barrier in between.  It sets G, perm and the flags
// (none of them A), waits at ONE barrier, which also publishes A, then runs at most NY_SWEEPS sweeps,
// the row norms and the sort.  Ends with a barrier.
__device__ int *tt_jacobi_svd(double *A, double *G, double *sv, int p, int n, int tid, int nt) {
  const int lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  int *perm = reinterpret_cast<int *>(sv + tt_even(p));
  int *flag = reinterpret_cast<int *>(sv + 2 * tt_even(p));
  for (int e = tid; e < p * p; e += nt) G[e] = (e / p == e % p) ? 1.0 : 0.0;
  for (int e = tid; e < NY_SWEEPS; e += nt) flag[e] = 0;
  for (int e = tid; e < p; e += nt) perm[e] = e;  // stays a valid index whatever the sort meets
  __syncthreads();
  const double tol = NY_EPS * (n > 16 ? (double)n : 16.0), tol2 = tol * tol;
  const int m = (p + 1) & ~1;
  for (int sweep = 0; sweep < NY_SWEEPS && p > 1; ++sweep) {
    for (int round = 0; round < m - 1; ++round) ny_jacobi_round(A, G, p, n, m, round, tol2, flag + sweep, tid, nt);
    if (flag[sweep] == 0) break;  // written before the round's barrier: every thread reads the same value
  }
  for (int j = wid; j < p; j += nw) {
    double part = 0.0;
    for (int c = lane; c < n; c += 64) part = fma(A[j * n + c], A[j * n + c], part);
    const double nrm = sqrt(ttk::wave_sum(part));
    if (lane == 0) sv[j] = nrm;
  }
  __syncthreads();
  for (int j = tid; j < p; j += nt) {
    int pos = 0;
    for (int i = 0; i < p; ++i) pos += (sv[i] > sv[j] || (sv[i] == sv[j] && i < j)) ? 1 : 0;
    perm[pos < p ? pos : p - 1] = j;  // a NaN compares false everywhere: stay in bounds
  }
  __syncthreads();
  return perm;
}
__device__ __forceinline__ int *tt_jacobi_svd(double *A, double *G, double *sv, int p, int n) {
  return tt_jacobi_svd(A, G, sv, p, n, threadIdx.x, blockDim.x);
}

// The kept rank of one truncation by the reference's rule (prune_singular_vals, cy_src/tt_ops_cy.pyx:161-177) on the
// pp singular values sv[perm[0]] >= ... : sc[j] = sum_{t >= j} sv[perm[t]]^2 summed from the smallest value
// upward (np.cumsum's order: rounded products, rounded sums), q = the first j with sc[j] < thr2 (0 if
// none), at least 1, and pp if sc[pp-1] > thr2; the all-zero spectrum gives 1.  *tail += sc[q] when q < pp
// and track.  The result is clamped to [1, pp] whatever the spectrum holds (a NaN compares false).
__device__ int rt_kept_rank(const double *sv, const int *perm, int pp, double thr2, bool track, double *tail) {
  double sc = 0.0;
  int q = 0;
  for (int j = pp - 1; j >= 0; --j) {
    const double s = sv[perm[j]];
    sc = __dadd_rn(sc, __dmul_rn(s, s));
    if (sc < thr2) q = j;
  }
  q = q < 1 ? 1 : q;
  const double last = sv[perm[pp - 1]];
  if (__dmul_rn(last, last) > thr2) q = pp;
  q = q > pp ? pp : q;
  if (track && q < pp) {
    sc = 0.0;
    for (int j = pp - 1; j >= q; --j) {
      const double s = sv[perm[j]];
      sc = __dadd_rn(sc, __dmul_rn(s, s));
    }
    *tail += sc;
  }
  return q;
}

// ---- host: planning
constexpr int TT_MAXD = 32;                 // cores per train (the plan travels as a kernel argument)
constexpr int64_t TT_LDS_MAX = 160 * 1024;  // bytes one workgroup may declare
constexpr int64_t TT_CAP = TT_LDS_MAX / 8;  // doubles: no single extent or product may pass the LDS capacity

// The planners' common checks on d middle extents and rank arrays of d + 1 entries: -2 unless d >= 2,
// no array is null and every entry is >= 1; then -1 for more than TT_MAXD cores or an entry above
// TT_CAP; else 0.  A planner adds its boundary rule to the -2 case before it passes a -1 on.
inline int tt_check_extents(int d, const int64_t *inner, std::initializer_list<const int64_t *> ranks) {
  if (d < 2 || !inner) return -2;
  for (const int64_t *r : ranks)
    if (!r) return -2;
  bool big = d > TT_MAXD;
  for (int k = 0; k <= d; ++k)
    for (const int64_t *r : ranks) {
      if (r[k] < 1) return -2;
      big |= r[k] > TT_CAP;
    }
  for (int k = 0; k < d; ++k) {
    if (inner[k] < 1) return -2;
    big |= inner[k] > TT_CAP;
  }
  return big ? -1 : 0;
}

// Sizes and offsets in doubles.  up: z = max(z, a b c) with the product saturating at TT_CAP + 1
// (factors <= TT_CAP: no overflow), which `over` remembers.  take: the next region of a block (LDS, or
// the call's scratch), regions back to back and rounded up to even; a plan has at most 4 TT_MAXD of
// them, none above TT_CAP + 2, so an offset fits an int.
struct TtLayout {
  bool over = false;
  int64_t words = 0;
  int64_t mul(int64_t a, int64_t b = 1, int64_t c = 1) {
    int64_t v = a * b;
    v = v > TT_CAP ? TT_CAP + 1 : v * c;
    if (v > TT_CAP) over = true, v = TT_CAP + 1;
    return v;
  }
  void up(int64_t &z, int64_t a, int64_t b = 1, int64_t c = 1) {
    const int64_t v = mul(a, b, c);
    z = v > z ? v : z;
  }
  int take(int64_t z) {
    const int at = (int)words;
    words += tt_even(z);
    return at;
  }
};

// small trains: fewer waves at each barrier; a Jacobi takes one wave per pair, up to 16 waves
inline int tt_threads(int64_t work, int64_t jacobi_rows) { return (work <= 2048 && jacobi_rows <= 8) ? 256 : 1024; }

// ---- host: the entry points
// the call's stream-ordered scratch block: allocated on the stream, freed on it when the call returns
struct TtScratch {
  hipStream_t st;
  void *p = nullptr;
  explicit TtScratch(hipStream_t s) : st(s) {}
  TtScratch(const TtScratch &) = delete;
  TtScratch &operator=(const TtScratch &) = delete;
  ~TtScratch() {
    if (p) (void)hipFreeAsync(p, st);
  }
  hipError_t alloc(int64_t words) { return hipMallocAsync(&p, (size_t)(words > 0 ? words : 2) * sizeof(double), st); }
  double *get() const { return static_cast<double *>(p); }
};

template <class K>
void tt_lds_attr(K kernel, int64_t shm) {
  if (shm > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)shm);
}

// a planner's result as the entry point's status: TTK_OK, or TTK_ERR_ARG with the message set
inline int tt_plan_status(int64_t shm, const char *bad_arguments, const char *does_not_fit) {
  if (shm >= 0) return TTK_OK;
  ttk::set_error("%s", shm == -2 ? bad_arguments : does_not_fit);
  return TTK_ERR_ARG;
}

}  // namespace
