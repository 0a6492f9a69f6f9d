// The whole tail of a two-site local solve of the step-size eigen-ALS in ONE launch of ONE workgroup
// (`ttk_trunc_kick`): normalise, truncation SVD, the rank decision, the kicked QR / RQ and the product with
// diag(S) Vt (`_step_size_local_solve`, src/tt_als.py:1022-1037, with `_add_kick_rank` /
// `_add_kick_rank_rev`, :1041-1053, and `prune_singular_vals`, cy_src/tt_ops_cy.pyx:161-177).
//
//   norm     ||M||_F by a fixed two-level tree (lane partials, wave tree, the waves' sums ascending);
//   stage    whichever of M / ||M|| and its transpose has fewer rows, row-major in LDS;
//   svd      one-sided Jacobi on its rows (tt_jacobi_svd): A = diag(S) W^T, the rotations in G;
//   rank     one thread: r = min(rt_kept_rank(S, trunc_tol^2), max_rank); one LDS word and one barrier publish it;
//   kick     cat = [U[:, :r] | G] (rev 0), or J cat^T J for cat = [U[:, :r]^T ; G] (rev 1), column-major in LDS,
//            Householder QR in place and Q beside it, as ttk_split_kick.hip does them;
//   store    the orthonormal factor, the product of the triangular factor with diag(S[:r]) Vt[:r], and info.
//
// rev = 1 factors M^T by indexing: no transposed copy is made.  U and diag(S) Vt are never formed: a column of
// U is a row of G or a row of A over its norm, a row of diag(S) Vt is the other one (ucol, svrow below).
// The rank is decided here and reaches the host only in info; the one workgroup runs through bounded loops
// (the Jacobi sweeps by NY_SWEEPS) and workgroup barriers only, waits for nobody and reads nothing back.
// Every product sums k ascending in one fma chain per output element and every reduction is a fixed tree: two
// calls on the same input give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ttk_common.h"
#include "ttk_internal.h"
#include "ttk_tt_gemm.h"

namespace {

struct TkPlan {
  int rev, a, b, r_add, unit, max_rank;
  int p, n;          // the Jacobi's matrix (p x n): M when a <= b, else its transpose
  int m;             // the rows of the concatenated matrix: a (rev 0) or b (rev 1)
  int nt;
  int oA, oG, oS, oY, oQ, oT, oW;  // LDS regions (offsets in doubles, all even)
  double thr2;       // trunc_tol^2
};

// Validates the extents and lays out LDS.  Returns the bytes of dynamic LDS, -1 when the working set
// does not fit one workgroup, -2 on invalid arguments.
int64_t tk_plan(int rev, int a, int b, int r_add, int max_rank, TkPlan *s, int64_t *qmax_out) {
  if ((rev != 0 && rev != 1) || a < 1 || b < 1 || r_add < 1 || max_rank < 1) return -2;
  if (a > TT_CAP || b > TT_CAP || r_add > TT_CAP) return -1;
  const int64_t p = a < b ? a : b, n = a < b ? b : a, m = rev ? b : a;
  const int64_t rmax = p < max_rank ? p : max_rank, nmax = rmax + r_add, qmax = m < nmax ? m : nmax;
  TtLayout L;
  const int64_t zA = L.mul(p, n), zG = L.mul(p, p), zY = L.mul(m, nmax), zQ = L.mul(m, qmax);
  s->oA = L.take(zA), s->oG = L.take(zG), s->oS = L.take(2 * tt_even(p) + NY_FLAGS);
  s->oY = L.take(zY), s->oQ = L.take(zQ), s->oT = L.take(qmax);
  s->oW = L.take(16 + 2);  // the waves' partial sums of ||M||^2, then the published rank
  if (L.over || L.words * 8 > TT_LDS_MAX) return -1;
  s->rev = rev, s->a = a, s->b = b, s->r_add = r_add, s->max_rank = max_rank;
  s->p = (int)p, s->n = (int)n, s->m = (int)m;
  s->nt = tt_threads(zA > zY ? zA : zY, p);
  if (qmax_out) *qmax_out = qmax;
  return L.words * 8;
}

__global__ __launch_bounds__(1024) void trunc_kick_kernel(const TkPlan s, const double *__restrict__ M,
                                                          const double *__restrict__ Gk, double *__restrict__ s1,
                                                          double *__restrict__ s2, double *__restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double tk_lds[];
  double *A = tk_lds + s.oA, *G = tk_lds + s.oG, *sv = tk_lds + s.oS, *Y = tk_lds + s.oY, *Qc = tk_lds + s.oQ;
  double *tau = tk_lds + s.oT, *red = tk_lds + s.oW;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  const int a = s.a, b = s.b, p = s.p, n = s.n, m = s.m, r_add = s.r_add;
  // ---- norm: thread t the elements t, t + nt, ... ascending; the wave tree; the waves' sums ascending
  double part = 0.0;
  for (int e = tid; e < a * b; e += nt) part = fma(M[e], M[e], part);
  part = ttk::wave_sum(part);
  if (lane == 0) red[wid] = part;
  __syncthreads();
  double tot = 0.0;
  for (int w = 0; w < nw; ++w) tot = __dadd_rn(tot, red[w]);
  const double nrm = sqrt(tot);
  const double scale = (s.unit && nrm != 0.0) ? 1.0 / nrm : 1.0;  // a zero matrix stays zero
  // ---- stage: A (p x n, row-major) = M scale when a <= b, else its transpose
  const bool rowsz = a <= b;
  for (int e = tid; e < a * b; e += nt) {
    const int i = e / b, j = e - i * b;
    A[rowsz ? e : j * a + i] = s.unit ? __dmul_rn(M[e], scale) : M[e];
  }
  const int *perm = tt_jacobi_svd(A, G, sv, p, n);
  // ---- rank: one thread decides, one barrier publishes: r is uniform and 1 <= r <= min(p, max_rank)
  if (tid == 0) {
    double tail = 0.0;
    int r0 = rt_kept_rank(sv, perm, p, s.thr2, false, &tail);
    red[16] = (double)(r0 < s.max_rank ? r0 : s.max_rank);
  }
  __syncthreads();
  const int r = (int)red[16], nn = r + r_add, q = m < nn ? m : nn;
  // M = U diag(S) Vt (rev 0) or M^T = U diag(S) Vt (rev 1).  With A_in = G^T diag(S) W^T after the Jacobi, U's
  // columns are G's rows when A_in is the factored matrix (rev 0 with M staged, rev 1 with M^T staged) and
  // diag(S) Vt's rows are A's; otherwise U's columns are A's rows over their norms and diag(S) Vt is diag(S) G.
  const bool fromG = rowsz != (s.rev != 0);
  auto ucol = [&](int t, int i) -> double {
    const int row = perm[t];
    if (fromG) return G[row * p + i];
    const double sg = sv[row];
    return sg > 0.0 ? A[row * n + i] / sg : 0.0;
  };
  auto svrow = [&](int t, int j) -> double {
    const int row = perm[t];
    return fromG ? A[row * n + j] : __dmul_rn(sv[row], G[row * p + j]);
  };
  // ---- kick: Y (m x nn, column-major) as split_kick_kernel stages it
  for (int e = tid; e < m * nn; e += nt) {
    const int c = e / m, i = e - c * m;
    double v;
    if (!s.rev) {
      v = c < r ? ucol(c, i) : Gk[i * r_add + (c - r)];
    } else {
      const int row = nn - 1 - c;
      const int col = m - 1 - i;
      v = row < r ? ucol(row, col) : Gk[(row - r) * m + col];
    }
    Y[e] = v;
  }
  __syncthreads();
  ro_householder(Y, m, nn, tau);
  ro_form_q(Y, tau, m, q, Qc);
  // the upper trapezoid of Y is R (q x nn): R(i, c) = Y[c m + i] for i <= c
  if (!s.rev) {
    // s1 = Q (a x q); s2 (q x b) = R[:, :r] (diag(S[:r]) Vt[:r])
    for (int e = tid; e < m * q; e += nt) {
      const int i = e / q, c = e - i * q;
      s1[e] = Qc[c * m + i];
    }
    for (int e = tid; e < q * b; e += nt) {
      const int i = e / b, j = e - i * b;
      double acc = 0.0;
      for (int k = i; k < r; ++k) acc = fma(Y[k * m + i], svrow(k, j), acc);
      s2[e] = acc;
    }
  } else {
    // J cat^T J = Qt Rt gives cat = (J Rt^T J) (J Qt^T J): Rm(k, j) = R(q-1-j, nn-1-k), Q(i, j) = Qt(m-1-j, q-1-i)
    // s1 (a x q) = (diag(S[:r]) Vt[:r])^T Rm[:r]; s2 = Q (q x b)
    for (int e = tid; e < a * q; e += nt) {
      const int i = e / q, j = e - i * q, row = q - 1 - j;
      double acc = 0.0;
      for (int k = 0; k < r; ++k) {
        const int c = nn - 1 - k;
        if (row > c) continue;  // below R's diagonal
        acc = fma(svrow(k, i), Y[c * m + row], acc);
      }
      s1[e] = acc;
    }
    for (int e = tid; e < q * m; e += nt) {
      const int i = e / m, j = e - i * m;
      s2[e] = Qc[(q - 1 - i) * m + (m - 1 - j)];
    }
  }
  // ---- info: r, q, the sweeps taken (negative at the cap), ||M||_F as found, S descending
  for (int t = tid; t < p; t += nt) info[4 + t] = sv[perm[t]];
  if (tid == 0) {
    const int *flag = reinterpret_cast<const int *>(sv + 2 * tt_even(p));
    int sw = 0;
    while (sw < NY_SWEEPS && flag[sw]) ++sw;
    info[0] = (double)r;
    info[1] = (double)q;
    info[2] = p > 1 ? (sw < NY_SWEEPS ? (double)(sw + 1) : -(double)NY_SWEEPS) : 0.0;
    info[3] = nrm;
  }
}

// Validates, plans and enqueues the one launch.  mapped == nullptr: info is the caller's device block.  Else info is
// the caller's host block (only tested for null here) and the kernel writes the context's host-coherent stage,
// whose host address goes to *mapped, for the caller to copy from once the stream has drained.
int tk_enqueue(int rev, int a, int b, int r_add, int unit, double trunc_tol, int max_rank, const double *M,
               const double *G, double *s1, double *s2, double *info, double **mapped) {
  TkPlan s;
  const bool ok = M && G && s1 && s2 && info && trunc_tol >= 0.0 && std::isfinite(trunc_tol);
  const int64_t shm = ok ? tk_plan(rev, a, b, r_add, max_rank, &s, nullptr) : -2;
  if (const int e = tt_plan_status(
          shm, "ttk_trunc_kick: bad arguments (rev 0 or 1, every extent >= 1, r_add >= 1, max_rank >= 1, trunc_tol "
               ">= 0 and finite, no null pointer)",
          "ttk_trunc_kick: the matrix, its rotations and the concatenated matrix do not fit one workgroup's LDS "
          "(ttk_trunc_kick_lds)"))
    return e;
  if (mapped) {
    *mapped = ttk::mapped_stage((size_t)(4 + s.p), &info);
    if (!*mapped) {
      ttk::set_error("ttk_trunc_kick_read: mapped allocation failed");
      return TTK_ERR_HIP;
    }
  }
  s.unit = unit != 0;
  s.thr2 = trunc_tol * trunc_tol;
  tt_lds_attr(trunc_kick_kernel, shm);
  hipLaunchKernelGGL(trunc_kick_kernel, dim3(1), dim3(s.nt), (size_t)shm, ttk::ctx().stream, s, M, G, s1, s2, info);
  TTK_LAUNCH_CHECK();
  return TTK_OK;
}

}  // namespace

extern "C" {

int64_t ttk_trunc_kick_lds(int rev, int a, int b, int r_add, int max_rank, int64_t *qmax_out) {
  TkPlan s;
  const int64_t bytes = tk_plan(rev, a, b, r_add, max_rank, &s, qmax_out);
  return bytes < 0 ? -1 : bytes;
}

int ttk_trunc_kick(ttk_ctx ctx, int rev, int a, int b, int r_add, int unit, double trunc_tol, int max_rank,
                   const double *M, const double *G, double *s1, double *s2, double *info) {
  ttk::CtxScope scope(ctx);
  return tk_enqueue(rev, a, b, r_add, unit, trunc_tol, max_rank, M, G, s1, s2, info, nullptr);
}

int ttk_trunc_kick_read(ttk_ctx ctx, int rev, int a, int b, int r_add, int unit, double trunc_tol, int max_rank,
                        const double *M, const double *G, double *s1, double *s2, double *info_host) {
  ttk::CtxScope scope(ctx);
  double *h = nullptr;
  if (const int e = tk_enqueue(rev, a, b, r_add, unit, trunc_tol, max_rank, M, G, s1, s2, info_host, &h)) return e;
  ttk::note_sync();
  TTK_HIP(hipStreamSynchronize(ttk::ctx().stream));
  std::memcpy(info_host, h, (size_t)(4 + (a < b ? a : b)) * sizeof(double));
  return TTK_OK;
}

}  // extern "C"
