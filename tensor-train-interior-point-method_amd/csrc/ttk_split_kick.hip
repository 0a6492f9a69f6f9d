// The truncate-and-kick split of a two-site local solve in ONE launch of ONE workgroup
// (`ttk_split_kick`): `_add_kick_rank` / `_add_kick_rank_rev` (src/tt_als.py:1041-1053) as the tail of
// `_step_size_local_solve` (:1023-1037) applies them to the truncation SVD's factors, and
// `add_kick_rank` (cy_src/tt_ops_cy.pyx:557-578) with S absent.
//
//   stage    cat = [U[:, :r] | G] (rev 0), or J cat^T J for cat = [U[:, :r]^T ; G] (rev 1: the transpose with
//            rows and columns reversed, J the anti-identity), column-major in LDS;
//   factor   Householder QR in place (LAPACK's sign convention, m < n handled), Q formed beside it;
//   store    the orthonormal factor, and the product of R[:, :r] (rev 0) or Rm[:r] (rev 1) with
//            diag(S[:r]) Vt[:r], which is read from global memory.
//
// The rank r is the host's decision on the singular values it has read; q = min(m, r + r_add) is host
// arithmetic; the kernel decides nothing and nothing is read back.  The one workgroup runs through
// bounded loops and workgroup barriers only.  Every product sums k ascending in one fma chain per
// output element and every reduction is a fixed wave tree: two calls on the same input give the same
// bits.
#include <hip/hip_runtime.h>

#include "ttk_common.h"
#include "ttk_internal.h"
#include "ttk_tt_gemm.h"

namespace {

struct SkPlan {
  int rev, a, b, p, r, r_add;
  int m, n, q;       // the factored matrix (m x n) and its rank bound
  int nt;
  int oY, oQ, oT;    // LDS regions (offsets in doubles, all even)
};

// Validates the extents and lays out LDS.  Returns the bytes of dynamic LDS, -1 when the working set
// does not fit one workgroup, -2 on invalid arguments.
int64_t sk_plan(int rev, int a, int b, int p, int r, int r_add, SkPlan *s) {
  if ((rev != 0 && rev != 1) || a < 1 || b < 1 || p < 1 || r < 1 || r_add < 1 || r > p) return -2;
  if (a > TT_CAP || b > TT_CAP || p > TT_CAP || r_add > TT_CAP) return -1;
  const int64_t m = rev ? b : a, n = (int64_t)r + r_add, q = m < n ? m : n;
  TtLayout L;
  const int64_t zY = L.mul(m, n), zQ = L.mul(m, q);
  s->oY = L.take(zY), s->oQ = L.take(zQ), s->oT = L.take(q);
  if (L.over || L.words * 8 > TT_LDS_MAX) return -1;
  s->rev = rev, s->a = a, s->b = b, s->p = p, s->r = r, s->r_add = r_add;
  s->m = (int)m, s->n = (int)n, s->q = (int)q;
  s->nt = tt_threads(zY, 1);
  return L.words * 8;
}

__global__ __launch_bounds__(1024) void split_kick_kernel(const SkPlan s, const double *__restrict__ U,
                                                          const double *__restrict__ S,
                                                          const double *__restrict__ Vt,
                                                          const double *__restrict__ G, double *__restrict__ s1,
                                                          double *__restrict__ s2) {
  extern __shared__ __attribute__((aligned(16))) double sk_lds[];
  double *Y = sk_lds + s.oY, *Qc = sk_lds + s.oQ, *tau = sk_lds + s.oT;
  const int m = s.m, n = s.n, q = s.q, r = s.r, p = s.p;
  // ---- stage: Y (m x n, column-major).  rev 0: column c is U[:, c] or G[:, c - r].  rev 1: column c is
  // row n-1-c of [U[:, :r]^T ; G] read backwards, Y = J cat^T J: its QR is LAPACK's dgerqf of cat, reflector
  // for reflector (the last entry of a row is the pivot), so Rm and Q come out in scipy.linalg.rq's gauge.
  for (int e = threadIdx.x; e < m * n; e += blockDim.x) {
    const int c = e / m, i = e - c * m;
    double v;
    if (!s.rev) {
      v = c < r ? U[i * p + c] : G[i * s.r_add + (c - r)];
    } else {
      const int row = n - 1 - c;
      const int col = m - 1 - i;
      v = row < r ? U[col * p + row] : G[(row - r) * m + col];
    }
    Y[e] = v;
  }
  __syncthreads();
  ro_householder(Y, m, n, tau);
  ro_form_q(Y, tau, m, q, Qc);
  // the upper trapezoid of Y is R (q x n): R(i, c) = Y[c m + i] for i <= c
  if (!s.rev) {
    // s1 = Q (a x q); s2 (q x b) = R[:, :r] (diag(S[:r]) Vt[:r])
    for (int e = threadIdx.x; e < m * q; e += blockDim.x) {
      const int i = e / q, c = e - i * q;
      s1[e] = Qc[c * m + i];
    }
    const int b = s.b;
    for (int e = threadIdx.x; e < q * b; e += blockDim.x) {
      const int i = e / b, j = e - i * b;
      double acc = 0.0;
      for (int k = i; k < r; ++k) acc = fma(Y[k * m + i], S ? S[k] * Vt[k * b + j] : Vt[k * b + j], acc);
      s2[e] = acc;
    }
  } else {
    // J cat^T J = Qt Rt gives cat = (J Rt^T J) (J Qt^T J): Rm(k, j) = R(q-1-j, n-1-k), Q(i, j) = Qt(m-1-j, q-1-i)
    // s1 (a x q) = (diag(S[:r]) Vt[:r])^T Rm[:r]; s2 = Q (q x b)
    const int a = s.a;
    for (int e = threadIdx.x; e < a * q; e += blockDim.x) {
      const int i = e / q, j = e - i * q, row = q - 1 - j;
      double acc = 0.0;
      for (int k = 0; k < r; ++k) {
        const int c = n - 1 - k;
        if (row > c) continue;  // below R's diagonal
        acc = fma(S ? S[k] * Vt[k * a + i] : Vt[k * a + i], Y[c * m + row], acc);
      }
      s1[e] = acc;
    }
    for (int e = threadIdx.x; e < q * m; e += blockDim.x) {
      const int i = e / m, j = e - i * m;
      s2[e] = Qc[(q - 1 - i) * m + (m - 1 - j)];
    }
  }
}

}  // namespace

extern "C" {

int64_t ttk_split_kick_lds(int rev, int a, int b, int p, int r, int r_add, int64_t *q_out) {
  SkPlan s;
  const int64_t bytes = sk_plan(rev, a, b, p, r, r_add, &s);
  if (bytes < 0) return -1;
  if (q_out) *q_out = s.q;
  return bytes;
}

int ttk_split_kick(ttk_ctx ctx, int rev, int a, int b, int p, int r, int r_add, const double *U, const double *S,
                   const double *Vt, const double *G, double *s1, double *s2) {
  ttk::CtxScope scope(ctx);
  SkPlan s;
  int64_t shm = (U && Vt && G && s1 && s2) ? sk_plan(rev, a, b, p, r, r_add, &s) : -2;
  if (shm >= 0 && S && p > (a < b ? a : b)) shm = -2;
  if (const int e = tt_plan_status(
          shm, "ttk_split_kick: bad arguments (rev 0 or 1, every extent >= 1, r <= p, p <= min(a, b) with S, no null "
               "pointer but S)",
          "ttk_split_kick: the concatenated matrix does not fit one workgroup's LDS (ttk_split_kick_lds)"))
    return e;
  tt_lds_attr(split_kick_kernel, shm);
  hipLaunchKernelGGL(split_kick_kernel, dim3(1), dim3(s.nt), (size_t)shm, ttk::ctx().stream, s, U, S, Vt, G, s1, s2);
  TTK_LAUNCH_CHECK();
  return TTK_OK;
}

}  // extern "C"
