// Randomised fixed-rank TT rounding in ONE launch of ONE workgroup (`ttk_rand_orth`): the
// randomise-then-orthogonalise sweep of `_tt_lr_random_orthogonalise` (src/tt_ops.py:89-101) with
// the sketch contractions of `tt_rl_contraction` (src/tt_ops.py:51-58).
//
//   phase A (right to left)  W_k = unfold(A_k W_{k+1}) unfold(B_k)^T for k = d-1 .. 1, each written to
//                            the call's scratch block (A the train, B the sketch);
//   phase B (left to right)  Y = Z W_{i+1}, Householder QR of Y, core i <- Q, carried core
//                            Z <- (Q^T Z) core_{i+1}, which stays in LDS until it is core i+1's turn.
//
// No SVD, no truncation decision, no host read: every extent follows from the host-side rank rule
// q_0 = r_0, q_{i+1} = min(q_i n_i, l_{i+1}) before the launch.  The one workgroup runs alone through
// bounded loops and workgroup barriers only (no inter-workgroup hand-off, no spin wait, no atomics),
// so it does not depend on co-residency.  Every product sums k ascending in one fma chain per output
// element and every reduction is a fixed wave tree, so two calls on the same input give the same bits.
//
// The products are VALU fma chains: at the extents this kernel accepts (a whole TT in 160 KiB of
// LDS: bond ranks of a few tens at most) a 16x16x4 fp64 MFMA tile would be mostly padding, and the
// sweep is bound by its barriers (one per Householder column), not by its FLOPs.
#include <hip/hip_runtime.h>

#include "ttk_common.h"
#include "ttk_internal.h"
#include "ttk_tt_gemm.h"

namespace {

struct RoPlan {
  int d, nt;
  int inner[TT_MAXD];   // middle extents; the last one carries the trailing boundary rank
  int r[TT_MAXD + 1];   // train bond ranks   (r[d] = 1 after folding the boundary into inner)
  int s[TT_MAXD + 1];   // sketch bond ranks  (s[d] = 1 likewise)
  int q[TT_MAXD + 1];   // output bond ranks
  int woff[TT_MAXD];    // W_k's offset in the scratch block (doubles), k = 1 .. d-1
  int oZ, oC, oY, oQ, oM, oW, oT;  // LDS regions (offsets in doubles, all even: 16-byte aligned)
  const double *core[TT_MAXD];
  const double *sk[TT_MAXD];
  double *out[TT_MAXD];
};

// Validates the extents, applies the rank rule and lays out LDS and scratch.  Returns the bytes of
// dynamic LDS, -1 when the train does not fit one workgroup (or has more than TT_MAXD cores), -2 on
// invalid arguments.  *wwords: doubles of scratch for W_1 .. W_{d-1}.
int64_t ro_plan(int d, const int64_t *inner, const int64_t *ranks, const int64_t *sranks, RoPlan *p, int64_t *wwords) {
  const int chk = tt_check_extents(d, inner, {ranks, sranks});
  // the last cores are contracted over (n_{d-1}, r_d) together
  if (chk == -2 || ranks[d] != sranks[d]) return -2;
  if (chk) return chk;
  int64_t n[TT_MAXD], r[TT_MAXD + 1], s[TT_MAXD + 1], q[TT_MAXD + 1];
  for (int k = 0; k < d; ++k) n[k] = inner[k];
  for (int k = 0; k <= d; ++k) r[k] = ranks[k], s[k] = sranks[k];
  n[d - 1] *= r[d];
  r[d] = s[d] = 1;
  if (n[d - 1] > TT_CAP) return -1;
  q[0] = r[0];
  for (int i = 0; i + 1 < d; ++i) {
    const int64_t m = q[i] * n[i];  // <= TT_CAP * TT_CAP: no overflow
    if (m > TT_CAP) return -1;
    q[i + 1] = m < s[i + 1] ? m : s[i + 1];
  }
  q[d] = 1;
  TtLayout L, S;  // LDS, scratch
  int64_t zZ = 2, zC = 2, zY = 2, zQ = 2, zM = 2, zW = 2, zT = 2;
  for (int i = 0; i < d; ++i) L.up(zZ, q[i], n[i], r[i + 1]);        // carried core
  for (int k = 1; k < d; ++k) {
    L.up(zZ, s[k], n[k], s[k + 1]);                                   // sketch core (phase A)
    L.up(zC, r[k], n[k], r[k + 1]);                                   // train core
    L.up(zY, r[k], n[k], s[k + 1]);                                   // A_k W_{k+1}
    L.up(zW, r[k], s[k]);
    p->woff[k] = S.take(L.mul(r[k], s[k]));
  }
  for (int i = 0; i + 1 < d; ++i) {
    L.up(zY, q[i], n[i], s[i + 1]);                                   // Y
    L.up(zQ, q[i], n[i], q[i + 1]);                                   // Q
    L.up(zM, q[i + 1], r[i + 1]);                                     // Q^T Z
    L.up(zT, q[i + 1]);                                               // tau
  }
  p->oZ = L.take(zZ), p->oC = L.take(zC), p->oY = L.take(zY), p->oQ = L.take(zQ), p->oM = L.take(zM);
  p->oW = L.take(zW), p->oT = L.take(zT);
  if (L.over || L.words * 8 > TT_LDS_MAX) return -1;
  *wwords = S.words;
  p->d = d;
  p->nt = tt_threads(zY > zZ ? zY : zZ, 1);
  for (int k = 0; k < d; ++k) p->inner[k] = (int)n[k];
  for (int k = 0; k <= d; ++k) p->r[k] = (int)r[k], p->s[k] = (int)s[k], p->q[k] = (int)q[k];
  return L.words * 8;
}

__global__ __launch_bounds__(1024) void rand_orth_kernel(const RoPlan p, double *wscr) {
  extern __shared__ __attribute__((aligned(16))) double ro_lds[];
  double *Z = ro_lds + p.oZ, *C = ro_lds + p.oC, *Y = ro_lds + p.oY, *Qc = ro_lds + p.oQ, *Mq = ro_lds + p.oM,
         *W = ro_lds + p.oW, *tau = ro_lds + p.oT;
  const int d = p.d;
  // ---- phase A: W_d = [1]; W_k = unfold(A_k W_{k+1}) unfold(B_k)^T, k = d-1 .. 1
  if (threadIdx.x == 0) W[0] = 1.0;
  for (int k = d - 1; k >= 1; --k)  // the sketch core borrows the carried core's region
    tt_sketch_step(p.core[k], p.sk[k], p.r[k], p.inner[k], p.r[k + 1], p.s[k], p.s[k + 1], false, C, Z, Y, W,
                   wscr + p.woff[k]);
  // ---- phase B: left to right; Z holds the current core (q_i, n_i, r_{i+1})
  ro_load(Z, p.core[0], p.q[0] * p.inner[0] * p.r[1]);
  for (int i = 0; i + 1 < d; ++i) {
    const int m = p.q[i] * p.inner[i], R = p.r[i + 1], l = p.s[i + 1], k = p.q[i + 1];
    const int rest = p.inner[i + 1] * p.r[i + 2];
    ro_load(W, wscr + p.woff[i + 1], R * l);
    ro_load(C, p.core[i + 1], R * rest);
    __syncthreads();
    // Y (m x l, column-major) = Z (m x R) W_{i+1} (R x l)
    ro_gemm(m, l, R, [&](int a, int c) { return Z[a * R + c]; }, [&](int c, int j) { return W[c * l + j]; },
            [&](int a, int j, double v) { Y[j * m + a] = v; });
    __syncthreads();
    ro_householder(Y, m, l, tau);
    ro_form_q(Y, tau, m, k, Qc);
    // core i <- Q (m x k, row-major: (q_i, n_i, k)); Mq (k x R) = Q^T Z
    double *oi = p.out[i];
    for (int e = threadIdx.x; e < m * k; e += blockDim.x) {
      const int a = e / k, c = e - a * k;
      oi[e] = Qc[c * m + a];
    }
    ro_gemm(k, R, m, [&](int a, int c) { return Qc[a * m + c]; }, [&](int c, int j) { return Z[c * R + j]; },
            [&](int a, int j, double v) { Mq[a * R + j] = v; });
    __syncthreads();
    // Z (k x rest) <- Mq (k x R) core_{i+1} (R x rest)
    ro_gemm(k, rest, R, [&](int a, int c) { return Mq[a * R + c]; }, [&](int c, int j) { return C[c * rest + j]; },
            [&](int a, int j, double v) { Z[a * rest + j] = v; });
    __syncthreads();
  }
  double *ol = p.out[d - 1];
  for (int e = threadIdx.x; e < p.q[d - 1] * p.inner[d - 1]; e += blockDim.x) ol[e] = Z[e];
}

}  // namespace

extern "C" {

int64_t ttk_rand_orth_lds(int d, const int64_t *inner, const int64_t *ranks, const int64_t *sketch_ranks) {
  RoPlan p;
  int64_t wwords;
  const int64_t b = ro_plan(d, inner, ranks, sketch_ranks, &p, &wwords);
  return b < 0 ? -1 : b;
}

int ttk_rand_orth(ttk_ctx ctx, int d, const double *const *cores, const int64_t *inner, const int64_t *ranks,
                  const double *const *sketch, const int64_t *sketch_ranks, double *const *out, int64_t *out_ranks) {
  ttk::CtxScope scope(ctx);
  RoPlan p;
  int64_t wwords = 0;
  const int64_t shm = (cores && sketch && out && out_ranks) ? ro_plan(d, inner, ranks, sketch_ranks, &p, &wwords) : -2;
  if (const int e = tt_plan_status(
          shm, "ttk_rand_orth: bad arguments (d >= 2, every rank and extent >= 1, equal trailing ranks)",
          "ttk_rand_orth: the train does not fit one workgroup's LDS (ttk_rand_orth_lds)"))
    return e;
  for (int k = 0; k < d; ++k) {
    if (!cores[k] || !out[k] || (k > 0 && !sketch[k])) {
      ttk::set_error("ttk_rand_orth: null core %d", k);
      return TTK_ERR_ARG;
    }
    p.core[k] = cores[k];
    p.sk[k] = sketch[k];
    p.out[k] = out[k];
  }
  TtScratch w(ttk::ctx().stream);  // W_1 .. W_{d-1}
  TTK_HIP(w.alloc(wwords));
  tt_lds_attr(rand_orth_kernel, shm);
  hipLaunchKernelGGL(rand_orth_kernel, dim3(1), dim3(p.nt), (size_t)shm, w.st, p, w.get());
  TTK_LAUNCH_CHECK();
  for (int k = 0; k < d; ++k) out_ranks[k] = p.q[k];
  out_ranks[d] = ranks[d];
  return TTK_OK;
}

}  // extern "C"
