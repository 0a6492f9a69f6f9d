// Generalised Nystroem TT rounding in THREE launches of independent workgroups (`ttk_nystroem`):
// `_tt_generalised_nystroem` (src/tt_ops.py:273-292) with the sketch contractions of
// `tt_lr_contraction` / `tt_rl_contraction` (src/tt_ops.py:51-65).
//
//   launch 1, grid 2     workgroup 0 walks right to left, W_R[k] = unfold(A_k W_R[k+1]) unfold(B_k)^T
//                        (A the train, B the right sketch: ttk_rand_orth's phase A); workgroup 1 walks
//                        left to right, W_L[k+1] = unfold(G_k)^T unfold(W_L[k] A_k) (G the left sketch),
//                        directly on the cores as they lie (no mirrored copies);
//   launch 2, grid d-1   workgroup k-1 forms P = W_L[k] W_R[k] in LDS, runs a one-sided Jacobi SVD on
//                        it and writes L_k = W_R V diag(1/sqrt(S)) and R_k = diag(1/sqrt(S)) U^T W_L;
//   launch 3, grid d     workgroup k writes out_k = R_k core_k L_{k+1} (no R on core 0, no L on the last).
//
// W_L, W_R, L and R live in one stream-ordered scratch block per call; stream order is the only
// dependency between the launches.  No truncation decision and no host read: the output ranks are
// min(lranks[k], rranks[k]), host arithmetic.  Inside a launch no workgroup waits on another:
// workgroup barriers only, no spin wait, no atomics, every loop bounded (the Jacobi sweeps by
// NY_SWEEPS), so nothing depends on co-residency.  Every product sums k ascending in one fma chain
// per output element and every reduction is a fixed wave tree; the Jacobi pairs follow one fixed
// round-robin order.  Two calls on the same input therefore give the same bits.
//
// The Jacobi rotates the rows of P when lranks[k] <= rranks[k] and the rows of P^T otherwise, so it
// always works on p = min(l, s) rows of length max(l, s): G P = diag(S) V^T with G = U^T the
// accumulated rotations (or G P^T = diag(S) U^T with G = V^T).  One wave takes one pair; the p/2
// disjoint pairs of a round run in parallel, one barrier per round.  Singular values are sorted
// descending (ties by row index).  Like the reference, nothing guards a zero singular value.
//
// The products are VALU fma chains: at the extents this call accepts (each core with its factors in
// 160 KiB of LDS, bond ranks of a few tens at most) a 16x16x4 fp64 MFMA tile would be mostly
// padding, and the three launches are bound by their latency, not by their FLOPs.
#include <hip/hip_runtime.h>

#include "ttk_common.h"
#include "ttk_internal.h"
#include "ttk_tt_gemm.h"

namespace {

struct NyPlan {
  int d, nt1, nt2;      // threads of launches 1 and 2
  int n[TT_MAXD];       // middle extents
  int r[TT_MAXD + 1];   // train bond ranks
  int l[TT_MAXD + 1];   // left sketch bond ranks
  int s[TT_MAXD + 1];   // right sketch bond ranks
  int q[TT_MAXD + 1];   // output bond ranks
  int owl[TT_MAXD], owr[TT_MAXD], ofl[TT_MAXD], ofr[TT_MAXD];  // W_L, W_R, L, R of bond k in the scratch block
  int oC, oZ, oY, oW;   // launch 1's LDS regions (offsets in doubles, all even: 16-byte aligned)
  const double *core[TT_MAXD];
  const double *skl[TT_MAXD];
  const double *skr[TT_MAXD];
  double *out[TT_MAXD];
};

// doubles of LDS launch 2 needs for a bond with W_L (l x r) and W_R (r x s)
inline int64_t ny_bond_words(int64_t l, int64_t r, int64_t s) {
  const int64_t p = l < s ? l : s;
  return tt_even(l * r) + tt_even(r * s) + tt_even(l * s) + tt_even(p * p) + 2 * tt_even(p) + NY_FLAGS;
}

// doubles of LDS launch 3 needs for a core (r, n, r1) with R (q x r) and L (r1 x q1); q = 0 / q1 = 0:
// the first / last core, which has no such factor
inline int64_t ny_core_words(int64_t q, int64_t r, int64_t n, int64_t r1, int64_t q1) {
  return tt_even(r * n * r1) + tt_even(q * r) + tt_even(r1 * q1) + tt_even(r * n * q1);
}

// Validates the extents and lays out scratch and LDS.  Returns the largest dynamic-LDS request of the
// three launches in bytes, -1 when some core does not fit one workgroup (or the train has more than
// TT_MAXD cores), -2 on invalid arguments.  shm[3]: bytes per launch; *words: doubles of scratch.
int64_t ny_plan(int d, const int64_t *inner, const int64_t *ranks, const int64_t *lranks, const int64_t *rranks,
                NyPlan *p, int64_t *shm, int64_t *words) {
  const int chk = tt_check_extents(d, inner, {ranks, lranks, rranks});
  if (chk == -2 || ranks[0] != lranks[0] || ranks[0] != rranks[0] || ranks[d] != lranks[d] || ranks[d] != rranks[d])
    return -2;
  if (chk) return chk;
  const int64_t *n = inner, *r = ranks, *l = lranks, *s = rranks;
  TtLayout L, S;  // launch 1's LDS, scratch
  // launch 1: the core, the sketch core, the intermediate and the running W of either chain
  int64_t zC = 2, zZ = 2, zY = 2, zW = 2, b2 = 0, b3 = 0, pmax = 1;
  for (int k = 0; k < d; ++k) L.up(zC, r[k], n[k], r[k + 1]);
  for (int k = 1; k < d; ++k) L.up(zZ, s[k], n[k], s[k + 1]);
  for (int k = 0; k + 1 < d; ++k) L.up(zZ, l[k], n[k], l[k + 1]);
  for (int k = 1; k + 1 < d; ++k) {
    L.up(zY, r[k], n[k], s[k + 1]);
    L.up(zY, l[k], n[k], r[k + 1]);
  }
  for (int k = 0; k <= d; ++k) {
    p->r[k] = (int)r[k], p->l[k] = (int)l[k], p->s[k] = (int)s[k];
    p->q[k] = (int)(k == 0 || k == d ? r[k] : (l[k] < s[k] ? l[k] : s[k]));
  }
  for (int k = 1; k < d; ++k) {
    const int64_t lr = L.mul(l[k], r[k]), rs = L.mul(r[k], s[k]);
    L.up(zW, lr);
    L.up(zW, rs);
    L.up(b2, ny_bond_words(l[k], r[k], s[k]));
    L.up(pmax, p->q[k]);
    // W_L, W_R, L (r x q <= r x s), R (q x r <= l x r)
    p->owl[k] = S.take(lr), p->owr[k] = S.take(rs), p->ofl[k] = S.take(rs), p->ofr[k] = S.take(lr);
  }
  for (int k = 0; k < d; ++k) {
    const int64_t q = k > 0 ? p->q[k] : 0, q1 = k + 1 < d ? p->q[k + 1] : 0;
    L.up(b3, ny_core_words(q, r[k], n[k], r[k + 1], q1));
  }
  p->oC = L.take(zC), p->oZ = L.take(zZ), p->oY = L.take(zY), p->oW = L.take(zW);
  const int64_t b1 = L.words, big = b1 > b2 ? (b1 > b3 ? b1 : b3) : (b2 > b3 ? b2 : b3);
  if (L.over || big * 8 > TT_LDS_MAX) return -1;
  shm[0] = b1 * 8, shm[1] = b2 * 8, shm[2] = b3 * 8;
  *words = S.words;
  p->d = d;
  for (int k = 0; k < d; ++k) p->n[k] = (int)n[k];
  p->nt1 = tt_threads(zY > zC ? zY : zC, 1);
  p->nt2 = tt_threads(0, pmax);
  return big * 8;
}

// ---- launch 1: the two sketch chains, one workgroup each
__global__ __launch_bounds__(1024) void nystroem_sketch_kernel(const NyPlan p, double *scr) {
  extern __shared__ __attribute__((aligned(16))) double ny_lds[];
  double *C = ny_lds + p.oC, *Z = ny_lds + p.oZ, *Y = ny_lds + p.oY, *W = ny_lds + p.oW;
  const int d = p.d;
  if (blockIdx.x == 0) {
    // right to left: W_R[k] (r_k x s_k) = unfold(A_k W_R[k+1]) (r_k x n s_{k+1}) unfold(B_k)^T
    for (int k = d - 1; k >= 1; --k)  // the last core meets its sketch core directly (r_d == s_d)
      tt_sketch_step(p.core[k], p.skr[k], p.r[k], p.n[k], p.r[k + 1], p.s[k], p.s[k + 1], k == d - 1, C, Z, Y, W,
                     scr + p.owr[k]);
  } else {
    // left to right: W_L[k+1] (l_{k+1} x r_{k+1}) = unfold(G_k)^T (l_{k+1} x l_k n) unfold(W_L[k] A_k)
    for (int k = 0; k + 1 < d; ++k) {
      const int rk = p.r[k], n = p.n[k], r1 = p.r[k + 1], lk = p.l[k], l1 = p.l[k + 1];
      ro_load(C, p.core[k], rk * n * r1);
      ro_load(Z, p.skl[k], lk * n * l1);
      __syncthreads();
      const double *T = C;  // the first core meets its sketch core directly (r_0 == l_0)
      const int N = n * r1;
      if (k > 0) {
        ro_gemm(lk, N, rk, [&](int i, int c) { return W[i * rk + c]; }, [&](int c, int j) { return C[c * N + j]; },
                [&](int i, int j, double v) { Y[i * N + j] = v; });
        __syncthreads();
        T = Y;
      }
      const int K = lk * n;
      double *wk = scr + p.owl[k + 1];
      ro_gemm(l1, r1, K, [&](int i, int c) { return Z[c * l1 + i]; }, [&](int c, int j) { return T[c * r1 + j]; },
              [&](int i, int j, double v) {
                W[i * r1 + j] = v;
                wk[i * r1 + j] = v;
              });
      __syncthreads();
    }
  }
}

// ---- launch 2: workgroup b owns bond k = b + 1
__global__ __launch_bounds__(1024) void nystroem_bond_kernel(const NyPlan pl, double *scr) {
  extern __shared__ __attribute__((aligned(16))) double ny_lds[];
  const int k = blockIdx.x + 1;
  const int l = pl.l[k], r = pl.r[k], s = pl.s[k];
  const bool rows = l <= s;  // rotate the rows of P, else those of P^T
  const int p = rows ? l : s, n = rows ? s : l;
  double *WL = ny_lds, *WR = WL + tt_even(l * r), *A = WR + tt_even(r * s), *G = A + tt_even(l * s);
  double *sv = G + tt_even(p * p);
  ro_load(WL, scr + pl.owl[k], l * r);
  ro_load(WR, scr + pl.owr[k], r * s);
  __syncthreads();
  // A = P (l x s) or P^T (s x l), P = W_L W_R
  ro_gemm(l, s, r, [&](int i, int c) { return WL[i * r + c]; }, [&](int c, int j) { return WR[c * s + j]; },
          [&](int i, int j, double v) { A[rows ? i * s + j : j * l + i] = v; });
  const int *perm = tt_jacobi_svd(A, G, sv, p, n);
  // rows: G = U^T, A = diag(S) V^T:   R = diag(S^-1/2) G W_L,    L = W_R A^T diag(S^-3/2)
  // else: G = V^T, A = diag(S) U^T:   L = W_R G^T diag(S^-1/2),  R = diag(S^-3/2) A W_L
  double *Lk = scr + pl.ofl[k], *Rk = scr + pl.ofr[k];
  const double *FR = rows ? G : A, *FL = rows ? A : G;  // R's factor has rows of length l, L's of length s
  ro_gemm(p, r, l, [&](int t, int c) { return FR[perm[t] * l + c]; }, [&](int c, int j) { return WL[c * r + j]; },
          [&](int t, int j, double v) {
            const double sg = sv[perm[t]], rt = sqrt(sg);
            Rk[t * r + j] = rows ? v * (1.0 / rt) : v / (sg * rt);
          });
  ro_gemm(r, p, s, [&](int i, int c) { return WR[i * s + c]; }, [&](int c, int t) { return FL[perm[t] * s + c]; },
          [&](int i, int t, double v) {
            const double sg = sv[perm[t]], rt = sqrt(sg);
            Lk[i * p + t] = rows ? v / (sg * rt) : v * (1.0 / rt);
          });
}

// ---- launch 3: workgroup k writes out_k = R_k core_k L_{k+1}
__global__ __launch_bounds__(1024) void nystroem_core_kernel(const NyPlan pl, const double *scr) {
  extern __shared__ __attribute__((aligned(16))) double ny_lds[];
  const int k = blockIdx.x, d = pl.d;
  const int r = pl.r[k], n = pl.n[k], r1 = pl.r[k + 1];
  const int q = k > 0 ? pl.q[k] : 0, q1 = k + 1 < d ? pl.q[k + 1] : 0;
  double *C = ny_lds, *R = C + tt_even(r * n * r1), *L = R + tt_even(q * r), *T = L + tt_even(r1 * q1);
  ro_load(C, pl.core[k], r * n * r1);
  if (q) ro_load(R, scr + pl.ofr[k], q * r);
  if (q1) ro_load(L, scr + pl.ofl[k + 1], r1 * q1);
  __syncthreads();
  const double *X = C;  // (r, n, c1)
  int c1 = r1;
  if (q1) {
    ro_gemm(r * n, q1, r1, [&](int i, int c) { return C[i * r1 + c]; }, [&](int c, int j) { return L[c * q1 + j]; },
            [&](int i, int j, double v) { T[i * q1 + j] = v; });
    __syncthreads();
    X = T;
    c1 = q1;
  }
  double *o = pl.out[k];
  const int N = n * c1;
  if (q) {
    ro_gemm(q, N, r, [&](int i, int c) { return R[i * r + c]; }, [&](int c, int j) { return X[c * N + j]; },
            [&](int i, int j, double v) { o[i * N + j] = v; });
  } else {
    for (int e = threadIdx.x; e < r * N; e += blockDim.x) o[e] = X[e];
  }
}

}  // namespace

extern "C" {

int64_t ttk_nystroem_lds(int d, const int64_t *inner, const int64_t *ranks, const int64_t *lranks,
                         const int64_t *rranks) {
  NyPlan p;
  int64_t shm[3], words;
  const int64_t b = ny_plan(d, inner, ranks, lranks, rranks, &p, shm, &words);
  return b < 0 ? -1 : b;
}

int ttk_nystroem(ttk_ctx ctx, int d, const double *const *cores, const int64_t *inner, const int64_t *ranks,
                 const double *const *sk_left, const int64_t *lranks, const double *const *sk_right,
                 const int64_t *rranks, double *const *out, int64_t *out_ranks) {
  ttk::CtxScope scope(ctx);
  NyPlan p;
  int64_t shm[3] = {0, 0, 0}, words = 0;
  const int64_t big =
      (cores && sk_left && sk_right && out && out_ranks) ? ny_plan(d, inner, ranks, lranks, rranks, &p, shm, &words) : -2;
  if (const int e = tt_plan_status(
          big, "ttk_nystroem: bad arguments (d >= 2, every rank and extent >= 1, equal boundary ranks)",
          "ttk_nystroem: a core does not fit one workgroup's LDS (ttk_nystroem_lds)"))
    return e;
  for (int k = 0; k < d; ++k) {
    if (!cores[k] || !out[k] || (k + 1 < d && !sk_left[k]) || (k > 0 && !sk_right[k])) {
      ttk::set_error("ttk_nystroem: null core %d", k);
      return TTK_ERR_ARG;
    }
    p.core[k] = cores[k];
    p.skl[k] = k + 1 < d ? sk_left[k] : nullptr;
    p.skr[k] = k > 0 ? sk_right[k] : nullptr;
    p.out[k] = out[k];
  }
  TtScratch w(ttk::ctx().stream);  // W_L, W_R, L, R of every bond
  TTK_HIP(w.alloc(words));
  tt_lds_attr(nystroem_sketch_kernel, shm[0]);
  tt_lds_attr(nystroem_bond_kernel, shm[1]);
  tt_lds_attr(nystroem_core_kernel, shm[2]);
  hipLaunchKernelGGL(nystroem_sketch_kernel, dim3(2), dim3(p.nt1), (size_t)shm[0], w.st, p, w.get());
  TTK_LAUNCH_CHECK();
  hipLaunchKernelGGL(nystroem_bond_kernel, dim3(d - 1), dim3(p.nt2), (size_t)shm[1], w.st, p, w.get());
  TTK_LAUNCH_CHECK();
  hipLaunchKernelGGL(nystroem_core_kernel, dim3(d), dim3(256), (size_t)shm[2], w.st, p, (const double *)w.get());
  TTK_LAUNCH_CHECK();
  for (int k = 0; k <= d; ++k) out_ranks[k] = p.q[k];
  return TTK_OK;
}

}  // extern "C"
