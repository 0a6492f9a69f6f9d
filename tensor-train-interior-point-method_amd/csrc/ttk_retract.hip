// Deterministic fixed-rank TT retraction in ONE launch of ONE workgroup (`ttk_retract`): the
// orthogonalise-then-truncate rounding of `tt_rank_retraction` (src/tt_ops.py:132-152).
//
//   phase A (right to left)  k = d-1 .. 1: the carried core k lies in LDS as (r_k, n_k rho_{k+1}), which
//                            is its transpose in column-major order; Householder QR of that transpose in
//                            place (rho_k = min(n_k rho_{k+1}, r_k) columns of Q, m < n handled), Q^T is the
//                            orthogonalised core k (rho_k, n_k, rho_{k+1}) and goes to the call's scratch
//                            block, carried core k-1 = core_{k-1} R^T stays in LDS;
//   phase B (left to right)  i = 0 .. d-2: one-sided Jacobi SVD of the carried Z (q_i n_i, rho_{i+1}) on the
//                            rows of whichever of Z or Z^T has fewer, singular values sorted descending
//                            (ties by index), out_i = U[:, :q_{i+1}], M = diag(S) V^T (q_{i+1} x rho_{i+1}),
//                            carried <- M x orthogonalised core i+1 (read back from scratch); the last
//                            carried core is out_{d-1}.
//
// No sketch, no random draw, no truncation decision and no host read: every extent follows from the
// host-side rank rule rho_d = 1, rho_k = min(n_k rho_{k+1}, r_k); q_0 = 1, q_{i+1} = min(upper_i, q_i n_i,
// rho_{i+1}) before the launch.  The reference's sweep also runs i = 0 and moves a scalar into the last
// core; this one leaves it in the first carried core: the gauge differs, the represented tensor does
// not.  The one workgroup runs alone through bounded loops (the Jacobi sweeps by NY_SWEEPS) and
// workgroup barriers only (no inter-workgroup hand-off, no spin wait, no atomics), so it does not
// depend on co-residency.  Every product sums k ascending in one fma chain per output element, every
// reduction is a fixed wave tree and the Jacobi pairs follow one fixed round-robin order, so two
// calls on the same input give the same bits.
//
// A singular value that is exactly 0 gives a zero column of U (rows of Z^T rotated) or a zero row of M
// (rows of Z rotated): nothing divides by it, so the all-zero train comes back as finite cores.
//
// `ttk_round_one` is the same two sweeps with the eps-truncating rank rule of `tt_rank_reduce` and its
// tracked variants (cy_src/tt_ops_cy.pyx:161-226, :299-309) decided in the kernel (retract_kernel<true, RtPlan>):
// after each Jacobi one thread sums the squared singular values from the smallest upward, picks q_{i+1}
// by the reference's rule, clamps it to [1, min(m, rho_{i+1})] and publishes it in one LDS word behind
// one workgroup barrier; from there q_{i+1}, m = q_i n_i, the orientation and the extents of out_i, M
// and the carried core are run-time values, uniform across the workgroup.  LDS and the thread count
// are planned from the bound ranks (no upper bound), which the run-time ranks can only undercut.  The
// ranks and the discarded tail go to `info` on the device; the call itself reads nothing back.
//
// `ttk_affine_round_one` is `ttk_round_one` on an operand that is never built: S = sum_j c_j op_j(T_j) of up to
// RS_TERMS terms, each a plain train or the core-wise product of two (at most RA_PRODS of them), in `tt_add`'s
// block layout at the prefix sums of the term ranks (cy_src/tt_ops_cy.pyx:94-114, :243-258).  The kernel reads
// its input cores in exactly two places, and there the core of S -- term j's block, times c_j in core 0, its two
// middle indices swapped where asked, exactly 0.0 elsewhere -- is written straight into the LDS region the plain
// load fills, each element once by the thread that owns it (rt_load_core on RtAffineArg).  A product term is the
// device path's `tt_fast_matrix_vec_mul`, `tt_fast_mat_mat_mul` or `tt_fast_hadamard` before its rounding
// (Kronecker bonds), row a r_b + b, column A R_b + B, each element one multiply or a short fma
// chain over the contracted index of two small cores read from global memory.  The plan is the one of the summed
// ranks; everything after the loads is retract_kernel<true, RtPlan>'s code.  With the plan's RT_NORM2 bit the
// kernel also leaves ||result||^2 in info[d + 2]: after phase B every output core but the last has orthonormal
// columns, so that is the sum of squares of the last carried core, reduced by wave 0 in a fixed order.
//
// `ttk_sum_round_one` (plain terms only) and `ttk_prod_round_one` (one product, weight exactly 1.0, not
// transposed) are that operand and that kernel: their entry points translate their arguments into terms, plan
// and launch through the same code, and clear RT_NORM2, since their info has d + 2 words.  A sum of plain terms
// or a single product given to `ttk_affine_round_one` therefore has their bits by construction.
//
// `ttk_affine_round_many` runs up to TTK_ROUND_MANY_MAX of these roundings in one launch, workgroup j on job j
// (retract_many_kernel).  The body is the same function (retract_body); the jobs' RtAffineArg records lie in a
// device-memory table at the front of the call's scratch block, uploaded stream-ordered before the launch, and each
// workgroup works with its own job's planned thread count whatever the launch width, so every job has the bits
// of its own `ttk_affine_round_one`.  The workgroups share read-only data only and none waits for another.
//
// LDS holds one step's working set, not the train: two carried-core regions that the phases use in
// turn (QR input / Q, then Z / the Jacobi's rows), one core from global memory or scratch, the
// rotations G, M and a few small vectors.  The products are VALU fma chains, as in the siblings.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "ttk_common.h"
#include "ttk_internal.h"
#include "ttk_tt_gemm.h"

namespace {

struct RtPlan {
  int d, nt;
  int n[TT_MAXD];        // middle extents
  int r[TT_MAXD + 1];    // train bond ranks
  int rho[TT_MAXD + 1];  // bond ranks after the QR sweep
  int q[TT_MAXD + 1];    // output bond ranks (ttk_round_one: their bounds)
  int so[TT_MAXD];       // orthogonalised core k's offset in the scratch block (doubles), k = 1 .. d-1
  int oP0, oP1, oC, oG, oM, oT, oS;  // LDS regions (offsets in doubles, all even: 16-byte aligned)
  int oQ;                // ttk_round_one: the run-time ranks q_0 .. q_{d-1} as doubles (each one published once)
  int track;             // ttk_round_one: RT_TRACK | RT_NORM2, uniform across the workgroup
  double thr2;           // ttk_round_one: the squared per-bond threshold
  double *info;          // ttk_round_one: d + 2 device doubles, the ranks and the tail (RT_NORM2: d + 3)
  const double *core[TT_MAXD];
  double *out[TT_MAXD];
};

constexpr int RT_TRACK = 1;  // mode 1: the discarded tail sums are accumulated
constexpr int RT_NORM2 = 2;  // ||result||^2 goes to info[d + 2] (the affine entries; the others own d + 2 words)

constexpr int RS_TERMS = 4;  // terms of an operand
constexpr int RA_PRODS = 2;  // product terms among them

// The operand of every rounding of a train that is never built (`ttk_sum_round_one`, `ttk_prod_round_one`,
// `ttk_affine_round_one` and `_many`): the plan of S (p.r the summed ranks, p.core unused) and the terms.  Term j
// is the train a[j] (kind -1) or the product of a[j] and b[slot[j]] (kinds 0 .. 3).  Per product slot: core k of a
// is (ra_k, m0_k, m1_k, ra_{k+1}); of b (rb_k, m1_k, m2_k, rb_{k+1}) where the products contract m1 (kind 0 with
// m2 = 1, kind 1), (rb_k, m0_k m1_k, rb_{k+1}) where they multiply elementwise (kind 2 with m1 = 1, kind 3); an
// extent the kind does not use is stored as 1.  Ranks and extents are 16-bit (TT_CAP fits) so that four terms,
// two of them products, travel as one kernel argument.
struct RtAffineArg {
  RtPlan p;
  int nterms;
  signed char kind[RS_TERMS], slot[RS_TERMS], tr[RS_TERMS];
  double coef[RS_TERMS];                      // applied to the term's core 0
  unsigned short n1[TT_MAXD];                 // first middle extent of S's core k
  unsigned short r[RS_TERMS][TT_MAXD + 1];    // the terms' bond ranks in S (ra rb for a product)
  unsigned short ra[RA_PRODS][TT_MAXD + 1], rb[RA_PRODS][TT_MAXD + 1];
  unsigned short m0[RA_PRODS][TT_MAXD], m1[RA_PRODS][TT_MAXD], m2[RA_PRODS][TT_MAXD];
  const double *a[RS_TERMS][TT_MAXD];
  const double *b[RA_PRODS][TT_MAXD];
};
static_assert(TT_CAP < 65536, "ranks and extents are stored as 16-bit");
static_assert(sizeof(RtAffineArg) < 4096, "the plan and the terms travel as one kernel argument");

// Validates the extents, applies the rank rule and lays out LDS and scratch.  Returns the bytes of
// dynamic LDS, -1 when the train does not fit one workgroup (or has more than TT_MAXD cores), -2 on
// invalid arguments.  *words: doubles of scratch for the orthogonalised cores 1 .. d-1.  adapt
// (ttk_round_one): no upper bound, q holds the bound ranks, and the plan takes one more region for the
// run-time ranks.
int64_t rt_plan(int d, const int64_t *inner, const int64_t *ranks, const int64_t *upper, bool adapt, RtPlan *p,
                int64_t *words) {
  const int chk = tt_check_extents(d, inner, {ranks});
  bool bad = chk == -2 || (!adapt && !upper) || ranks[0] != 1 || ranks[d] != 1;
  for (int k = 0; !bad && !adapt && k + 1 < d; ++k) bad = upper[k] < 1;
  if (bad) return -2;
  if (chk) return chk;
  const int64_t *n = inner, *r = ranks;
  int64_t rho[TT_MAXD + 1], q[TT_MAXD + 1];
  rho[d] = 1;
  rho[0] = 1;
  for (int k = d - 1; k >= 1; --k) {
    const int64_t m = n[k] * rho[k + 1];  // <= TT_CAP * TT_CAP: no overflow
    rho[k] = m < r[k] ? m : r[k];
  }
  q[0] = 1;
  q[d] = 1;
  for (int i = 0; i + 1 < d; ++i) {
    const int64_t m = q[i] * n[i];
    int64_t v = (!adapt && upper[i] < m) ? upper[i] : m;
    q[i + 1] = v < rho[i + 1] ? v : rho[i + 1];
  }
  TtLayout L, S;  // LDS, scratch
  int64_t zP = 2, zC = 2, zG = 2, zM = 2, zT = 2, zS = 2, pmax = 1;
  for (int k = d - 1; k >= 1; --k) {
    L.up(zP, r[k], n[k], rho[k + 1]);            // carried core k; Q^T (rho_k n_k rho_{k+1}) is no larger
    L.up(zP, r[k - 1], n[k - 1], rho[k]);        // carried core k-1
    L.up(zC, r[k - 1], n[k - 1], r[k]);          // core k-1 as it lies
    L.up(zT, rho[k]);                            // tau
    const int64_t qs = L.mul(rho[k], n[k], rho[k + 1]);
    L.up(zC, qs);                                // orthogonalised core k, read back in phase B
    p->so[k] = S.take(qs);
  }
  for (int i = 0; i < d; ++i) {
    L.up(zP, q[i], n[i], rho[i + 1]);            // Z, and the Jacobi's rows (Z or Z^T)
    if (i + 1 == d) break;
    const int64_t m = q[i] * n[i], pp = m < rho[i + 1] ? m : rho[i + 1];
    L.up(zG, pp, pp);
    L.up(zS, pp);
    L.up(pmax, pp);
    L.up(zM, q[i + 1], rho[i + 1]);
  }
  p->oP0 = L.take(zP), p->oP1 = L.take(zP), p->oC = L.take(zC), p->oG = L.take(zG), p->oM = L.take(zM);
  p->oT = L.take(zT), p->oS = L.take(zS);  // sv, then perm and the flags
  L.take(zS), L.take(NY_FLAGS);
  p->oQ = adapt ? L.take(d) : 0;
  if (L.over || L.words * 8 > TT_LDS_MAX) return -1;
  *words = S.words;
  p->d = d;
  p->track = 0, p->thr2 = 0.0, p->info = nullptr;
  p->nt = tt_threads(zP > zC ? zP : zC, pmax);
  for (int k = 0; k < d; ++k) p->n[k] = (int)n[k];
  for (int k = 0; k <= d; ++k) p->r[k] = (int)r[k], p->rho[k] = (int)rho[k], p->q[k] = (int)q[k];
  return L.words * 8;
}

__device__ __forceinline__ const RtPlan &rt_plan_of(const RtPlan &a) { return a; }
__device__ __forceinline__ const RtPlan &rt_plan_of(const RtAffineArg &a) { return a.p; }

// Core k of the train, (r_k, n_k, r_{k+1}) row-major, into dst.  No barrier: the caller's next one publishes it.
// (tid, nt): the team, as in ttk_tt_gemm.h, here and in the operand's loader below.
__device__ __forceinline__ void rt_load_core(double *dst, const RtPlan &a, int k, int tid, int nt) {
  ro_load(dst, a.core[k], a.r[k] * a.n[k] * a.r[k + 1], tid, nt);
}

// The element code of the operand's loader.
// The term's own middle index of S's middle index i = i1 n2 + i2: i2 n1 + i1 where the term is transposed.
__device__ __forceinline__ int rt_term_mid(bool tr, int i, int n1, int n2) {
  if (!tr) return i;
  const int i1 = i / n2, i2 = i - i1 * n2;
  return i2 * n1 + i1;
}

// The weight, applied in core 0 only; a weight of exactly 1.0 copies the bits.
__device__ __forceinline__ double rt_weighted(bool first, double coef, double x) {
  return (first && coef != 1.0) ? __dmul_rn(coef, x) : x;
}

// Element (a rb + b, mid, A Rb + B) of a product core from the factors' cores in global memory.  Kinds 0 and
// 1: mid = i m2 + j, sum over c < m1 of a[a, i, c, A] b[b, c, j, B], the first term a rounded product, the
// others added by fma with c ascending.  Kinds 2 and 3: a[a, mid, A] b[b, mid, B], one rounded product, n the
// product's middle extent.  The largest source index is below the factor core's size, which the plan's fit
// keeps under 2^31 (ra m0 Ra and rb m2 Rb <= TT_CAP each, m1 <= TT_CAP).
__device__ __forceinline__ double rt_prod_elem(bool contract, const double *__restrict__ pa,
                                               const double *__restrict__ pb, int a, int b, int mid, int A, int B,
                                               int Ra, int Rb, int m0, int m1, int m2, int n) {
  if (contract) {
    const int i = mid / m2, j = mid - i * m2;
    const double *xa = pa + ((a * m0 + i) * m1) * Ra + A;  // stride Ra over c
    const double *xb = pb + (b * m1 * m2 + j) * Rb + B;    // stride m2 Rb over c
    const int sb = m2 * Rb;
    double v = __dmul_rn(xa[0], xb[0]);
    for (int c = 1; c < m1; ++c) v = fma(xa[c * Ra], xb[c * sb], v);
    return v;
  }
  return __dmul_rn(pa[(a * n + mid) * Ra + A], pb[(b * n + mid) * Rb + B]);
}

// Core k of the operand: element (row, i, col) belongs to the one term whose row range holds row (every term at
// k = 0, where R_0 = 1) and whose column range holds col (every term at k = d-1), and is 0.0 if there is none.
// The term's middle index is remapped first where it is transposed, then the plain element is loaded or the
// product element (row a rb + b, column A Rb + B of the term) computed at that index, then the weight applied.
// Each destination element is written once, by the thread that owns it; kind, the term tables and every
// extent are kernel arguments (in the batched launch, the job's record) indexed by the uniform j and k.
__device__ __forceinline__ void rt_load_core(double *dst, const RtAffineArg &s, int k, int tid, int nt) {
  const int n = s.p.n[k], R1 = s.p.r[k + 1], nR1 = n * R1, total = s.p.r[k] * nR1;
  const int n1 = s.n1[k], n2 = n / n1;
  const bool first = k == 0, last = k == s.p.d - 1;
  for (int e = tid; e < total; e += nt) {
    const int row = e / nR1, rem = e - row * nR1, i = rem / R1, col = rem - i * R1;
    double v = 0.0;
    int A0 = 0, B0 = 0;
    for (int j = 0; j < s.nterms; ++j) {
      const int rj = s.r[j][k], Rj = s.r[j][k + 1];
      const int la = first ? 0 : row - A0, lb = last ? 0 : col - B0;
      if (la >= 0 && la < rj && lb >= 0 && lb < Rj) {
        const int mid = rt_term_mid(s.tr[j] != 0, i, n1, n2);
        double x;
        if (s.kind[j] < 0) {
          x = s.a[j][k][(la * n + mid) * Rj + lb];
        } else {
          const int t = s.slot[j], rb = s.rb[t][k], Rb = s.rb[t][k + 1];
          const int a = la / rb, b = la - a * rb, A = lb / Rb, B = lb - A * Rb;
          x = rt_prod_elem(s.kind[j] < 2, s.a[j][k], s.b[t][k], a, b, mid, A, B, s.ra[t][k + 1], Rb, s.m0[t][k],
                           s.m1[t][k], s.m2[t][k], n);
        }
        v = rt_weighted(first, s.coef[j], x);
      }
      A0 += rj, B0 += Rj;
    }
    dst[e] = v;
  }
}

// ADAPT false: `ttk_retract`, every q_i from the plan.  ADAPT true: `ttk_round_one`, p.q holds the bounds and
// q_{i+1} is decided after bond i's Jacobi.  Arg: RtPlan, the cores as they lie in global memory, or RtAffineArg,
// the cores of a weighted sum of trains and products (`ttk_sum_round_one`, `ttk_prod_round_one`,
// `ttk_affine_round_one`); it only enters the two rt_load_core calls.  Whether info[d + 2] is written is the
// plan's RT_NORM2 bit, read at run time: the sum and product entries own d + 2 words of info and leave it clear.
//
// The body is one function for the single-call kernel and the batched one (retract_many_kernel).  (tid, nt) is
// the team of ttk_tt_gemm.h: the single-call kernels pass (threadIdx.x, blockDim.x) with blockDim.x == p.nt; the
// batched kernel passes p.nt and TT_IDLE for the threads its wider workgroup has beyond it.  Every loop strides
// by nt and every reduction is ordered by nt, so the bits are those of a launch with blockDim.x == nt.
template <bool ADAPT, class Arg>
__device__ __forceinline__ void retract_body(const Arg &arg, double *scr, const int tid, const int nt) {
  const RtPlan &p = rt_plan_of(arg);
  extern __shared__ __attribute__((aligned(16))) double rt_lds[];
  double *P[2] = {rt_lds + p.oP0, rt_lds + p.oP1};
  double *C = rt_lds + p.oC, *G = rt_lds + p.oG, *Mq = rt_lds + p.oM, *tau = rt_lds + p.oT, *sv = rt_lds + p.oS;
  const int d = p.d;
  int cur = 0;
  // ---- phase A: right to left; P[cur] holds the carried core k as (r_k, n_k rho_{k+1})
  rt_load_core(P[0], arg, d - 1, tid, nt);
  for (int k = d - 1; k >= 1; --k) {
    const int rk = p.r[k], m = p.n[k] * p.rho[k + 1], kk = p.rho[k], rows = p.r[k - 1] * p.n[k - 1];
    double *Y = P[cur], *Qc = P[cur ^ 1];
    rt_load_core(C, arg, k - 1, tid, nt);
    __syncthreads();
    // the carried core's rows are the columns of its transpose (m x r_k, column-major)
    ro_householder(Y, m, rk, tau, tid, nt);
    ro_form_q(Y, tau, m, kk, Qc, tid, nt);
    // Q (m x kk, column-major) is Q^T row-major: the orthogonalised core k (rho_k, n_k, rho_{k+1})
    double *ok = scr + p.so[k];
    for (int e = tid; e < m * kk; e += nt) ok[e] = Qc[e];
    __syncthreads();
    // carried core k-1 (rows x kk) = core_{k-1} (rows x r_k) R^T, R (kk x r_k) the upper trapezoid of Y
    ro_gemm(rows, kk, rk, [&](int i, int c) { return C[i * rk + c]; },
            [&](int c, int j) { return j <= c ? Y[c * m + j] : 0.0; },
            [&](int i, int j, double v) { Qc[i * kk + j] = v; }, tid, nt);
    __syncthreads();
    cur ^= 1;
  }
  // ---- phase B: left to right; Z holds the carried core i as (q_i n_i, rho_{i+1})
  double *Z = P[cur], *A = P[cur ^ 1];
  double *qd = rt_lds + p.oQ;  // ADAPT: q_i as decided, one word per bond
  double tail = 0.0;           // ADAPT: thread 0's sum of the discarded tails
  int qi = 1;
  for (int i = 0; i + 1 < d; ++i) {
    if (!ADAPT) qi = p.q[i];
    const int m = qi * p.n[i], R = p.rho[i + 1], rest = p.n[i + 1] * p.rho[i + 2];
    const bool rowsz = m <= R;  // rotate the rows of Z, else those of Z^T
    const int pp = rowsz ? m : R, n = rowsz ? R : m;
    ro_load(C, scr + p.so[i + 1], R * rest, tid, nt);
    for (int e = tid; e < m * R; e += nt) {
      const int a = e / R, c = e - a * R;
      A[rowsz ? e : c * m + a] = Z[e];
    }
    const int *perm = tt_jacobi_svd(A, G, sv, pp, n, tid, nt);
    int qn = p.q[i + 1];
    if (ADAPT) {  // one thread decides, one barrier publishes: qn is uniform and 1 <= qn <= pp <= p.q[i + 1]
      if (tid == 0) qd[i + 1] = (double)rt_kept_rank(sv, perm, pp, p.thr2, (p.track & RT_TRACK) != 0, &tail);
      __syncthreads();
      qn = (int)qd[i + 1];
    }
    // rows of Z:   G = U^T, A = diag(S) V^T:  out_i = G^T[:, top],        M = A[top]
    // rows of Z^T: G = V^T, A = diag(S) U^T:  out_i = (A / S)^T[:, top],  M = diag(S) G[top]
    double *oi = p.out[i];
    for (int e = tid; e < m * qn; e += nt) {
      const int a = e / qn, t = e - a * qn, row = perm[t];
      if (rowsz) {
        oi[e] = G[row * pp + a];
      } else {
        const double sg = sv[row];
        oi[e] = sg > 0.0 ? A[row * n + a] / sg : 0.0;
      }
    }
    for (int e = tid; e < qn * R; e += nt) {
      const int t = e / R, c = e - t * R, row = perm[t];
      Mq[e] = rowsz ? A[row * n + c] : sv[row] * G[row * pp + c];
    }
    __syncthreads();
    // Z (qn x rest) <- M (qn x R) x orthogonalised core i+1 (R x rest)
    ro_gemm(qn, rest, R, [&](int a, int c) { return Mq[a * R + c]; }, [&](int c, int j) { return C[c * rest + j]; },
            [&](int a, int j, double v) { Z[a * rest + j] = v; }, tid, nt);
    __syncthreads();
    qi = qn;
  }
  if (!ADAPT) qi = p.q[d - 1];
  double *ol = p.out[d - 1];
  for (int e = tid; e < qi * p.n[d - 1]; e += nt) ol[e] = Z[e];
  if (ADAPT && tid == 0) {  // the ranks (thread 0's own LDS words) and the tail
    p.info[0] = 1.0;
    for (int k = 1; k < d; ++k) p.info[k] = qd[k];
    p.info[d] = 1.0;
    p.info[d + 1] = tail;
  }
  if (ADAPT && (p.track & RT_NORM2)) {
    // ||result||^2 = the sum of squares of the last carried core (published by the loop's last barrier): wave 0
    // alone, lane l the elements l, l + 64, ... ascending, then the fixed wave tree
    if (tid < 64) {
      const int cnt = qi * p.n[d - 1];
      double part = 0.0;
      for (int e = tid; e < cnt; e += 64) part = fma(Z[e], Z[e], part);
      part = ttk::wave_sum(part);
      if (tid == 0) p.info[d + 2] = part;
    }
  }
}

template <bool ADAPT, class Arg>
__global__ __launch_bounds__(1024) void retract_kernel(const Arg arg, double *scr) {
  retract_body<ADAPT>(arg, scr, threadIdx.x, blockDim.x);
}

// `ttk_affine_round_many`: one record per job, a table in device memory.  a.p.info already points at the job's
// words of the call's info block; scr is the job's offset (doubles) into the call's scratch block.
struct alignas(16) RtManyJob {
  RtAffineArg a;
  int64_t scr;
};
static_assert(sizeof(RtManyJob) % 16 == 0, "the table is an array of aligned records");

// Workgroup j rounds job j with retract_kernel<true, RtAffineArg>'s body and the job's own team: the launch is as
// wide as the widest plan, and a workgroup's threads beyond its job's p.nt are TT_IDLE.  The workgroups share
// nothing but the read-only inputs and the table, and none waits for another.  The record is read through the
// uniform index blockIdx.x.
__global__ __launch_bounds__(1024) void retract_many_kernel(const RtManyJob *__restrict__ jobs, double *scr) {
  const RtManyJob &job = jobs[blockIdx.x];
  const int nt = job.a.p.nt;
  retract_body<true>(job.a, scr + job.scr, (int)threadIdx.x < nt ? (int)threadIdx.x : TT_IDLE, nt);
}

// The checks on the two factors of a product term (`ttk_prod_round_one`'s, which takes its middle extents from
// here, and those of `ttk_affine_round_one`): -2 on invalid arguments, -1 when a rank, an extent or a product of
// two passes TT_CAP or d passes TT_MAXD, else 0 with inner[k] the product's middle extents and m[3k ..] the physical extents (1 where the kind has none).
int rp_check(int kind, int d, const int64_t *a_ranks, const int64_t *b_ranks, const int64_t *modes, int64_t *inner,
             int *m) {
  if (kind < 0 || kind > 3 || d < 2 || !a_ranks || !b_ranks || !modes) return -2;
  const bool use1 = kind != 2, use2 = kind == 1;  // whether modes[3k + 1], modes[3k + 2] mean anything
  bool big = d > TT_MAXD;
  for (int k = 0; k <= d; ++k) {
    if (a_ranks[k] < 1 || b_ranks[k] < 1) return -2;
    big |= a_ranks[k] > TT_CAP || b_ranks[k] > TT_CAP || a_ranks[k] * b_ranks[k] > TT_CAP;  // factors <= TT_CAP first
  }
  for (int k = 0; k < d; ++k) {
    const int64_t m0 = modes[3 * k], m1 = use1 ? modes[3 * k + 1] : 1, m2 = use2 ? modes[3 * k + 2] : 1;
    if (m0 < 1 || m1 < 1 || m2 < 1) return -2;
    big |= m0 > TT_CAP || m1 > TT_CAP || m2 > TT_CAP || m0 * (kind == 1 ? m2 : kind == 3 ? m1 : 1) > TT_CAP;
  }
  if (a_ranks[0] != 1 || a_ranks[d] != 1 || b_ranks[0] != 1 || b_ranks[d] != 1) return -2;
  if (big) return -1;  // d <= TT_MAXD, every rank, extent and product of two <= TT_CAP from here on
  for (int k = 0; k < d; ++k) {
    const int64_t m0 = modes[3 * k], m1 = use1 ? modes[3 * k + 1] : 1, m2 = use2 ? modes[3 * k + 2] : 1;
    inner[k] = kind == 1 ? m0 * m2 : kind == 3 ? m0 * m1 : m0;
    m[3 * k] = (int)m0, m[3 * k + 1] = (int)m1, m[3 * k + 2] = (int)m2;
  }
  return 0;
}

// The checks on the terms of an operand and the plan of S: the bytes of dynamic LDS, -1 when S does not fit one
// workgroup, -2 on invalid arguments or more than RS_TERMS terms or RA_PRODS products.  sum: the summed ranks,
// d + 1 entries.  ptrs false (`ttk_prod_round_one_lds`, which is given no cores): the core tables a and b are
// neither examined nor copied.
int64_t ra_plan(int d, const int64_t *inner, int nterms, const ttk_affine_term *terms, bool ptrs, RtAffineArg *a,
                int64_t *words, int64_t *sum) {
  if (nterms < 1 || nterms > RS_TERMS || !terms) return -2;
  if (tt_check_extents(d, inner, {}) == -2) return -2;
  int nprod = 0;
  for (int j = 0; j < nterms; ++j) nprod += terms[j].kind >= 0;
  if (nprod > RA_PRODS) return -2;
  bool big = false;
  int64_t mid[TT_MAXD];
  int m[RA_PRODS][3 * TT_MAXD];
  nprod = 0;
  for (int j = 0; j < nterms; ++j) {
    const ttk_affine_term &t = terms[j];
    if (t.kind < -1 || t.kind > 3 || (ptrs && !t.a) || !t.a_ranks || !std::isfinite(t.coef) ||
        (t.transpose != 0 && t.transpose != 1))
      return -2;
    if (t.kind < 0) {
      if (t.b || t.b_ranks || t.modes) return -2;
      const int chk = tt_check_extents(d, inner, {t.a_ranks});
      if (chk == -2 || t.a_ranks[0] != 1 || t.a_ranks[d] != 1) return -2;
      big |= chk != 0;
    } else {
      if (ptrs && !t.b) return -2;
      const int chk = rp_check(t.kind, d, t.a_ranks, t.b_ranks, t.modes, mid, m[nprod++]);
      if (chk == -2) return -2;
      big |= chk != 0;
      for (int k = 0; !chk && k < d; ++k)
        if (mid[k] != inner[k]) return -2;  // the product's middle extent is S's
    }
  }
  if (big || tt_check_extents(d, inner, {}) != 0) return -1;  // d <= TT_MAXD, ranks and extents <= TT_CAP from here on
  for (int j = 0; ptrs && j < nterms; ++j)
    for (int k = 0; k < d; ++k)
      if (!terms[j].a[k] || (terms[j].kind >= 0 && !terms[j].b[k])) return -2;
  sum[0] = sum[d] = 1;
  for (int k = 1; k < d; ++k) {
    sum[k] = 0;
    for (int j = 0; j < nterms; ++j)
      sum[k] += terms[j].kind < 0 ? terms[j].a_ranks[k] : terms[j].a_ranks[k] * terms[j].b_ranks[k];
  }
  const int64_t shm = rt_plan(d, inner, sum, nullptr, true, &a->p, words);
  if (shm < 0) return shm;
  a->nterms = nterms;
  nprod = 0;
  for (int t = 0; t < RA_PRODS; ++t)
    for (int k = 0; k <= d; ++k) {
      a->ra[t][k] = a->rb[t][k] = 1;
      if (k < d) a->m0[t][k] = a->m1[t][k] = a->m2[t][k] = 1, a->b[t][k] = nullptr;
    }
  for (int j = 0; j < RS_TERMS; ++j) {
    const bool on = j < nterms, prod = on && terms[j].kind >= 0;
    const int t = prod ? nprod++ : 0;
    a->kind[j] = on ? (signed char)terms[j].kind : -1;
    a->slot[j] = (signed char)t;
    a->tr[j] = on ? (signed char)terms[j].transpose : 0;
    a->coef[j] = on ? terms[j].coef : 0.0;
    for (int k = 0; k <= d; ++k) {
      const int64_t ra = on ? terms[j].a_ranks[k] : 0, rb = prod ? terms[j].b_ranks[k] : 1;
      a->r[j][k] = (unsigned short)(ra * rb);
      if (prod) a->ra[t][k] = (unsigned short)ra, a->rb[t][k] = (unsigned short)rb;
    }
    for (int k = 0; k < d; ++k) {
      a->a[j][k] = on && ptrs ? terms[j].a[k] : nullptr;
      if (prod) {
        a->b[t][k] = ptrs ? terms[j].b[k] : nullptr;
        a->m0[t][k] = (unsigned short)m[t][3 * k], a->m1[t][k] = (unsigned short)m[t][3 * k + 1];
        a->m2[t][k] = (unsigned short)m[t][3 * k + 2];
      }
    }
  }
  for (int k = 0; k < d; ++k) a->n1[k] = (unsigned short)inner[k], a->p.core[k] = nullptr;
  return shm;
}

// The three `_lds` planners: ra_plan's bytes of LDS, -1 for both of its failures, with the summed (product) ranks
// and the bound ranks, d + 1 entries each, where the caller asks for them.
int64_t ra_lds(int d, const int64_t *inner, int nterms, const ttk_affine_term *terms, bool ptrs, int64_t *sum_ranks,
               int64_t *bound) {
  RtAffineArg a;
  int64_t words, sum[TT_MAXD + 1];
  const int64_t b = ra_plan(d, inner, nterms, terms, ptrs, &a, &words, sum);
  if (b < 0) return -1;
  for (int k = 0; sum_ranks && k <= d; ++k) sum_ranks[k] = sum[k];
  for (int k = 0; bound && k <= d; ++k) bound[k] = a.p.q[k];
  return b;
}

// What each entry's bad-arguments message lists: only the rules its own caller can break.
const char RS_RULES[] =
    "d >= 2, 1 to 4 terms, every rank and extent >= 1, boundary ranks 1, no null pointer, coef finite, transpose 0 "
    "or 1, eps finite and >= 0, mode 0 or 1";
const char RP_RULES[] =
    "kind 0 to 3, d >= 2, every rank and extent >= 1, boundary ranks 1, no null pointer, eps finite and >= 0, mode "
    "0 or 1";
const char RA_RULES[] =
    "d >= 2, 1 to 4 terms, at most 2 of them products, kind -1 to 3, b, b_ranks and modes null exactly for kind -1, "
    "every rank and extent >= 1, boundary ranks 1, a product's middle extent equal to inner, no null pointer, coef "
    "finite, transpose 0 or 1, eps finite and >= 0, mode 0 or 1";

// A failed plan (-2 invalid, -1 no fit) as the entry's error.  who: the name the message starts with, or null for
// the planners, which set none.
int ra_fail(const char *who, const char *rules, int64_t shm) {
  if (who && shm == -2) ttk::set_error("%s: bad arguments (%s)", who, rules);
  if (who && shm != -2) ttk::set_error("%s: the operand does not fit one workgroup's LDS (its _lds gives -1)", who);
  return TTK_ERR_ARG;
}

// Every check of the three entries on one operand, also for each job of `ttk_affine_round_many`, and the finished
// kernel argument (plan, terms, rows, threshold, mode, out, info).  who, rules: ra_fail's.  outs: whether out and
// info are examined.  norm2: info has d + 3 words and the last takes ||result||^2.  Returns TTK_OK with *shm and
// *words set, else TTK_ERR_ARG.
int ra_prepare(const char *who, const char *rules, int d, const int64_t *inner, const int64_t *rows, int nterms,
               const ttk_affine_term *terms, double eps, int mode, bool outs, bool norm2, double *const *out,
               double *info, RtAffineArg *a, int64_t *words, int64_t *shm) {
  int64_t sum[TT_MAXD + 1];
  const bool ok = (!outs || (out && info)) && eps >= 0.0 && eps <= 1.79769313486231570e308 && (mode == 0 || mode == 1);
  *shm = ok ? ra_plan(d, inner, nterms, terms, true, a, words, sum) : -2;
  if (*shm < 0) return ra_fail(who, rules, *shm);
  bool transposed = false;
  for (int j = 0; j < nterms; ++j) transposed |= terms[j].transpose != 0;
  if (transposed && !rows) {
    if (who) ttk::set_error("%s: a transposed term needs rows", who);
    return TTK_ERR_ARG;
  }
  for (int k = 0; k < d; ++k) {
    if (rows && (rows[k] < 1 || inner[k] % rows[k] != 0)) {
      if (who) ttk::set_error("%s: rows[%d] does not divide inner[%d]", who, k, k);
      return TTK_ERR_ARG;
    }
    if (outs && !out[k]) {
      if (who) ttk::set_error("%s: null out %d", who, k);
      return TTK_ERR_ARG;
    }
    if (rows) a->n1[k] = (unsigned short)rows[k];
    a->p.out[k] = outs ? out[k] : nullptr;
  }
  const double e = (mode ? eps / 2.0 : eps) / std::sqrt((double)(d - 1));
  a->p.thr2 = e * e;
  a->p.track = (mode ? RT_TRACK : 0) | (norm2 ? RT_NORM2 : 0);
  a->p.info = info;
  return TTK_OK;
}

// One launch of the operand's kernel on the context's stream: `ttk_sum_round_one`, `ttk_prod_round_one` and
// `ttk_affine_round_one` after ra_prepare.
int ra_launch(const RtAffineArg &a, int64_t words, int64_t shm) {
  TtScratch w(ttk::ctx().stream);  // the orthogonalised cores 1 .. d-1
  TTK_HIP(w.alloc(words));
  tt_lds_attr(retract_kernel<true, RtAffineArg>, shm);
  hipLaunchKernelGGL((retract_kernel<true, RtAffineArg>), dim3(1), dim3(a.p.nt), (size_t)shm, w.st, a, w.get());
  TTK_LAUNCH_CHECK();
  return TTK_OK;
}

// `ttk_sum_round_one`'s terms as plain terms of the operand (kind -1: the train, its weight and transposition as
// given), in t; null when there is no table.  nterms is ra_plan's to check.
const ttk_affine_term *rs_terms(int nterms, const ttk_sum_term *terms, ttk_affine_term *t) {
  for (int j = 0; terms && j < nterms && j < RS_TERMS; ++j)
    t[j] = {-1, terms[j].transpose, terms[j].coef, terms[j].cores, terms[j].ranks, nullptr, nullptr, nullptr};
  return terms ? t : nullptr;
}

// `ttk_prod_round_one`'s factors as the operand's one product term, weight exactly 1.0 (the bits are copied) and
// not transposed, in *t, and the product's middle extents in inner (TT_MAXD entries): rp_check's status.
int rp_term(int kind, int d, const double *const *a, const int64_t *a_ranks, const double *const *b,
            const int64_t *b_ranks, const int64_t *modes, ttk_affine_term *t, int64_t *inner) {
  int m[3 * TT_MAXD];
  *t = {kind, 0, 1.0, a, a_ranks, b, b_ranks, modes};
  return rp_check(kind, d, a_ranks, b_ranks, modes, inner, m);
}

// `ttk_affine_round_many`'s plan: every job prepared (ra_prepare) into tab[j], with its scratch offset behind
// the table and its info words at the prefix sums of d_j + 3.  *shm the largest LDS request, *nt the largest
// thread count, *words the scratch block (the table first).  who null: the planner, out and info not examined.
int rm_plan(const char *who, int njobs, const ttk_affine_job *jobs, double *info, RtManyJob *tab, int64_t *shm,
            int *nt, int64_t *words, int64_t *info_off) {
  if (njobs < 1 || njobs > TTK_ROUND_MANY_MAX || !jobs || (who && !info)) {
    if (who) ttk::set_error("%s: bad arguments (1 to %d jobs, jobs and info non-null)", who, TTK_ROUND_MANY_MAX);
    return TTK_ERR_ARG;
  }
  int64_t scr = (int64_t)njobs * (int64_t)(sizeof(RtManyJob) / sizeof(double)), off = 0;
  *shm = 0, *nt = 0;
  for (int j = 0; j < njobs; ++j) {
    const ttk_affine_job &b = jobs[j];
    char name[64];
    if (who) snprintf(name, sizeof name, "%s: job %d", who, j);
    int64_t w = 0, s = 0;
    if (const int e = ra_prepare(who ? name : nullptr, RA_RULES, b.d, b.inner, b.rows, b.nterms, b.terms, b.eps,
                                 b.mode, who != nullptr, true, b.out, info ? info + off : nullptr, &tab[j].a, &w, &s))
      return e;
    tab[j].scr = scr;
    scr += tt_even(w > 0 ? w : 2);
    if (info_off) info_off[j] = off;
    off += b.d + 3;
    *shm = s > *shm ? s : *shm;
    *nt = tab[j].a.p.nt > *nt ? tab[j].a.p.nt : *nt;
  }
  if (info_off) info_off[njobs] = off;
  *words = scr;
  return TTK_OK;
}

}  // namespace

extern "C" {

int64_t ttk_retract_lds(int d, const int64_t *inner, const int64_t *ranks, const int64_t *upper) {
  RtPlan p;
  int64_t words;
  const int64_t b = rt_plan(d, inner, ranks, upper, false, &p, &words);
  return b < 0 ? -1 : b;
}

int ttk_retract(ttk_ctx ctx, int d, const double *const *cores, const int64_t *inner, const int64_t *ranks,
                const int64_t *upper, double *const *out, int64_t *out_ranks) {
  ttk::CtxScope scope(ctx);
  RtPlan p;
  int64_t words = 0;
  const int64_t shm = (cores && out && out_ranks) ? rt_plan(d, inner, ranks, upper, false, &p, &words) : -2;
  if (const int e = tt_plan_status(
          shm, "ttk_retract: bad arguments (d >= 2, every rank, extent and upper >= 1, boundary ranks 1)",
          "ttk_retract: the train does not fit one workgroup's LDS (ttk_retract_lds)"))
    return e;
  for (int k = 0; k < d; ++k) {
    if (!cores[k] || !out[k]) {
      ttk::set_error("ttk_retract: null core %d", k);
      return TTK_ERR_ARG;
    }
    p.core[k] = cores[k];
    p.out[k] = out[k];
  }
  TtScratch w(ttk::ctx().stream);  // the orthogonalised cores 1 .. d-1
  TTK_HIP(w.alloc(words));
  tt_lds_attr(retract_kernel<false, RtPlan>, shm);
  hipLaunchKernelGGL((retract_kernel<false, RtPlan>), dim3(1), dim3(p.nt), (size_t)shm, w.st, p, w.get());
  TTK_LAUNCH_CHECK();
  for (int k = 0; k <= d; ++k) out_ranks[k] = p.q[k];
  return TTK_OK;
}

int64_t ttk_round_one_lds(int d, const int64_t *inner, const int64_t *ranks, int64_t *bound) {
  RtPlan p;
  int64_t words;
  const int64_t b = rt_plan(d, inner, ranks, nullptr, true, &p, &words);
  if (b < 0) return -1;
  for (int k = 0; bound && k <= d; ++k) bound[k] = p.q[k];
  return b;
}

int ttk_round_one(ttk_ctx ctx, int d, const double *const *cores, const int64_t *inner, const int64_t *ranks,
                  double eps, int mode, double *const *out, double *info) {
  ttk::CtxScope scope(ctx);
  RtPlan p;
  int64_t words = 0;
  const bool ok = cores && out && info && eps >= 0.0 && eps <= 1.79769313486231570e308 && (mode == 0 || mode == 1);
  const int64_t shm = ok ? rt_plan(d, inner, ranks, nullptr, true, &p, &words) : -2;
  if (const int e = tt_plan_status(shm,
                                   "ttk_round_one: bad arguments (d >= 2, every rank and extent >= 1, boundary ranks "
                                   "1, eps finite and >= 0, mode 0 or 1)",
                                   "ttk_round_one: the train does not fit one workgroup's LDS (ttk_round_one_lds)"))
    return e;
  for (int k = 0; k < d; ++k) {
    if (!cores[k] || !out[k]) {
      ttk::set_error("ttk_round_one: null core %d", k);
      return TTK_ERR_ARG;
    }
    p.core[k] = cores[k];
    p.out[k] = out[k];
  }
  const double e = (mode ? eps / 2.0 : eps) / std::sqrt((double)(d - 1));
  p.thr2 = e * e;
  p.track = mode;
  p.info = info;
  TtScratch w(ttk::ctx().stream);  // the orthogonalised cores 1 .. d-1
  TTK_HIP(w.alloc(words));
  tt_lds_attr(retract_kernel<true, RtPlan>, shm);
  hipLaunchKernelGGL((retract_kernel<true, RtPlan>), dim3(1), dim3(p.nt), (size_t)shm, w.st, p, w.get());
  TTK_LAUNCH_CHECK();
  return TTK_OK;
}

int64_t ttk_sum_round_one_lds(int d, const int64_t *inner, int nterms, const ttk_sum_term *terms, int64_t *sum_ranks,
                              int64_t *bound) {
  ttk_affine_term t[RS_TERMS];
  return ra_lds(d, inner, nterms, rs_terms(nterms, terms, t), true, sum_ranks, bound);
}

int ttk_sum_round_one(ttk_ctx ctx, int d, const int64_t *inner, const int64_t *rows, int nterms,
                      const ttk_sum_term *terms, double eps, int mode, double *const *out, double *info) {
  ttk::CtxScope scope(ctx);
  RtAffineArg a;
  ttk_affine_term t[RS_TERMS];
  int64_t words = 0, shm = 0;
  if (const int e = ra_prepare("ttk_sum_round_one", RS_RULES, d, inner, rows, nterms, rs_terms(nterms, terms, t), eps,
                               mode, true, false, out, info, &a, &words, &shm))
    return e;
  return ra_launch(a, words, shm);
}

int64_t ttk_prod_round_one_lds(int kind, int d, const int64_t *a_ranks, const int64_t *b_ranks, const int64_t *modes,
                               int64_t *prod_ranks, int64_t *bound) {
  ttk_affine_term t;
  int64_t inner[TT_MAXD];
  if (rp_term(kind, d, nullptr, a_ranks, nullptr, b_ranks, modes, &t, inner)) return -1;
  return ra_lds(d, inner, 1, &t, false, prod_ranks, bound);
}

int ttk_prod_round_one(ttk_ctx ctx, int kind, int d, const double *const *a, const int64_t *a_ranks,
                       const double *const *b, const int64_t *b_ranks, const int64_t *modes, double eps, int mode,
                       double *const *out, double *info) {
  ttk::CtxScope scope(ctx);
  const char *who = "ttk_prod_round_one";
  RtAffineArg g;
  ttk_affine_term t;
  int64_t words = 0, shm = 0, inner[TT_MAXD];
  if (const int chk = (a && b) ? rp_term(kind, d, a, a_ranks, b, b_ranks, modes, &t, inner) : -2)
    return ra_fail(who, RP_RULES, chk);
  if (const int e = ra_prepare(who, RP_RULES, d, inner, nullptr, 1, &t, eps, mode, true, false, out, info, &g, &words,
                               &shm))
    return e;
  return ra_launch(g, words, shm);
}

int64_t ttk_affine_round_one_lds(int d, const int64_t *inner, int nterms, const ttk_affine_term *terms,
                                 int64_t *sum_ranks, int64_t *bound) {
  return ra_lds(d, inner, nterms, terms, true, sum_ranks, bound);
}

int ttk_affine_round_one(ttk_ctx ctx, int d, const int64_t *inner, const int64_t *rows, int nterms,
                         const ttk_affine_term *terms, double eps, int mode, double *const *out, double *info) {
  ttk::CtxScope scope(ctx);
  RtAffineArg a;
  int64_t words = 0, shm = 0;
  if (const int e = ra_prepare("ttk_affine_round_one", RA_RULES, d, inner, rows, nterms, terms, eps, mode, true, true,
                               out, info, &a, &words, &shm))
    return e;
  return ra_launch(a, words, shm);
}

int64_t ttk_affine_round_many_lds(int njobs, const ttk_affine_job *jobs, int64_t *info_off, int *threads) {
  RtManyJob tab[TTK_ROUND_MANY_MAX];
  int64_t shm = 0, words = 0;
  int nt = 0;
  if (rm_plan(nullptr, njobs, jobs, nullptr, tab, &shm, &nt, &words, info_off)) return -1;
  for (int j = 0; threads && j < njobs; ++j) threads[j] = tab[j].a.p.nt;
  return shm;
}

int ttk_affine_round_many(ttk_ctx ctx, int njobs, const ttk_affine_job *jobs, double *info) {
  ttk::CtxScope scope(ctx);
  RtManyJob tab[TTK_ROUND_MANY_MAX];
  int64_t shm = 0, words = 0;
  int nt = 0;
  if (const int e = rm_plan("ttk_affine_round_many", njobs, jobs, info, tab, &shm, &nt, &words, nullptr)) return e;
  // one stream-ordered block: the table, then every job's orthogonalised cores
  TtScratch w(ttk::ctx().stream);
  TTK_HIP(w.alloc(words));
  if (const int e = ttk::upload_ring(w.st, reinterpret_cast<const double *>(tab), w.get(),
                                     (int64_t)njobs * (int64_t)(sizeof(RtManyJob) / sizeof(double))))
    return e;
  tt_lds_attr(retract_many_kernel, shm);
  hipLaunchKernelGGL(retract_many_kernel, dim3(njobs), dim3(nt), (size_t)shm, w.st,
                     reinterpret_cast<const RtManyJob *>(w.get()), w.get());
  TTK_LAUNCH_CHECK();
  return TTK_OK;
}

}  // extern "C"
