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

constexpr int RO_MAXD = 32;                  // cores per train (the plan travels as a kernel argument)
constexpr int64_t RO_LDS_MAX = 160 * 1024;   // bytes one workgroup may declare

struct RoPlan {
  int d, nt;
  int inner[RO_MAXD];   // middle extents; the last one carries the trailing boundary rank
  int r[RO_MAXD + 1];   // train bond ranks   (r[d] = 1 after folding the boundary into inner)
  int s[RO_MAXD + 1];   // sketch bond ranks  (s[d] = 1 likewise)
  int q[RO_MAXD + 1];   // output bond ranks
  int woff[RO_MAXD];    // W_k's offset in the scratch block (doubles), k = 1 .. d-1
  int oZ, oC, oY, oQ, oM, oW, oT;  // LDS regions (offsets in doubles, all even: 16-byte aligned)
  const double *core[RO_MAXD];
  const double *sk[RO_MAXD];
  double *out[RO_MAXD];
};

inline int64_t even(int64_t n) { return (n + 1) & ~(int64_t)1; }

// Validates the extents, applies the rank rule and lays out LDS and scratch.  Returns the bytes of
// dynamic LDS, -1 when the train does not fit one workgroup (or has more than RO_MAXD cores), -2 on
// invalid arguments.  *wwords: doubles of scratch for W_1 .. W_{d-1}.
int64_t ro_plan(int d, const int64_t *inner, const int64_t *ranks, const int64_t *sranks, RoPlan *p, int64_t *wwords) {
  if (d < 2 || !inner || !ranks || !sranks) return -2;
  for (int k = 0; k <= d; ++k)
    if (ranks[k] < 1 || sranks[k] < 1) return -2;
  for (int k = 0; k < d; ++k)
    if (inner[k] < 1) return -2;
  if (ranks[d] != sranks[d]) return -2;  // the last cores are contracted over (n_{d-1}, r_d) together
  if (d > RO_MAXD) return -1;
  const int64_t cap = RO_LDS_MAX / 8;  // no single extent or product may pass the LDS capacity
  int64_t n[RO_MAXD], r[RO_MAXD + 1], s[RO_MAXD + 1], q[RO_MAXD + 1];
  for (int k = 0; k < d; ++k) n[k] = inner[k];
  for (int k = 0; k <= d; ++k) {
    r[k] = ranks[k];
    s[k] = sranks[k];
    if (r[k] > cap || s[k] > cap) return -1;
  }
  if (n[d - 1] > cap) return -1;
  n[d - 1] *= r[d];
  r[d] = s[d] = 1;
  for (int k = 0; k < d; ++k)
    if (n[k] > cap) return -1;
  q[0] = r[0];
  for (int i = 0; i + 1 < d; ++i) {
    const int64_t m = q[i] * n[i];  // <= cap * cap: no overflow
    if (m > cap) return -1;
    q[i + 1] = m < s[i + 1] ? m : s[i + 1];
  }
  q[d] = 1;
  int64_t zZ = 2, zC = 2, zY = 2, zQ = 2, zM = 2, zW = 2, zT = 2, ww = 0;
  auto up = [&](int64_t &z, int64_t a, int64_t b, int64_t c) {  // z = max(z, a b c), saturating at cap + 1
    int64_t v = a * b;
    v = v > cap ? cap + 1 : v * c;
    v = v > cap ? cap + 1 : v;
    z = v > z ? v : z;
  };
  for (int i = 0; i < d; ++i) up(zZ, q[i], n[i], r[i + 1]);          // carried core
  for (int k = 1; k < d; ++k) {
    up(zZ, s[k], n[k], s[k + 1]);                                     // sketch core (phase A)
    up(zC, r[k], n[k], r[k + 1]);                                     // train core
    up(zY, r[k], n[k], s[k + 1]);                                     // A_k W_{k+1}
    up(zW, r[k], s[k], 1);
    if (p) p->woff[k] = (int)ww;
    ww += even(r[k] * s[k] > cap ? cap + 1 : r[k] * s[k]);
    if (ww > ((int64_t)1 << 30)) return -1;
  }
  for (int i = 0; i + 1 < d; ++i) {
    up(zY, q[i], n[i], s[i + 1]);                                     // Y
    up(zQ, q[i], n[i], q[i + 1]);                                     // Q
    up(zM, q[i + 1], r[i + 1], 1);                                    // Q^T Z
    up(zT, q[i + 1], 1, 1);                                           // tau
  }
  const int64_t total = even(zZ) + even(zC) + even(zY) + even(zQ) + even(zM) + even(zW) + even(zT);
  if (total * 8 > RO_LDS_MAX) return -1;
  if (wwords) *wwords = ww;
  if (p) {
    p->d = d;
    for (int k = 0; k < d; ++k) p->inner[k] = (int)n[k];
    for (int k = 0; k <= d; ++k) {
      p->r[k] = (int)r[k];
      p->s[k] = (int)s[k];
      p->q[k] = (int)q[k];
    }
    int64_t o = 0;
    p->oZ = (int)o, o += even(zZ);
    p->oC = (int)o, o += even(zC);
    p->oY = (int)o, o += even(zY);
    p->oQ = (int)o, o += even(zQ);
    p->oM = (int)o, o += even(zM);
    p->oW = (int)o, o += even(zW);
    p->oT = (int)o;
    const int64_t work = zY > zZ ? zY : zZ;
    p->nt = work <= 2048 ? 256 : 1024;  // small trains: fewer waves at each barrier
  }
  return total * 8;
}

__global__ __launch_bounds__(1024) void rand_orth_kernel(const RoPlan p, double *wscr) {
  extern __shared__ __attribute__((aligned(16))) double ro_lds[];
  double *Z = ro_lds + p.oZ, *C = ro_lds + p.oC, *Y = ro_lds + p.oY, *Qc = ro_lds + p.oQ, *Mq = ro_lds + p.oM,
         *W = ro_lds + p.oW, *tau = ro_lds + p.oT;
  const int d = p.d;
  // ---- phase A: W_d = [1]; W_k = unfold(A_k W_{k+1}) unfold(B_k)^T, k = d-1 .. 1
  if (threadIdx.x == 0) W[0] = 1.0;
  for (int k = d - 1; k >= 1; --k) {
    const int rk = p.r[k], n = p.inner[k], r1 = p.r[k + 1], sk = p.s[k], s1 = p.s[k + 1];
    ro_load(C, p.core[k], rk * n * r1);
    ro_load(Z, p.sk[k], sk * n * s1);  // the sketch core borrows the carried core's region
    __syncthreads();
    // T (r_k n x s_{k+1}) = A_k (r_k n x r_{k+1}) W_{k+1} (r_{k+1} x s_{k+1})
    ro_gemm(rk * n, s1, r1, [&](int i, int c) { return C[i * r1 + c]; }, [&](int c, int j) { return W[c * s1 + j]; },
            [&](int i, int j, double v) { Y[i * s1 + j] = v; });
    __syncthreads();
    // W_k (r_k x s_k) = T (r_k x n s_{k+1}) B_k (s_k x n s_{k+1})^T
    const int K = n * s1;
    double *wk = wscr + p.woff[k];
    ro_gemm(rk, sk, K, [&](int i, int c) { return Y[i * K + c]; }, [&](int c, int j) { return Z[j * K + c]; },
            [&](int i, int j, double v) {
              W[i * sk + j] = v;
              wk[i * sk + j] = v;
            });
    __syncthreads();
  }
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
  const int64_t b = ro_plan(d, inner, ranks, sketch_ranks, nullptr, nullptr);
  return b < 0 ? -1 : b;
}

int ttk_rand_orth(ttk_ctx ctx, int d, const double *const *cores, const int64_t *inner, const int64_t *ranks,
                  const double *const *sketch, const int64_t *sketch_ranks, double *const *out, int64_t *out_ranks) {
  ttk::CtxScope scope(ctx);
  hipStream_t st = ttk::ctx().stream;
  RoPlan p;
  int64_t wwords = 0;
  const int64_t shm = (cores && sketch && out && out_ranks) ? ro_plan(d, inner, ranks, sketch_ranks, &p, &wwords) : -2;
  if (shm == -2) {
    ttk::set_error("ttk_rand_orth: bad arguments (d >= 2, every rank and extent >= 1, equal trailing ranks)");
    return TTK_ERR_ARG;
  }
  if (shm < 0) {
    ttk::set_error("ttk_rand_orth: the train does not fit one workgroup's LDS (ttk_rand_orth_lds)");
    return TTK_ERR_ARG;
  }
  for (int k = 0; k < d; ++k) {
    if (!cores[k] || !out[k] || (k > 0 && !sketch[k])) {
      ttk::set_error("ttk_rand_orth: null core %d", k);
      return TTK_ERR_ARG;
    }
    p.core[k] = cores[k];
    p.sk[k] = sketch[k];
    p.out[k] = out[k];
  }
  void *w = nullptr;  // W_1 .. W_{d-1}: one stream-ordered block per call
  TTK_HIP(hipMallocAsync(&w, (size_t)(wwords > 0 ? wwords : 2) * sizeof(double), st));
  if (shm > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(rand_orth_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  hipLaunchKernelGGL(rand_orth_kernel, dim3(1), dim3(p.nt), (size_t)shm, st, p, static_cast<double *>(w));
  const hipError_t le = hipGetLastError();
  (void)hipFreeAsync(w, st);
  ttk::note_launch();
  if (le != hipSuccess) {
    ttk::set_error("%s:%d launch: %s", __FILE__, __LINE__, hipGetErrorString(le));
    return TTK_ERR_HIP;
  }
  for (int k = 0; k < d; ++k) out_ranks[k] = p.q[k];
  out_ranks[d] = ranks[d];
  return TTK_OK;
}

}  // extern "C"
