// Products, loads, the Householder QR and the one-sided Jacobi round shared by the one-workgroup TT
// kernels (ttk_randorth.hip, ttk_nystroem.hip, ttk_retract.hip).
// The summation order is part of their contract: one ascending-k fma chain per output element.
#pragma once
#include <hip/hip_runtime.h>

#include "ttk_common.h"

// C(i, j) = sum_k a(i, k) b(k, j), k ascending in one fma chain from 0; element e = i N + j goes to
// thread e mod blockDim.x.
template <class FA, class FB, class FC>
__device__ __forceinline__ void ro_gemm(int M, int N, int K, FA a, FB b, FC store) {
  for (int e = threadIdx.x; e < M * N; e += blockDim.x) {
    const int i = e / N, j = e - i * N;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = fma(a(i, k), b(k, j), acc);
    store(i, j, acc);
  }
}

__device__ __forceinline__ void ro_load(double *dst, const double *src, int n) {
  for (int e = threadIdx.x; e < n; e += blockDim.x) dst[e] = src[e];
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
__device__ void ro_householder(double *Y, int m, int n, double *tau) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
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

// Qc (m x k, column-major, in LDS) = H_0 ... H_{k-1} [I_k; 0] from the reflectors ro_householder left
// in Y.  Column c only meets the reflectors j = c, c-1, ..., 0, so a wave takes whole columns through
// all their reflectors with no workgroup barrier in between.  Ends with a barrier.
__device__ void ro_form_q(const double *Y, const double *tau, int m, int k, double *Qc) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int e = threadIdx.x; e < m * k; e += blockDim.x) {
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

// One sweep-round of the one-sided Jacobi on the rows of A (p x n) with the rotations accumulated in
// G (p x p): the round's disjoint pairs (circle method over m = p rounded up to even players, the
// last one fixed) go to the waves in turn.  A pair (i, j) is rotated when |<a_i, a_j>| exceeds
// tol ||a_i|| ||a_j||.  Returns after a workgroup barrier.
__device__ void ny_jacobi_round(double *A, double *G, int p, int n, int m, int round, double tol2, int *flag) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
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

}  // namespace
