// Products and loads shared by the one-workgroup TT kernels (ttk_randorth.hip, ttk_nystroem.hip).
// The summation order is part of their contract: one ascending-k fma chain per output element.
#pragma once
#include <hip/hip_runtime.h>

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
