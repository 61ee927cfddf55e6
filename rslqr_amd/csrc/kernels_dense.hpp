// kernels_dense.hpp -- the kernels behind the dense Matrix* helpers (ndlqr_hip_gemm / potrf / potrs / trsv,
// hip_dense.hip): the reference's internal routines (src/linalg_custom.c), one element / column per thread.
#pragma once
#include <hip/hip_runtime.h>

namespace ndlqr {

// ------------------------------------------------------------------------------------- dense helpers
// Device versions of the reference's internal routines, one element / column per thread.
// C = alpha*op(A)*op(B) + beta*C  (linalg_custom.c:20-43): beta first, then k ascending.
static __global__ void dense_gemm(int tA, int tB, int m, int n, int k, double alpha, const double* A, int lda,
                           const double* B, int ldb, double beta, double* C, int ldc) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * n) return;
  const int i = e % m, j = e / m;
  double acc = C[i + (size_t)ldc * j] * beta;
  for (int p = 0; p < k; ++p) {
    const double a = tA ? A[p + (size_t)lda * i] : A[i + (size_t)lda * p];
    const double bv = tB ? B[j + (size_t)ldb * p] : B[p + (size_t)ldb * j];
    acc = acc + (alpha * a) * bv;
  }
  C[i + (size_t)ldc * j] = acc;
}

// in-place lower Cholesky (linalg_custom.c:88-111); single block.
static __global__ void dense_potrf(int n, double* A, int lda, int* info) {
  for (int j = 0; j < n; ++j) {
    for (int i = j + threadIdx.x; i < n; i += blockDim.x) {
      double acc = A[i + (size_t)lda * j];
      for (int k = 0; k < j; ++k) acc = acc - A[i + (size_t)lda * k] * A[j + (size_t)lda * k];
      A[i + (size_t)lda * j] = acc;
    }
    __syncthreads();
    const double pivot = A[j + (size_t)lda * j];
    if (!(pivot > 0.0)) {
      if (threadIdx.x == 0) *info = j + 1;
      return;
    }
    const double root = sqrt(pivot);
    __syncthreads();
    for (int i = j + threadIdx.x; i < n; i += blockDim.x) A[i + (size_t)lda * j] /= root;
    __syncthreads();
  }
}

// L L' x = b (linalg_custom.c:113-138); one thread per right-hand side. which = 1: the forward substitution
// alone (L x = b), 2: the transposed one alone (L' x = b) -- clap_LowerTriBackSub.
static __global__ void dense_potrs(int n, int nrhs, const double* L, int ldl, double* B, int ldb, int which) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nrhs) return;
  double* x = B + (size_t)ldb * c;
  if (which != 2)
    for (int j = 0; j < n; ++j) {
      const double xj = x[j] / L[j + (size_t)ldl * j];
      x[j] = xj;
      for (int i = j + 1; i < n; ++i) x[i] = x[i] - L[i + (size_t)ldl * j] * xj;
    }
  if (which != 1)
    for (int j = n - 1; j >= 0; --j) {
      const double xj = x[j] / L[j + (size_t)ldl * j];
      x[j] = xj;
      for (int i = 0; i < j; ++i) x[i] = x[i] - L[j + (size_t)ldl * i] * xj;
    }
}

}  // namespace ndlqr
