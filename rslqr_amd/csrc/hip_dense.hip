// hip_dense.hip -- the dense Matrix* helpers (ndlqr_hip_gemm / potrf_lower / potrs_lower / trsv_lower) with their
// scratch lease: the host side, the kernels of kernels_dense.hpp. They need no context.
#include <mutex>

#include "hip_host.hpp"
#include "kernels_dense.hpp"

// ------------------------------------------------------------------------------ dense helpers

// Host matrices in, host matrices out (the reference's Matrix* layer, src/linalg.c:55-190). One call = one
// packed H2D copy of the operands, one kernel, one D2H copy of the result, all on the stream of a pooled
// scratch (a device buffer + a pinned staging buffer, grown on demand): no allocation and no blocking
// null-stream copy per call, and calls from different host threads (the reference's tests call these from
// an OpenMP team, test/parallel_test.c:30-239) run side by side on different scratches.
namespace {
struct DenseScratch {
  DevBuf<double> dev;       // both of one capacity, grown on demand
  PinnedBuf<double> host;
  hipStream_t stream = nullptr;
  int device = -1;  // the device its stream and buffer live on: leased only to calls whose current device is this one
};
std::mutex g_dense_mu;
std::vector<DenseScratch*> g_dense_pool;  // idle scratches; never freed (bounded by the peak concurrency)

struct DenseLease {
  DenseScratch* s = nullptr;
  DenseLease() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::lock_guard<std::mutex> lock(g_dense_mu);
    for (size_t i = g_dense_pool.size(); i-- > 0;)
      if (g_dense_pool[i]->device == dev) {
        s = g_dense_pool[i];
        g_dense_pool.erase(g_dense_pool.begin() + (long)i);
        return;
      }
    s = new DenseScratch();
    s->device = dev;
  }
  ~DenseLease() {
    std::lock_guard<std::mutex> lock(g_dense_mu);
    g_dense_pool.push_back(s);
  }
  int ensure(size_t doubles) {
    if (!s->stream) HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    size_t cap = s->host.count() ? s->host.count() : 4096;
    while (cap < doubles) cap *= 2;
    HIP_TRY(s->dev.grow(cap));
    HIP_TRY(s->host.grow(cap));
    return NDLQR_OK;
  }
};
}  // namespace

static int dense_ready() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    refuse("no HIP device for the dense Matrix* helpers (no CPU fallback)");
    return NDLQR_ERR_NO_DEVICE;
  }
  return NDLQR_OK;
}

int ndlqr_hip_gemm(int tA, int tB, int m, int n, int k, double alpha, const double* A, int lda,
                   const double* B, int ldb, double beta, double* C, int ldc) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (m <= 0 || n <= 0 || k < 0 || !A || !B || !C) return NDLQR_ERR_INVALID;
  // stored shapes: A is (Ar x Ac) with leading dimension lda, ...; the last column ends after its rows
  const int Ar = tA ? k : m, Ac = tA ? m : k, Br = tB ? n : k, Bc = tB ? k : n;
  if (k > 0 && (lda < Ar || ldb < Br)) return NDLQR_ERR_INVALID;
  if (ldc < m) return NDLQR_ERR_INVALID;
  const size_t nA = k > 0 ? (size_t)lda * (Ac - 1) + Ar : 0, nB = k > 0 ? (size_t)ldb * (Bc - 1) + Br : 0,
               nC = (size_t)ldc * (n - 1) + m;
  DenseLease L;
  const int err = L.ensure(nA + nB + nC);
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, A, sizeof(double) * nA);
  memcpy(s->host + nA, B, sizeof(double) * nB);
  memcpy(s->host + nA + nB, C, sizeof(double) * nC);
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nA + nB + nC), hipMemcpyHostToDevice, s->stream));
  const int total = m * n;
  hipLaunchKernelGGL(ndlqr::dense_gemm, dim3((total + 255) / 256), dim3(256), 0, s->stream, tA, tB, m, n, k, alpha,
                     s->dev, lda, s->dev + nA, ldb, beta, s->dev + nA + nB, ldc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host + nA + nB, s->dev + nA + nB, sizeof(double) * nC, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(C, s->host + nA + nB, sizeof(double) * nC);
  return NDLQR_OK;
}

int ndlqr_hip_potrf_lower(int n, double* A, int lda) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (n <= 0 || !A) return NDLQR_ERR_INVALID;
  if (lda < n) return NDLQR_ERR_INVALID;
  const size_t nA = (size_t)lda * (n - 1) + n;
  DenseLease L;
  const int err = L.ensure(nA + 1);  // + one slot for the failure word
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, A, sizeof(double) * nA);
  s->host[nA] = 0.0;  // (all-zero bits: the int the kernel writes into starts at 0)
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nA + 1), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(ndlqr::dense_potrf, dim3(1), dim3(256), 0, s->stream, n, s->dev, lda,
                     reinterpret_cast<int*>(s->dev + nA));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host, s->dev, sizeof(double) * (nA + 1), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(A, s->host, sizeof(double) * nA);
  int info = 0;
  memcpy(&info, s->host + nA, sizeof(int));
  return info ? -1 : 0;
}

// which: 0 = L L' x = b (both substitutions), 1 = L x = b, 2 = L' x = b
static int dense_tri_solve(int which, int n, int nrhs, const double* Lm, int ldl, double* B, int ldb) {
  if (dense_ready()) return NDLQR_ERR_NO_DEVICE;
  if (n <= 0 || nrhs <= 0 || !Lm || !B) return NDLQR_ERR_INVALID;
  if (ldl < n || ldb < n) return NDLQR_ERR_INVALID;
  const size_t nL = (size_t)ldl * (n - 1) + n, nB = (size_t)ldb * (nrhs - 1) + n;
  DenseLease L;
  const int err = L.ensure(nL + nB);
  if (err) return err;
  DenseScratch* s = L.s;
  memcpy(s->host, Lm, sizeof(double) * nL);
  memcpy(s->host + nL, B, sizeof(double) * nB);
  HIP_TRY(hipMemcpyAsync(s->dev, s->host, sizeof(double) * (nL + nB), hipMemcpyHostToDevice, s->stream));
  hipLaunchKernelGGL(ndlqr::dense_potrs, dim3((nrhs + 63) / 64), dim3(64), 0, s->stream, n, nrhs, s->dev, ldl,
                     s->dev + nL, ldb, which);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->host + nL, s->dev + nL, sizeof(double) * nB, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  memcpy(B, s->host + nL, sizeof(double) * nB);
  return NDLQR_OK;
}

int ndlqr_hip_potrs_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb) {
  return dense_tri_solve(0, n, nrhs, L, ldl, B, ldb);
}

int ndlqr_hip_trsv_lower(int n, int nrhs, const double* L, int ldl, double* B, int ldb, int transposed) {
  return dense_tri_solve(transposed ? 2 : 1, n, nrhs, L, ldl, B, ldb);
}
