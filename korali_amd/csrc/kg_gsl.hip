// kg_gsl.hip — kg_gsl.hpp's functions behind two testing entry points, with
// no solver around them (tests/test_gpu_shared_numerics.py).
#include "kg_gsl.hpp"

namespace kg {
namespace {

__global__ void __launch_bounds__(256) k_debug_cholesky(int N, double *A, int *failed) {
  const bool bad = block_cholesky_gsl(A, N, N);
  if (threadIdx.x == 0) *failed = bad ? 1 : 0;
}

__global__ void k_debug_prior_logdens(int kind, double a, double b, const double *__restrict__ x, size_t n,
                                      double *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double cn = prior_const(kind, a, b);
  if (e < n) out[e] = prior_logdens(kind, x[e], a, b, cn);
  if (e == 0) out[n] = cn;
}

}  // namespace
}  // namespace kg

using namespace kg;

extern "C" int kg_debug_cholesky(int device, size_t N, const double *in, double *out, int *failed) {
  KG_CHECK(in && out && failed, "kg_debug_cholesky: null argument");
  KG_CHECK(N >= 1 && N <= 1024, "kg_debug_cholesky: 1 <= N <= 1024");
  KG_HIP(hipSetDevice(device));
  const size_t nb = N * N * sizeof(double);
  double *d = nullptr;
  KG_HIP(dev_alloc(&d, nb + sizeof(int)));
  int *f = (int *)(d + N * N);
  int rc = hipMemcpy(d, in, nb, hipMemcpyHostToDevice) != hipSuccess;
  if (!rc) {
    hipLaunchKernelGGL(k_debug_cholesky, dim3(1), dim3(256), 0, 0, (int)N, d, f);
    rc = hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
         hipMemcpy(out, d, nb, hipMemcpyDeviceToHost) != hipSuccess ||
         hipMemcpy(failed, f, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess;
  }
  dev_release(d);
  if (rc) set_error("kg_debug_cholesky: device call failed");
  return rc;
}

extern "C" int kg_debug_prior_logdens(int device, int kind, double a, double b, const double *x, size_t n,
                                      double *out_const, double *out) {
  KG_CHECK(x && out_const && out, "kg_debug_prior_logdens: null argument");
  KG_CHECK(kind >= KG_PRIOR_UNIFORM && kind <= KG_PRIOR_LOGNORMAL, "kg_debug_prior_logdens: kind out of range");
  KG_CHECK(n >= 1 && n <= (1u << 24), "kg_debug_prior_logdens: 1 <= n <= 2^24");
  KG_HIP(hipSetDevice(device));
  upload_dd_tables();
  double *d = nullptr;  // x (n), the densities (n), the constant
  KG_HIP(dev_alloc(&d, (2 * n + 1) * sizeof(double)));
  int rc = hipMemcpy(d, x, n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess;
  if (!rc) {
    hipLaunchKernelGGL(k_debug_prior_logdens, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, kind, a, b,
                       (const double *)d, n, d + n);
    rc = hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
         hipMemcpy(out, d + n, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
         hipMemcpy(out_const, d + 2 * n, sizeof(double), hipMemcpyDeviceToHost) != hipSuccess;
  }
  dev_release(d);
  if (rc) set_error("kg_debug_prior_logdens: device call failed");
  return rc;
}
