// kg_gsl.hpp — the reference numerics more than one solver replays: the
// univariate priors' log-densities (TMCMC, the hierarchical problems, Nested)
// and GSL's Level-2 Cholesky (TMCMC, MOCMAES, Nested).  One expression tree
// each, so the solvers cannot drift apart;
// tests/test_gpu_shared_numerics.py runs them without a solver around them.
#pragma once

#include "../../include/korali_amd.h"
#include "kg_common.hpp"

namespace kg {

// ------------------------------------------------------------------ priors
// a, b: the distribution's two parameters (Uniform: Minimum, Maximum; Normal:
// Mean, Standard Deviation; Exponential: Location, Mean; Laplace: Mean, Width;
// Cauchy: Location, Scale; LogNormal: Mu, Sigma).

// the constant of getLogDensity, as updateDistribution forms it
// (uniform.cpp.base:38-44, normal :42, exponential getLogDensity :16,
// laplace :41, cauchy :41, logNormal :45)
__device__ __forceinline__ double prior_const(int kind, double a, double b) {
  const double pi = 3.14159265358979323846;
  switch (kind) {
    case KG_PRIOR_NORMAL:
    case KG_PRIOR_LOGNORMAL: return -0.5 * log_cr(2 * pi) - log_cr(b);
    case KG_PRIOR_EXPONENTIAL: return -log_cr(b);
    case KG_PRIOR_LAPLACE: return -log_cr(2. * b);
    case KG_PRIOR_CAUCHY: return -log_cr(b * pi);
    default: return -log_cr(b - a);
  }
}

// the updateDistribution checks of the scale parameter (exponential.cpp.base
// has none)
__host__ __device__ __forceinline__ bool prior_scale_invalid(int kind, double b) {
  return (kind == KG_PRIOR_NORMAL || kind == KG_PRIOR_LOGNORMAL || kind == KG_PRIOR_LAPLACE ||
          kind == KG_PRIOR_CAUCHY) && b <= 0.0;
}

// ... and how the reference's error text names that parameter
inline const char *prior_scale_name(int kind) {
  return kind == KG_PRIOR_NORMAL      ? "Standard Deviation parameter of Normal"
         : kind == KG_PRIOR_LOGNORMAL ? "Sigma parameter of LogNormal"
         : kind == KG_PRIOR_LAPLACE   ? "Width parameter of Laplace"
                                      : "Scale parameter of Cauchy";
}

// getLogDensity at x; cn = prior_const(kind, a, b); lx = log_cr(x), read only
// where kind is LogNormal and x > 0
__device__ __forceinline__ double prior_logdens(int kind, double x, double lx, double a, double b, double cn) {
  switch (kind) {
    case KG_PRIOR_NORMAL: {
      const double d = (x - a) / b;
      return cn - 0.5 * d * d;
    }
    case KG_PRIOR_EXPONENTIAL: {  // exponential.cpp.base: -log(mean) - (x - location) / mean
      const double y = x - a;
      return y < 0 ? -INFINITY : cn - y / b;
    }
    case KG_PRIOR_LAPLACE: return cn - fabs(x - a) / b;  // laplace.cpp.base: aux - |x - mean| / width
    case KG_PRIOR_CAUCHY: {  // cauchy.cpp.base: aux - log(1 + (x - loc)^2 / scale^2)
      const double y = x - a;
      return cn - log_cr(1. + y * y / (b * b));
    }
    case KG_PRIOR_LOGNORMAL: {  // logNormal.cpp.base: aux - log x - 0.5 d^2, d = (log x - mu) / sigma
      if (x <= 0) return -INFINITY;
      const double d = (lx - a) / b;
      return cn - lx - 0.5 * d * d;
    }
    default: return (x >= a && x <= b) ? cn : -INFINITY;
  }
}

// the same, forming the logarithm a LogNormal needs
__device__ __forceinline__ double prior_logdens(int kind, double x, double a, double b, double cn) {
  return prior_logdens(kind, x, (kind == KG_PRIOR_LOGNORMAL && x > 0) ? log_cr(x) : 0.0, a, b, cn);
}

// ---------------------------------------------------------------- Cholesky
// gsl_linalg_cholesky_decomp1 (GSL 2.6 linalg/cholesky.c, Level-2 form, with
// gslcblas dgemv order: temp = sum_i x[i] A[r][i] from 0, y += alpha * temp)
// on the lower triangle of the N x N matrix A, in place, rows S doubles
// apart, by one workgroup.  Every thread calls it, after a barrier behind the
// last write to A; on return the last barrier has been passed.  Returns
// whether a pivot was non-positive: the factorisation stops at that column
// and leaves the partial factor, as GSL does with the error handler off
// (engine.cpp:30).  A NaN pivot is not `<= 0` and propagates, as in GSL.
__device__ __forceinline__ bool block_cholesky_gsl(double *A, int N, int S) {
  const int tid = threadIdx.x, nt = blockDim.x;
  // dgemv's alpha, a run-time value there.  Kept one here: folded into a
  // negation, `+= -temp` gives a NaN temp the other sign (the source modifier
  // flips it), where the reference's product leaves the sign alone.
  double alpha = -1.0;
  asm volatile("" : "+v"(alpha));
  for (int j = 0; j < N; j++) {
    if (j > 0) {
      for (int r = j + tid; r < N; r += nt) {
        double temp = 0.0;
        for (int i = 0; i < j; i++) temp += A[j * S + i] * A[r * S + i];
        A[r * S + j] += alpha * temp;
      }
      __syncthreads();
    }
    const double ajj = A[j * S + j];
    if (ajj <= 0.0) return true;
    const double f = 1.0 / sqrt(ajj);
    __syncthreads();  // every thread has read the pivot before its owner scales it
    for (int r = j + tid; r < N; r += nt) A[r * S + j] *= f;
    __syncthreads();
  }
  return false;
}

// ------------------------------------------------------------ small kernels
__global__ void k_fill(double *p, size_t n, double v) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) p[e] = v;
}

}  // namespace kg
