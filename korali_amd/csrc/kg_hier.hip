// kg_hier.hip — the Hierarchical/Psi, Hierarchical/ThetaNew and Hierarchical/
// Theta log-likelihoods (problem/hierarchical/psi/psi.cpp.base:120-141,
// thetaNew/thetaNew.cpp.base:35-54, theta/theta.cpp.base:59-124) on the device,
// for kg_tmcmc_* handles.
//
// All are  LL(c) = sum_{g<G} [ LSE_{j<K_g}( base_{g,j} + sum_{k<D} logdens_k ) ]
// (ThetaNew: G = 1 and -log(M) in front; Theta: as ThetaNew with row j's
// precomputed denominator subtracted from its term and the sub-problem's own
// log-likelihood in front; Theta's denominators: one point per Psi row over
// the sub-experiment's samples, their log-prior subtracted last and -log(K) in
// front), with logSumExp as auxiliar/math.hpp:
// 205-225 writes it: max by `>`, +-inf returned as it is, else the exponentials
// of (v_j - max) added from 0.0 in j order, max + log(sum).
//
// One workgroup per (point, group).  Pass 1 forms every v_j (rows strided over
// the 256 lanes, columns of the database stored one after the other so a
// wavefront reads consecutive doubles) and reduces the max; NaN never wins a
// `>` and which of two equal values wins does not change a bit of the result.
// Pass 2 forms the terms again, one tile of 256 rows at a time, leaves
// exp_cr(v_j - max) in LDS, and lane 0 adds the tile in row order while the
// other wavefronts already work on the next tile (two LDS tiles, one barrier
// per tile).  The P x G group values go to a scratch array; k_hier_finish adds
// them per point in group order.  Nothing waits on another workgroup and every
// loop is bounded by a group's size.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/korali_amd.h"
#include "kg_common.hpp"
#include "kg_gsl.hpp"

namespace kg {
namespace hier {

constexpr int MAX_D = 128;  // conditional priors (a TMCMC handle has at most 120 variables)
constexpr int TPB = 256;    // lanes of a workgroup = rows of a tile

// status word: the first offence, lowest chain first (atomicMin);
// chain << 32 | code << 16 | conditional prior; code 0 = invalid parameter,
// 1 = NaN log-posterior of a chain with a finite prior
constexpr unsigned long long ST_CLEAR = ~0ull;

// the fourth workgroup mode, internal: Theta's denominators (theta.cpp.base:64-83)
constexpr int MODE_THETA_DEN = 3;

struct Layout {
  int mode = 0, D = 0, G = 0, W = 0;  // W: doubles per point (Psi: handle's N; ThetaNew: D)
  size_t R = 0;                       // rows of all groups
  int *kind = nullptr;                // D
  int *psrc = nullptr;                // 2 D: variable / column that supplies the parameter, or -1
  double *pconst = nullptr;           // 2 D
  unsigned long long *goff = nullptr; // G + 1 row offsets
  // Psi: x (D x R), log_cr(x) of the LogNormal columns (D x R), base = -logPrior (R)
  // ThetaNew: a, b, constant of every (prior, row) (D x R each)
  double *A = nullptr, *B = nullptr, *Cn = nullptr, *base = nullptr;
  double *part = nullptr;             // rows x G group values of the last evaluation
  size_t partRows = 0;
  double *X = nullptr;                // points of kg_tmcmc_hierarchical_loglik
  double *out = nullptr;
  size_t xRows = 0;
  unsigned long long *status = nullptr, *hStatus = nullptr;
  const double *lastX = nullptr;      // the points the last evaluation read (device)
  size_t lastLd = 0;
  double negLogM = 0.0;               // ThetaNew, Theta: -log(M)
  // Theta: row r's precomputed denominator (R), the sub-problem's
  // log-likelihoods of kg_tmcmc_theta_loglik (xRows), and the stream the
  // group kernel of a host-fed round runs on beside the handle's
  double *den = nullptr, *sub = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool sidePending = false;
};

// prior_const of a conditional prior, whose parameters may come from a
// sample: a Uniform of no or negative width has the constant NaN here (the
// guard is this file's alone)
__device__ __forceinline__ double conditional_const(int kind, double a, double b) {
  const double cn = prior_const(kind, a, b);
  return (kind == KG_PRIOR_UNIFORM && b - a <= 0.0) ? (double)NAN : cn;
}

// set-up: Psi — log_cr of the LogNormal columns; ThetaNew — every row's
// parameters and constants
__global__ void k_hier_setup(int mode, int D, size_t R, int W, const int *__restrict__ kind,
                             const int *__restrict__ psrc, const double *__restrict__ pconst,
                             const double *__restrict__ rows, double *__restrict__ A, double *__restrict__ B,
                             double *__restrict__ Cn) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)D * R) return;
  const int k = (int)(e / R);
  const size_t r = e % R;
  if (mode == KG_HIER_PSI) {
    const double x = rows[r * W + k];
    A[e] = x;
    B[e] = (kind[k] == KG_PRIOR_LOGNORMAL && x > 0) ? log_cr(x) : 0.0;
  } else {
    const double a = psrc[2 * k] >= 0 ? rows[r * W + psrc[2 * k]] : pconst[2 * k];
    const double b = psrc[2 * k + 1] >= 0 ? rows[r * W + psrc[2 * k + 1]] : pconst[2 * k + 1];
    A[e] = a;
    B[e] = b;
    Cn[e] = conditional_const(kind[k], a, b);
  }
}

template <int MODE>
__global__ void __launch_bounds__(TPB) k_hier_group(int D, int G, int W, size_t R, size_t npts, size_t ld,
                                                   const double *__restrict__ X, const unsigned char *__restrict__ pend,
                                                   const double *__restrict__ lp, const int *__restrict__ kind,
                                                   const int *__restrict__ psrc, const double *__restrict__ pconst,
                                                   const unsigned long long *__restrict__ goff,
                                                   const double *__restrict__ A, const double *__restrict__ B,
                                                   const double *__restrict__ Cn, const double *__restrict__ base,
                                                   const double *__restrict__ den, const double *__restrict__ pA,
                                                   const double *__restrict__ pB, const double *__restrict__ pCn,
                                                   size_t pR, double *__restrict__ part,
                                                   unsigned long long *status) {
  __shared__ double sa[MAX_D], sb[MAX_D], sc[MAX_D];
  __shared__ int sk[MAX_D];
  __shared__ double tile[2][TPB];
  __shared__ double red[TPB];
  const size_t c = blockIdx.x / (unsigned)G;
  const int g = (int)(blockIdx.x % (unsigned)G);
  if (c >= npts) return;
  if (pend && !pend[c]) return;
  if (lp && isinf(lp[c]) && lp[c] < 0) return;  // hierarchical.cpp.base:39-43: not evaluated
  const int t = threadIdx.x;
  const double *x = X + c * ld;
  for (int k = t; k < D; k += TPB) {
    sk[k] = kind[k];
    if (MODE == MODE_THETA_DEN) {  // Psi row c's conditional priors, as k_hier_setup left them
      sa[k] = pA[(size_t)k * pR + c];
      sb[k] = pB[(size_t)k * pR + c];
      sc[k] = pCn[(size_t)k * pR + c];
    } else if (MODE == KG_HIER_PSI) {  // updateConditionalPriors (psi.cpp.base:110-118)
      const double a = psrc[2 * k] >= 0 ? x[psrc[2 * k]] : pconst[2 * k];
      const double b = psrc[2 * k + 1] >= 0 ? x[psrc[2 * k + 1]] : pconst[2 * k + 1];
      sa[k] = a;
      sb[k] = b;
      sc[k] = conditional_const(sk[k], a, b);
      if (g == 0 && prior_scale_invalid(sk[k], b))
        atomicMin(status, ((unsigned long long)c << 32) | (unsigned long long)k);
    } else {  // the point itself and, for LogNormal priors, its logarithm
      const double v = x[k];
      sa[k] = v;
      sb[k] = (sk[k] == KG_PRIOR_LOGNORMAL && v > 0) ? log_cr(v) : 0.0;
    }
  }
  __syncthreads();
  const size_t r0 = goff[g];
  const size_t K = goff[g + 1] - r0;
  auto value = [&](size_t j) -> double {
    const size_t r = r0 + j;
    double v;
    if (MODE == KG_HIER_PSI) {
      v = base[r];  // psi.cpp.base:132
      for (int k = 0; k < D; k++) v += prior_logdens(sk[k], A[(size_t)k * R + r], B[(size_t)k * R + r], sa[k], sb[k], sc[k]);
    } else if (MODE == MODE_THETA_DEN) {
      v = 0.;  // theta.cpp.base:73-77: the sub-sample's log-prior (base, not negated) comes off last
      for (int k = 0; k < D; k++) v += prior_logdens(sk[k], A[(size_t)k * R + r], B[(size_t)k * R + r], sa[k], sb[k], sc[k]);
      v -= base[r];
    } else {
      v = 0.;  // thetaNew.cpp.base:48, theta.cpp.base:116
      for (int k = 0; k < D; k++)
        v += prior_logdens(sk[k], sa[k], sb[k], A[(size_t)k * R + r], B[(size_t)k * R + r], Cn[(size_t)k * R + r]);
      if (MODE == KG_HIER_THETA) v -= den[r];  // theta.cpp.base:120
    }
    return v;
  };
  // math.hpp:207-210
  double m = -INFINITY;
  for (size_t j = t; j < K; j += TPB) {
    const double v = value(j);
    if (v > m) m = v;
  }
  red[t] = m;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (t < s && red[t + s] > red[t]) red[t] = red[t + s];
    __syncthreads();
  }
  m = red[0];
  if (isinf(m)) {  // :212-218
    if (t == 0) part[c * G + g] = m;
    return;
  }
  // :220-224
  double sum = 0.0;
  const size_t tiles = (K + TPB - 1) / TPB;
  for (size_t q = 0; q < tiles; q++) {
    const size_t j = q * TPB + t;
    double *buf = tile[q & 1];
    if (j < K) buf[t] = exp_cr(value(j) - m);
    __syncthreads();
    if (t == 0) {
      const int n = (int)min((size_t)TPB, K - q * TPB);
      for (int i = 0; i < n; i++) sum += buf[i];
    }
  }
  if (t == 0) part[c * G + g] = m + log_cr(sum);
}

// psi.cpp.base:124,137 (0.0, += each group) / thetaNew.cpp.base:53
// (-log(M) + lse; Theta's denominators theta.cpp.base:80 likewise with
// -log(K)) / theta.cpp.base:123 ((subLL - log(M)) + lse; subll may be out
// itself, or null for 0.0); hierarchical.cpp.base:51: a NaN log-posterior is
// an error
__global__ void k_hier_finish(int mode, int G, size_t npts, double negLogM, const unsigned char *__restrict__ pend,
                              const double *__restrict__ lp, const double *__restrict__ part, const double *subll,
                              double *out, unsigned long long *status) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= npts) return;
  if (pend && !pend[c]) return;
  if (lp && isinf(lp[c]) && lp[c] < 0) return;  // k_tm_evaluate left -inf
  double ll;
  if (mode == KG_HIER_PSI) {
    ll = 0.0;
    for (int g = 0; g < G; g++) ll += part[c * G + g];
  } else if (mode == KG_HIER_THETA) {
    ll = ((subll ? subll[c] : 0.0) + negLogM) + part[c];
  } else {
    ll = negLogM + part[c];
  }
  out[c] = ll;
  if (lp && isnan(lp[c] + ll)) atomicMin(status, ((unsigned long long)c << 32) | (1ull << 16));
}

// -log(M) as thetaNew.cpp.base:53 writes it
__global__ void k_hier_neglog(double M, double *out) { out[0] = -log_cr(M); }

inline unsigned nblocks(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// the group values of npts points X (ld doubles apart) into L.part; pend / lp
// as the handle's pending mask and log-priors, or null (every point, prior not
// consulted)
inline int group(Layout &L, const double *X, size_t ld, size_t npts, const unsigned char *pend, const double *lp,
                 hipStream_t stream) {
  KG_CHECK(npts * (size_t)L.G < 0x7fffffffull, "hierarchical likelihood: too many (point, group) pairs");
  if (L.partRows < npts) {
    if (L.part) dev_release(L.part, stream);
    L.part = nullptr;
    KG_HIP(dev_alloc(&L.part, npts * (size_t)L.G * sizeof(double)));
    L.partRows = npts;
  }
  const unsigned grid = (unsigned)(npts * (size_t)L.G);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(TPB), 0, stream, L.D, L.G, L.W, L.R, npts, ld, X, pend, lp, L.kind,
                       L.psrc, L.pconst, L.goff, L.A, L.B, L.Cn, L.base, L.den, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, (size_t)0, L.part, L.status);
  };
  if (L.mode == KG_HIER_PSI)
    launch(k_hier_group<KG_HIER_PSI>);
  else if (L.mode == KG_HIER_THETA)
    launch(k_hier_group<KG_HIER_THETA>);
  else
    launch(k_hier_group<KG_HIER_THETANEW>);
  KG_HIP(hipGetLastError());
  L.lastX = X;
  L.lastLd = ld;
  return 0;
}

// the points' LL from L.part into out (Theta: subll, the sub-problem's own
// log-likelihoods, in front)
inline int finish(Layout &L, size_t npts, const unsigned char *pend, const double *lp, const double *subll,
                  double *out, hipStream_t stream) {
  hipLaunchKernelGGL(k_hier_finish, dim3(nblocks(npts, 128)), dim3(128), 0, stream, L.mode, L.G, npts, L.negLogM, pend,
                     lp, L.part, subll, out, L.status);
  KG_HIP(hipGetLastError());
  return 0;
}

// LL of npts points X into out, both launches on one stream
inline int evaluate(Layout &L, const double *X, size_t ld, size_t npts, const unsigned char *pend, const double *lp,
                    const double *subll, double *out, hipStream_t stream) {
  if (npts == 0) return 0;
  if (group(L, X, ld, npts, pend, lp, stream)) return 1;
  return finish(L, npts, pend, lp, subll, out, stream);
}

// Theta's denominators (theta.cpp.base:64-83) into L.den: one point per Psi
// row, one group of K sub-samples whose columns S / logS (D x K) and
// log-priors lpS (K) the caller holds; negLogK = -log_cr(K)
inline int denominators(Layout &L, size_t K, const double *S, const double *logS, const double *lpS,
                        const unsigned long long *goffK, double negLogK, double *part, hipStream_t stream) {
  KG_CHECK(L.R < 0x7fffffffull, "hierarchical likelihood: too many (point, group) pairs");
  hipLaunchKernelGGL(k_hier_group<MODE_THETA_DEN>, dim3((unsigned)L.R), dim3(TPB), 0, stream, L.D, 1, L.D, K, L.R,
                     (size_t)0, (const double *)nullptr, (const unsigned char *)nullptr, (const double *)nullptr, L.kind,
                     L.psrc, L.pconst, goffK, S, logS, (const double *)nullptr, lpS, (const double *)nullptr, L.A, L.B,
                     L.Cn, L.R, part, L.status);
  hipLaunchKernelGGL(k_hier_finish, dim3(nblocks(L.R, 128)), dim3(128), 0, stream, (int)MODE_THETA_DEN, 1, L.R, negLogK,
                     (const unsigned char *)nullptr, (const double *)nullptr, part, (const double *)nullptr, L.den,
                     L.status);
  KG_HIP(hipGetLastError());
  return 0;
}

inline void release(Layout &L) {
  if (L.side) (void)hipStreamSynchronize(L.side);  // its last group kernel reads the arrays below
  if (L.fork) (void)hipEventDestroy(L.fork);
  if (L.join) (void)hipEventDestroy(L.join);
  if (L.side) (void)hipStreamDestroy(L.side);
  for (void *p : {(void *)L.kind, (void *)L.psrc, (void *)L.pconst, (void *)L.goff, (void *)L.A, (void *)L.B,
                  (void *)L.Cn, (void *)L.base, (void *)L.part, (void *)L.X, (void *)L.out, (void *)L.status,
                  (void *)L.den, (void *)L.sub})
    if (p) dev_release(p);
  if (L.hStatus) host_release(L.hStatus);
  L = Layout();
}

}  // namespace hier
}  // namespace kg
