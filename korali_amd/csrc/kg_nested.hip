// kg_nested.hip — nested sampling on the MI355X (Nested.cpp.base, resampling
// methods Box and Ellipse; see include/korali_amd.h for the per-entry-point
// reference map and DESIGN.md §19).
//
// HBM per handle (FP64, sample-major as the reference's vectors):
//   live   L x N  "Live Samples" (unit cube)     cand  B x N  "Candidates"
//   liveLL, liveLP, liveLPW  L                   candLL, candLP, candLPW  B
//   rank[2]  L ints  "Live Samples Rank" (double-buffered by the selection)
//   boxLo, boxUp  N     mean N, cov / invCov / axes N x N, NsEllipse scalars
//   theta  max(L, B) x N  the rows after priorTransform (what a host model reads)
//   z      W x N  the window's normals, scaled in place      tryX  W x N  the window's tries
//   out    2 + 4 + 2 B + B (N + 4) doubles  what one selection hands the host
//   two MtStreams: the Uniform and the Normal Generator.
//
// Host / device split: everything that touches the live set, the bounds or a
// generator runs on the device.  The evidence recurrences are a scalar chain
// per accepted candidate whose exp / log / log1p the reference takes from
// libm, so they run on the host, in the reference's order, on the at most B
// removed rows and (lStar, lStarOld) pairs one selection emits.
//
// Candidate draw: a try consumes a fixed amount of stream (Box: N uniforms;
// Ellipse: N normals and one uniform), so try t of a window is a function of
// the window's words alone.  k_ns_try_* evaluates W tries in parallel,
// k_ns_scan keeps the first B accepted over all windows and records how many
// tries lie before the B-th, and the streams are advanced by exactly those.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/korali_amd.h"
#include "kg_common.hpp"
#include "kg_gsl.hpp"
#include "kg_profile.hpp"
#include "kg_rng.hpp"

namespace kg {

constexpr int NS_TPB = 256;
constexpr int NS_MAXN = 64;
constexpr double NS_LOWEST = -1.7976931348623157e308;  // korali::Lowest
constexpr double NS_MAX = 1.7976931348623157e308;      // korali::Max

struct NsEllipse {
  double det, volume, maxDist, enlargement;
  unsigned int errors;
};

// where a draw stands between two windows
struct NsChain {
  unsigned long long used;       // tries of this window the candidates consume (blocks of N normals / uniforms)
  unsigned long long usedWords;  // Box: used * N uniform words
  int kept;                      // candidates placed so far
  int keptBefore;                // ... before this window
  int done;
};

__global__ void k_ns_prior_const(int N, const double *__restrict__ pmin, const double *__restrict__ pmax,
                                 const int *__restrict__ kind, const double *__restrict__ width,
                                 double *__restrict__ cst, double *__restrict__ logWidth) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  cst[d] = prior_const(kind[d], pmin[d], pmax[d]);
  logWidth[d] = log_cr(width[d]);  // :373
}

// priorTransform (:275-279), evaluateLogPrior (prior_logdens per variable),
// logPriorWeight (:366-376) and the builtin log-likelihood of n rows;
// lik < 0: the caller sets logLikelihood
__global__ void __launch_bounds__(NS_TPB) k_ns_evaluate(int N, int n, int lik, const double *__restrict__ X,
                                                        const double *__restrict__ lower,
                                                        const double *__restrict__ width,
                                                        const double *__restrict__ logWidth,
                                                        const double *__restrict__ pmin,
                                                        const double *__restrict__ pmax,
                                                        const double *__restrict__ cst, const int *__restrict__ kind,
                                                        double *__restrict__ theta, double *__restrict__ LL,
                                                        double *__restrict__ LP, double *__restrict__ LPW) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double *x = X + (size_t)c * N;
  double *t = theta + (size_t)c * N;
  double lp = 0.0, lpw = 0.0, ss = 0.0;
  for (int d = 0; d < N; d++) {
    const double xw = x[d] * width[d];
    const double v = lower[d] + xw;
    t[d] = v;
    const double ld = prior_logdens(kind[d], v, pmin[d], pmax[d], cst[d]);
    lp += ld;
    lpw += ld;
    lpw += logWidth[d];
    ss += v * v;
  }
  LP[c] = lp;
  LPW[c] = lpw;
  if (lik < 0) return;
  // bayesian.cpp.base:61-65: no model evaluation behind a -inf prior
  LL[c] = (isinf(lp) && lp < 0) ? -INFINITY : -0.5 * ss;
}

// the -inf prior rule for caller-set log-likelihoods
__global__ void k_ns_mask_ll(int n, const double *__restrict__ LP, double *__restrict__ LL) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n && isinf(LP[c]) && LP[c] < 0) LL[c] = -INFINITY;
}

// sortLiveSamplesAscending (:506-516) as a rank count: position of i = live
// points before it in (key, index) order
__global__ void __launch_bounds__(NS_TPB) k_ns_sort(int L, const double *__restrict__ LPW,
                                                    const double *__restrict__ LL, int *__restrict__ rank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const double ki = LPW[i] + LL[i];
  int pos = 0;
  for (int j = 0; j < L; j++) {
    const double kj = LPW[j] + LL[j];
    if (kj < ki || (kj == ki && j < i)) pos++;
  }
  rank[pos] = i;
}

// :246-250 after the first sort.  out: [0] accepted, [1] maxEvaluation, [2] lStar, [3] lStarOld
__global__ void k_ns_first_stats(int L, const double *__restrict__ LPW, const double *__restrict__ LL,
                                 const int *__restrict__ rank, double *__restrict__ lstar, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int lo = rank[0], hi = rank[L - 1];
  const double k = LPW[lo] + LL[lo];
  if (isfinite(k)) lstar[0] = k;
  out[0] = 0.0;
  out[1] = LPW[hi] + LL[hi];
  out[2] = lstar[0];
  out[3] = lstar[1];
}

// updateBox (:493-504)
__global__ void __launch_bounds__(64) k_ns_box(int N, int L, const double *__restrict__ live, double *__restrict__ lo,
                                               double *__restrict__ up) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  double mn = NS_MAX, mx = NS_LOWEST;
  for (int i = 0; i < L; i++) {
    const double x = live[(size_t)i * N + d];
    mn = x < mn ? x : mn;  // std::min(mn, x)
    mx = mx < x ? x : mx;  // std::max(mx, x)
  }
  lo[d] = mn;
  up[d] = mx;
}

// updateEllipseMean (:685-699): ordered over the live index
__global__ void __launch_bounds__(64) k_ns_mean(int N, int L, const double *__restrict__ live,
                                                double *__restrict__ mean) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  const double s = ordered_sum(0.0, L, [&](int i) { return live[(size_t)i * N + d]; });
  mean[d] = s / (double)L;
}

// updateEllipseCov (:701-737): one thread per entry (i, j >= i), ordered over
// k; diag: the `num <= dim` branch, which also sets invCov
__global__ void __launch_bounds__(NS_TPB) k_ns_cov(int N, int L, int diag, double weight,
                                                   const double *__restrict__ live, const double *__restrict__ mean,
                                                   double *__restrict__ cov, double *__restrict__ invCov) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= N * N) return;
  const int i = e / N, j = e % N;
  if (diag) {
    if (i != j) {
      cov[e] = 0.0;
      invCov[e] = 0.0;
      return;
    }
    const double m = mean[i];
    const double c = ordered_sum(0.0, L, [&](int k) {
      const double x = live[(size_t)k * N + i] - m;
      return x * x;
    });
    cov[e] = (L == 1) ? 1. : weight * c;
    invCov[e] = (L == 1) ? 1. : 1. / (weight * c);
    return;
  }
  if (j < i) return;
  const double mi = mean[i], mj = mean[j];
  const double c = ordered_sum(0.0, L, [&](int k) {
    const double *x = live + (size_t)k * N;
    return (x[i] - mi) * (x[j] - mj);
  });
  const double v = weight * c;
  cov[i * N + j] = v;
  cov[j * N + i] = v;
}

// The rest of updateEllipseCov and updateEllipseVolume (:739-878) in one
// workgroup: LU with partial pivoting (first maximal pivot, unblocked,
// right-looking) in LDS -> det, invCov column by column (forward, then back
// substitution of the permuted unit vector; one thread per column); the
// Level-2 Cholesky of gsl_linalg_cholesky_decomp1 (block_cholesky_gsl) into
// axes (upper triangle: the original matrix); the largest Mahalanobis distance over the live set;
// the enlargement and the rescalings of :852-875.
__global__ void __launch_bounds__(NS_TPB) k_ns_factor(int N, int L, int diag, const double *__restrict__ live,
                                                      const double *__restrict__ mean, double *__restrict__ cov,
                                                      double *__restrict__ invCov, double *__restrict__ axes,
                                                      double logVolume, double scaling, double K, NsEllipse *el) {
  extern __shared__ double lu[];  // N x N
  __shared__ int perm[NS_MAXN];
  __shared__ double red[NS_TPB];
  __shared__ double sc[3];
  const int tid = threadIdx.x, NN = N * N;
  for (int e = tid; e < NN; e += NS_TPB) {
    const double v = cov[e];
    lu[e] = v;
    axes[e] = v;
  }
  if (tid < N) perm[tid] = tid;
  double signum = 1.0;
  __syncthreads();
  for (int j = 0; j < N; j++) {
    double amax = fabs(lu[j * N + j]);
    int ip = j;
    for (int i = j + 1; i < N; i++) {
      const double a = fabs(lu[i * N + j]);
      if (a > amax) {
        amax = a;
        ip = i;
      }
    }
    __syncthreads();
    if (ip != j) {
      if (tid < N) {
        const double a = lu[j * N + tid];
        lu[j * N + tid] = lu[ip * N + tid];
        lu[ip * N + tid] = a;
      }
      if (tid == 0) {
        const int p = perm[j];
        perm[j] = perm[ip];
        perm[ip] = p;
      }
      signum = -signum;
      __syncthreads();
    }
    const double ajj = lu[j * N + j];
    if (ajj != 0.0) {
      __syncthreads();
      for (int i = j + 1 + tid; i < N; i += NS_TPB) lu[i * N + j] = lu[i * N + j] / ajj;
      __syncthreads();
      const int m = N - j - 1;
      for (int e = tid; e < m * m; e += NS_TPB) {
        const int i = j + 1 + e / m, k = j + 1 + e % m;
        const double p = lu[i * N + j] * lu[j * N + k];
        lu[i * N + k] = lu[i * N + k] - p;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    double det = signum;  // gsl_linalg_LU_det
    for (int i = 0; i < N; i++) det *= lu[i * N + i];
    sc[0] = det;
  }
  if (!diag && tid < N) {
    // column tid of the inverse: x[i] lives in invCov[i * N + tid]
    double *x = invCov + tid;
    for (int i = 0; i < N; i++) x[(size_t)i * N] = perm[i] == tid ? 1.0 : 0.0;
    for (int i = 1; i < N; i++) {
      double tmp = x[(size_t)i * N];
      for (int k = 0; k < i; k++) tmp -= lu[i * N + k] * x[(size_t)k * N];
      x[(size_t)i * N] = tmp;
    }
    x[(size_t)(N - 1) * N] = x[(size_t)(N - 1) * N] / lu[(N - 1) * N + (N - 1)];
    for (int i = N - 2; i >= 0; i--) {
      double tmp = x[(size_t)i * N];
      for (int k = i + 1; k < N; k++) tmp -= lu[i * N + k] * x[(size_t)k * N];
      x[(size_t)i * N] = tmp / lu[i * N + i];
    }
  }
  __syncthreads();
  if (block_cholesky_gsl(axes, N, N)) {  // the lower triangle of axes in place
    if (tid == 0) el->errors |= KG_ERR_CHOLESKY;
    return;
  }
  // mahalanobisDistance (:880-897) of every live point, its maximum from Lowest
  double mx = NS_LOWEST;
  for (int s = tid; s < L; s += NS_TPB) {
    const double *x = live + (size_t)s * N;
    double dist = 0.0;
    for (int i = 0; i < N; i++) {
      double tmp = 0.0;
      for (int k = 0; k < N; k++) tmp += (x[k] - mean[k]) * invCov[i + N * k];
      tmp *= x[i] - mean[i];
      dist += tmp;
    }
    if (dist > mx) mx = dist;
  }
  red[tid] = mx;
  __syncthreads();
  for (int s = NS_TPB / 2; s > 0; s >>= 1) {
    if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
    __syncthreads();
  }
  if (tid == 0) {
    const double det = sc[0], max = red[0], Nd = (double)N;
    const double pointVolume = exp_cr(logVolume) * (double)L / (double)L;  // :861
    const double vol = sqrt(pow_cr(scaling * max, Nd) * det) * K;           // :864
    const double ef =
        vol > pointVolume ? scaling * max : pow_cr((pointVolume * pointVolume) / (K * K * det), 1. / Nd);  // :866
    el->det = det;
    el->maxDist = max;
    el->enlargement = ef;
    el->volume = pow_cr(ef, Nd / 2.) * sqrt(det) * K;  // :867
    sc[1] = ef;
  }
  __syncthreads();
  const double ef = sc[1], inv = 1. / ef, sq = sqrt(ef);
  for (int e = tid; e < NN; e += NS_TPB) {
    cov[e] *= ef;      // :872
    invCov[e] *= inv;  // :873
    axes[e] *= sq;     // :875
  }
}

// generateCandidatesFromBox (:402-411): try t = uniforms [t N, (t + 1) N)
__global__ void __launch_bounds__(NS_TPB) k_ns_try_box(int N, unsigned long long W, const double *__restrict__ u,
                                                       const double *__restrict__ lo, const double *__restrict__ up,
                                                       double *__restrict__ tryX, int *__restrict__ flag) {
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W) return;
  bool ok = true;
  for (int d = 0; d < N; d++) {
    const double w = up[d] - lo[d];
    const double s = u[t * N + d] * w;
    const double x = lo[d] + s;
    tryX[t * N + d] = x;
    if (x < 0. || x > 1.) ok = false;
  }
  flag[t] = ok ? 1 : 0;
}

// generateSampleFromEllipse (:413-434): try t = normals [t N, (t + 1) N) and
// uniform t.  The scaled vector replaces the normals in z.
__global__ void __launch_bounds__(NS_TPB) k_ns_try_ellipse(int N, unsigned long long W, double *__restrict__ z,
                                                           const double *__restrict__ u,
                                                           const double *__restrict__ mean,
                                                           const double *__restrict__ axes,
                                                           double *__restrict__ tryX,
                                                           int *__restrict__ flag) {
  const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W) return;
  double *v = z + t * N;
  double len = 0.0;
  for (int d = 0; d < N; d++) len += v[d] * v[d];
  const double s = pow_cr(u[t], 1. / ((double)N)) / sqrt(len);
  for (int d = 0; d < N; d++) v[d] *= s;
  bool ok = true;
  for (int k = 0; k < N && ok; k++) {
    double x = mean[k];
    for (int l = 0; l < k + 1; l++) x += axes[k * N + l] * v[l];
    tryX[t * N + k] = x;
    if (x < 0. || x > 1.) ok = false;  // the rest of a rejected try is never read
  }
  flag[t] = ok ? 1 : 0;
}

// the first B accepted tries over all windows, one workgroup: sel[c] = the
// window's try that becomes candidate c; used = tries up to the B-th accepted
__global__ void __launch_bounds__(NS_TPB) k_ns_scan(int N, int B, unsigned long long W,
                                                    const int *__restrict__ flag,
                                                    unsigned long long *__restrict__ sel, NsChain *ch) {
  __shared__ unsigned int cnt[NS_TPB];
  __shared__ unsigned long long last;
  const int tid = threadIdx.x;
  const int kept = ch->kept;
  const unsigned long long chunk = (W + NS_TPB - 1) / NS_TPB;
  const unsigned long long t0 = tid * chunk, t1 = t0 + chunk < W ? t0 + chunk : W;
  unsigned int c = 0;
  for (unsigned long long t = t0; t < t1; t++) c += flag[t];
  cnt[tid] = c;
  if (tid == 0) last = W;
  __syncthreads();
  unsigned int before = 0, total = 0;
  for (int q = 0; q < NS_TPB; q++) {
    if (q < tid) before += cnt[q];
    total += cnt[q];
  }
  const unsigned int need = (unsigned int)(B - kept);
  unsigned int r = before;
  for (unsigned long long t = t0; t < t1 && r < need; t++) {
    if (flag[t]) {
      sel[kept + r] = t;
      if (r + 1 == need) last = t + 1;
      r++;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int now = kept + (int)(total < need ? total : need);
    ch->keptBefore = kept;
    ch->kept = now;
    ch->used = last;
    ch->usedWords = last * (unsigned long long)N;
    ch->done = now >= B ? 1 : 0;
  }
}

__global__ void __launch_bounds__(NS_TPB) k_ns_gather(int N, const double *__restrict__ tryX,
                                                      const unsigned long long *__restrict__ sel, const NsChain *ch,
                                                      double *__restrict__ cand) {
  const int lo = ch->keptBefore, n = (ch->kept - lo) * N;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
    const int c = lo + e / N, d = e % N;
    cand[(size_t)c * N + d] = tryX[sel[c] * N + d];
  }
}

// processGeneration's live-set part (:297-353), one workgroup, candidates in
// order.  out: [0] accepted, [1] maxEvaluation, [2] lStar, [3] lStarOld, then
// B pairs (lStar, lStarOld) as they stand after each accepted candidate, then
// the removed rows (N values, logPrior, logPriorWeight, logLikelihood, finite
// flag).  The rank alternates between rk[0] and rk[1]; *cur names the current.
__global__ void __launch_bounds__(NS_TPB) k_ns_select(int N, int L, int B, double *__restrict__ live,
                                                      double *__restrict__ LL, double *__restrict__ LP,
                                                      double *__restrict__ LPW, const double *__restrict__ cand,
                                                      const double *__restrict__ cLL, const double *__restrict__ cLP,
                                                      const double *__restrict__ cLPW, int *rk0, int *rk1, int *cur,
                                                      double *__restrict__ lstar, double *__restrict__ out) {
  __shared__ int cnt[NS_TPB];
  const int tid = threadIdx.x;
  int *ra = *cur ? rk1 : rk0, *rb = *cur ? rk0 : rk1;
  double lStar = lstar[0], lStarOld = lstar[1];
  int accepted = 0;
  double *pairs = out + 4, *rows = out + 4 + 2 * (size_t)B;
  __syncthreads();
  for (int c = 0; c < B; c++) {
    const double ll = cLL[c];
    if (ll < lStar) continue;  // :305 (uniform)
    const int s = ra[0];
    double *row = rows + (size_t)accepted * (N + 4);
    const double oldKey = LPW[s] + LL[s];
    for (int d = tid; d < N; d += NS_TPB) row[d] = live[(size_t)s * N + d];
    if (tid == 0) {
      row[N] = LP[s];
      row[N + 1] = LPW[s];
      row[N + 2] = LL[s];
      row[N + 3] = isfinite(oldKey) ? 1.0 : 0.0;  // :330
    }
    __syncthreads();
    for (int d = tid; d < N; d += NS_TPB) live[(size_t)s * N + d] = cand[(size_t)c * N + d];
    const double lpw = cLPW[c];
    if (tid == 0) {
      LP[s] = cLP[c];
      LPW[s] = lpw;
      LL[s] = ll;
    }
    // :342, the re-sort: ra[1..L) is sorted; s goes behind the p points before it
    const double key = lpw + ll;
    int p = 0;
    for (int i = 1 + tid; i < L; i += NS_TPB) {
      const int j = ra[i];
      const double kj = LPW[j] + LL[j];
      if (kj < key || (kj == key && j < s)) p++;
    }
    cnt[tid] = p;
    __syncthreads();
    for (int q = NS_TPB / 2; q > 0; q >>= 1) {
      if (tid < q) cnt[tid] += cnt[tid + q];
      __syncthreads();
    }
    p = cnt[0];
    for (int i = tid; i < L; i += NS_TPB) rb[i] = i < p ? ra[i + 1] : (i == p ? s : ra[i]);
    __syncthreads();
    int *t = ra;
    ra = rb;
    rb = t;
    const int w = ra[0];
    const double wk = (w == s) ? key : LPW[w] + LL[w];
    if (isfinite(wk)) {  // :348-352
      lStarOld = lStar;
      lStar = wk;
    }
    if (tid == 0) {
      pairs[2 * accepted] = lStar;
      pairs[2 * accepted + 1] = lStarOld;
    }
    accepted++;
    __syncthreads();
  }
  if (tid == 0) {
    const int hi = ra[L - 1];
    out[0] = (double)accepted;
    out[1] = LPW[hi] + LL[hi];  // :356-357
    out[2] = lStar;
    out[3] = lStarOld;
    lstar[0] = lStar;
    lstar[1] = lStarOld;
    *cur = (ra == rk1) ? 1 : 0;
  }
}

__global__ void k_ns_rank_to_double(int L, const int *__restrict__ rank, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) out[i] = (double)rank[i];
}

__global__ void k_ns_rank_from_double(int L, const double *__restrict__ in, int *__restrict__ rank) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  int r = (int)in[i];
  rank[i] = r < 0 ? 0 : (r >= L ? L - 1 : r);  // (a restored rank cannot index outside the live set)
}

}  // namespace kg

using namespace kg;

struct kg_nested_s {
  kg_nested_cfg cfg;
  int N = 0, L = 0, B = 0;
  bool ellipse = false;
  hipStream_t stream = nullptr;
  double *live = nullptr, *liveLL = nullptr, *liveLP = nullptr, *liveLPW = nullptr;
  double *cand = nullptr, *candLL = nullptr, *candLP = nullptr, *candLPW = nullptr;
  int *rank[2] = {nullptr, nullptr}, *cur = nullptr;
  double *boxLo = nullptr, *boxUp = nullptr, *mean = nullptr, *cov = nullptr, *invCov = nullptr, *axes = nullptr;
  NsEllipse *el = nullptr;
  double *lower = nullptr, *width = nullptr, *logWidth = nullptr, *pmin = nullptr, *pmax = nullptr, *cst = nullptr;
  int *kind = nullptr;
  double *theta = nullptr, *z = nullptr, *tryX = nullptr, *ubuf = nullptr, *out = nullptr, *lstar = nullptr;
  double *tmp = nullptr;  // L doubles: the rank as doubles
  int *flag = nullptr;
  unsigned long long *blockEnd = nullptr, *sel = nullptr;
  NsChain *chain = nullptr;
  size_t window = 0, windowMax = 0, maxWindows = 0, windowsLast = 0, triesLast = 0;
  MtStream uniform, normal;
  double K = 0.0;  // :863
  std::vector<double> hLower, hWidth, hout;
  // the host's part of the state (Nested.config Internal Settings)
  double acceptedSamples = 0, generatedSamples = 0, logEvidence = NS_LOWEST, logEvidenceVar = 0, logVolume = 0,
         boundLogVolume = 0, lastAccepted = 0, nextUpdate = 0, information = 0, lStar = NS_LOWEST,
         lStarOld = NS_LOWEST, logWeight = 0, expectedLogShrinkage = 0, maxEvaluation = 0, remainingLogEvidence = 0,
         logEvidenceDifference = NS_MAX, effectiveSampleSize = 0, sumLogWeights = NS_LOWEST,
         sumSquareLogWeights = NS_LOWEST, modelEvaluationCount = 0, numberDeadSamples = 0;
  std::vector<double> deadSamples, deadLL, deadLP, deadLPW, deadLW;
  std::vector<double> postSamples, postLP, postLL;
  int stage = 0;         // 0: nothing pending; 1: prepared; 2: evaluated
  size_t pendingRows = 0;
  bool pendingLive = false;  // the pending rows are the live set (generation 1)
  bool started = false;  // the first generation ran (or a state was restored)
  bool acceptedLast = true;
  StageTimes times;
};

namespace {

// auxiliar/math.hpp:165-196
double ns_safe_log_plus(double x, double y) {
  if (x > y) return x + log1p(std::exp(y - x));
  return y + log1p(std::exp(x - y));
}

int ns_safe_log_minus(double x, double y, double *r) {
  if (x - y > 12.0) {
    *r = x;
    return 0;
  }
  if (x > y) {
    *r = y + std::log(std::exp(x - y) - 1.);
    return 0;
  }
  char buf[200];
  snprintf(buf, sizeof buf, "Invalid input to mathematical function 'safeLogMinus, x (%.*e) must be larger than y (%.*e)\n",
           6, x, 6, y);
  set_error(buf);
  return 1;
}

// Gamma(n / 2), n >= 1: the closed product, factors ascending
double ns_gamma_half(size_t n) {
  double g;
  if (n % 2 == 0) {
    g = 1.0;  // Gamma(m) = (m - 1)!
    for (size_t k = 1; k < n / 2; k++) g *= (double)k;
  } else {
    g = std::sqrt(M_PI);  // Gamma(m + 1/2) = sqrt(pi) (1/2)(3/2)...(m - 1/2)
    for (size_t k = 0; k < n / 2; k++) g *= (double)k + 0.5;
  }
  return g;
}

enum NsWhere { NS_DEV, NS_RANK, NS_HOST, NS_VEC, NS_DEAD };
struct NsField {
  NsWhere where = NS_DEV;
  double *dev = nullptr;               // NS_DEV
  double *host = nullptr;              // NS_HOST (n values)
  std::vector<double> *vec = nullptr;  // NS_VEC / NS_DEAD
  size_t n = 0;
  size_t rowWidth = 1;
};

bool ns_field(kg_nested_s *h, const char *name, NsField &f) {
  const std::string k = name ? name : "";
  const size_t N = h->N, L = h->L, B = h->B;
  auto dev = [&](double *p, size_t n) {
    f.where = NS_DEV;
    f.dev = p;
    f.n = n;
    return true;
  };
  auto host = [&](double *p, size_t n = 1) {
    f.where = NS_HOST;
    f.host = p;
    f.n = n;
    return true;
  };
  auto vec = [&](std::vector<double> *v, NsWhere w, size_t width = 1) {
    f.where = w;
    f.vec = v;
    f.n = v->size();
    f.rowWidth = width;
    return true;
  };
  if (k == "Live Samples") return dev(h->live, L * N);
  if (k == "Live LogLikelihoods") return dev(h->liveLL, L);
  if (k == "Live LogPriors") return dev(h->liveLP, L);
  if (k == "Live LogPrior Weights") return dev(h->liveLPW, L);
  if (k == "Live Samples Rank") {
    f.where = NS_RANK;
    f.n = L;
    return true;
  }
  if (k == "Candidates") return dev(h->cand, B * N);
  if (k == "Candidate LogLikelihoods") return dev(h->candLL, B);
  if (k == "Candidate LogPriors") return dev(h->candLP, B);
  if (k == "Candidate LogPrior Weights") return dev(h->candLPW, B);
  if (!h->ellipse) {
    if (k == "Box Lower Bound") return dev(h->boxLo, N);
    if (k == "Box Upper Bound") return dev(h->boxUp, N);
  } else {
    if (k == "Ellipse Axes") return dev(h->axes, N * N);
    if (k == "Ellipse Mean") return dev(h->mean, N);
    if (k == "Covariance Matrix") return dev(h->cov, N * N);
    if (k == "Ellipse Inverse Covariance") return dev(h->invCov, N * N);
    if (k == "Ellipse Determinant") return dev(&h->el->det, 1);
    if (k == "Ellipse Volume") return dev(&h->el->volume, 1);
  }
  if (k == "Prior Lower Bound") return host(h->hLower.data(), N);
  if (k == "Prior Width") return host(h->hWidth.data(), N);
  if (k == "Accepted Samples") return host(&h->acceptedSamples);
  if (k == "Generated Samples") return host(&h->generatedSamples);
  if (k == "LogEvidence") return host(&h->logEvidence);
  if (k == "LogEvidence Var") return host(&h->logEvidenceVar);
  if (k == "LogVolume") return host(&h->logVolume);
  if (k == "Bound LogVolume") return host(&h->boundLogVolume);
  if (k == "Last Accepted") return host(&h->lastAccepted);
  if (k == "Next Update") return host(&h->nextUpdate);
  if (k == "Information") return host(&h->information);
  if (k == "LStar") return host(&h->lStar);
  if (k == "LStarOld") return host(&h->lStarOld);
  if (k == "LogWeight") return host(&h->logWeight);
  if (k == "Expected LogShrinkage") return host(&h->expectedLogShrinkage);
  if (k == "Max Evaluation") return host(&h->maxEvaluation);
  if (k == "Remaining Log Evidence") return host(&h->remainingLogEvidence);
  if (k == "Log Evidence Difference") return host(&h->logEvidenceDifference);
  if (k == "Effective Sample Size") return host(&h->effectiveSampleSize);
  if (k == "Sum Log Weights") return host(&h->sumLogWeights);
  if (k == "Sum Square Log Weights") return host(&h->sumSquareLogWeights);
  if (k == "Number Dead Samples") return host(&h->numberDeadSamples);
  if (k == "Model Evaluation Count") return host(&h->modelEvaluationCount);
  if (k == "Dead Samples") return vec(&h->deadSamples, NS_DEAD, N);
  if (k == "Dead LogLikelihoods") return vec(&h->deadLL, NS_DEAD);
  if (k == "Dead LogPriors") return vec(&h->deadLP, NS_DEAD);
  if (k == "Dead LogPrior Weights") return vec(&h->deadLPW, NS_DEAD);
  if (k == "Dead LogWeights") return vec(&h->deadLW, NS_DEAD);
  if (k == "Posterior Samples Database") return vec(&h->postSamples, NS_VEC, N);
  if (k == "Posterior Samples LogPrior Database") return vec(&h->postLP, NS_VEC);
  if (k == "Posterior Samples LogLikelihood Database") return vec(&h->postLL, NS_VEC);
  return false;
}

int ns_push_lstar(kg_nested_s *h) {
  const double v[2] = {h->lStar, h->lStarOld};
  KG_HIP(hipMemcpyAsync(h->lstar, v, sizeof v, hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

// updateDeadSamples (:518-530) with updateEffectiveSamples (:981-987)
void ns_dead(kg_nested_s *h, const double *x, double lp, double lpw, double ll) {
  h->numberDeadSamples += 1;
  for (int d = 0; d < h->N; d++) {
    const double xw = x[d] * h->hWidth[d];
    h->deadSamples.push_back(h->hLower[d] + xw);
  }
  h->deadLP.push_back(lp);
  h->deadLPW.push_back(lpw);
  h->deadLL.push_back(ll);
  h->deadLW.push_back(h->logWeight);
  const double w = h->logWeight;
  h->sumLogWeights = ns_safe_log_plus(h->sumLogWeights, w);
  h->sumSquareLogWeights = ns_safe_log_plus(h->sumSquareLogWeights, 2. * w);
  h->effectiveSampleSize = std::exp(2. * h->sumLogWeights - h->sumSquareLogWeights);
}

// setBoundsVolume (:378-392)
int ns_bounds_volume(kg_nested_s *h) {
  if (!h->ellipse) {
    std::vector<double> b(2 * (size_t)h->N);
    KG_HIP(hipMemcpyAsync(b.data(), h->boxLo, h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipMemcpyAsync(b.data() + h->N, h->boxUp, h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    h->boundLogVolume = NS_LOWEST;
    for (int d = 0; d < h->N; d++)
      h->boundLogVolume = ns_safe_log_plus(h->boundLogVolume, std::log(b[h->N + d] - b[d]));
  } else {
    NsEllipse e;
    KG_HIP(hipMemcpyAsync(&e, h->el, sizeof e, hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    h->boundLogVolume = std::log(e.volume);
  }
  return 0;
}

int ns_terminated(kg_nested_s *h, size_t generation) {
  int t = 0;
  if (generation > 1 && h->logEvidenceDifference <= h->cfg.min_log_evidence_delta) t |= KG_NESTED_MIN_LOG_EVIDENCE_DELTA;
  if (h->cfg.max_effective_sample_size <= h->effectiveSampleSize) t |= KG_NESTED_MAX_EFFECTIVE_SAMPLE_SIZE;
  if (h->cfg.max_log_likelihood <= h->lStar) t |= KG_NESTED_MAX_LOG_LIKELIHOOD;
  return t;
}

// updateBounds (:253-273)
int ns_update_bounds(kg_nested_s *h) {
  // (:255: the Box method holds no ellipse, so it updates on every call)
  if (h->ellipse && h->generatedSamples < h->nextUpdate) return 0;
  h->nextUpdate += (double)h->cfg.proposal_update_frequency;
  Stage st(h->times, h->stream, "bounds");
  const int N = h->N, L = h->L;
  if (!h->ellipse) {
    hipLaunchKernelGGL(k_ns_box, dim3((N + 63) / 64), dim3(64), 0, h->stream, N, L, (const double *)h->live, h->boxLo,
                       h->boxUp);
    KG_HIP(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(k_ns_mean, dim3((N + 63) / 64), dim3(64), 0, h->stream, N, L, (const double *)h->live, h->mean);
  KG_HIP(hipGetLastError());
  const int diag = L <= N ? 1 : 0;
  const double weight = 1. / ((double)L - 1.);
  hipLaunchKernelGGL(k_ns_cov, dim3((N * N + NS_TPB - 1) / NS_TPB), dim3(NS_TPB), 0, h->stream, N, L, diag, weight,
                     (const double *)h->live, (const double *)h->mean, h->cov, h->invCov);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_ns_factor, dim3(1), dim3(NS_TPB), (size_t)N * N * sizeof(double), h->stream, N, L, diag,
                     (const double *)h->live, (const double *)h->mean, h->cov, h->invCov, h->axes, h->logVolume,
                     h->cfg.ellipsoidal_scaling, h->K, h->el);
  KG_HIP(hipGetLastError());
  return 0;
}

// generateCandidates (:402-443)
int ns_draw(kg_nested_s *h) {
  Stage st(h->times, h->stream, "draw");
  const int N = h->N, B = h->B;
  KG_HIP(hipMemsetAsync(h->chain, 0, sizeof(NsChain), h->stream));
  h->windowsLast = 0;
  h->triesLast = 0;
  for (size_t w = 0;; w++) {
    NsChain ch{};
    if (w >= h->maxWindows) {
      set_error("Nested: no " + std::to_string(B) + " candidates inside the unit cube after " + std::to_string(w) +
                " windows (" + std::to_string(h->triesLast) + " tries): the reference would redraw forever");
      return 1;
    }
    const unsigned long long W = h->window;
    const unsigned grid = (unsigned)((W + NS_TPB - 1) / NS_TPB);
    if (h->ellipse) {
      if (h->normal.polar_normals(h->z, W * N, N, h->blockEnd, h->stream)) return 1;
      if (h->uniform.peek_uniforms(h->ubuf, W, h->stream)) return 1;
      hipLaunchKernelGGL(k_ns_try_ellipse, dim3(grid), dim3(NS_TPB), 0, h->stream, N, W, h->z,
                         (const double *)h->ubuf, (const double *)h->mean, (const double *)h->axes, h->tryX, h->flag);
    } else {
      if (h->uniform.peek_uniforms(h->ubuf, W * N, h->stream)) return 1;
      hipLaunchKernelGGL(k_ns_try_box, dim3(grid), dim3(NS_TPB), 0, h->stream, N, W, (const double *)h->ubuf,
                         (const double *)h->boxLo, (const double *)h->boxUp, h->tryX, h->flag);
    }
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ns_scan, dim3(1), dim3(NS_TPB), 0, h->stream, N, B, W, (const int *)h->flag, h->sel,
                       h->chain);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ns_gather, dim3((unsigned)std::min<size_t>(64, ((size_t)B * N + NS_TPB - 1) / NS_TPB)),
                       dim3(NS_TPB), 0, h->stream, N, (const double *)h->tryX, (const unsigned long long *)h->sel,
                       (const NsChain *)h->chain, h->cand);
    KG_HIP(hipGetLastError());
    if (h->ellipse) {
      if (h->normal.consume_normals_dev(&h->chain->used, N, h->blockEnd, h->stream)) return 1;
      if (h->uniform.consume_words_dev(&h->chain->used, h->stream)) return 1;
    } else {
      if (h->uniform.consume_words_dev(&h->chain->usedWords, h->stream)) return 1;
    }
    h->windowsLast++;
    KG_HIP(hipMemcpyAsync(&ch, h->chain, sizeof(ch), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    h->triesLast += ch.used;
    if (ch.done) break;
    // a window that did not finish the batch: the next, and those of later draws, hold twice as many
    if (2 * h->window <= h->windowMax) h->window *= 2;
  }
  return 0;
}

int ns_evaluate_rows(kg_nested_s *h, const double *X, size_t n, double *LL, double *LP, double *LPW) {
  Stage st(h->times, h->stream, "evaluate");
  hipLaunchKernelGGL(k_ns_evaluate, dim3((unsigned)((n + NS_TPB - 1) / NS_TPB)), dim3(NS_TPB), 0, h->stream, h->N,
                     (int)n, h->cfg.likelihood, X, (const double *)h->lower, (const double *)h->width,
                     (const double *)h->logWidth, (const double *)h->pmin, (const double *)h->pmax,
                     (const double *)h->cst, (const int *)h->kind, h->theta, LL, LP, LPW);
  KG_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int kg_nested_create(const kg_nested_cfg *cfg, kg_nested_t *out) {
  KG_CHECK(cfg && out, "kg_nested_create: null argument");
  // Nested.cpp.base:64-68
  if (cfg->min_log_evidence_delta < 0.) {
    char buf[160];
    snprintf(buf, sizeof buf, "Min Log Evidence Delta must be larger equal 0.0 (is %lf).\n", cfg->min_log_evidence_delta);
    set_error(buf);
    return 1;
  }
  KG_CHECK(cfg->resampling_method != KG_NESTED_MULTI_ELLIPSE,
           "Resampling Method 'Multi Ellipse' is not available on the device (use 'Box' or 'Ellipse').");
  KG_CHECK(cfg->resampling_method == KG_NESTED_BOX || cfg->resampling_method == KG_NESTED_ELLIPSE,
           "Only accepted Resampling Method are 'Box', 'Ellipse' and 'Multi Ellipse'");
  KG_CHECK(cfg->proposal_update_frequency > 0, "Proposal Update Frequency must be larger 0");
  KG_CHECK(cfg->variable_count >= 1, "Nested: 'Variable Count' must be >= 1");
  KG_CHECK(cfg->variable_count <= (size_t)NS_MAXN, "Nested: more than 64 variables are not supported on the device");
  // :93
  KG_CHECK(cfg->resampling_method != KG_NESTED_ELLIPSE || cfg->variable_count >= 3,
           "Resampling Method 'Ellipse' and 'Multi Ellipse' only suitable for problems of dim larger 2 (use "
           "Resampling Method 'Box').");
  KG_CHECK(cfg->number_live_points >= 2, "Nested: 'Number Live Points' must be at least 2");
  KG_CHECK(cfg->number_live_points < (1u << 24), "Nested: 'Number Live Points' too large");
  KG_CHECK(cfg->batch_size >= 1, "Nested: 'Batch Size' must be at least 1");
  KG_CHECK(cfg->batch_size < (1u << 24), "Nested: 'Batch Size' too large");
  KG_CHECK(cfg->prior_min && cfg->prior_max, "Nested needs the parameters of every variable's prior");
  KG_CHECK(cfg->likelihood == KG_LIK_GAUSSIAN || cfg->likelihood == -1, "unknown builtin likelihood");
  const size_t N = cfg->variable_count, L = cfg->number_live_points, B = cfg->batch_size;
  std::vector<int> kind(N, KG_PRIOR_UNIFORM);
  std::vector<double> lower(N), width(N);
  for (size_t d = 0; d < N; d++) {
    if (cfg->prior_kind) kind[d] = cfg->prior_kind[d];
    KG_CHECK(kind[d] >= KG_PRIOR_UNIFORM && kind[d] <= KG_PRIOR_LOGNORMAL,
             "prior_kind entries must be KG_PRIOR_UNIFORM .. KG_PRIOR_LOGNORMAL");
    if (kind[d] == KG_PRIOR_UNIFORM) {  // :81-85
      width[d] = cfg->prior_max[d] - cfg->prior_min[d];
      lower[d] = cfg->prior_min[d];
    } else {  // :77-79, :86-90
      KG_CHECK(cfg->lower_bound && std::isfinite(cfg->lower_bound[d]),
               "Prior of variable " + std::to_string(d) + " is not 'Univariate/Uniform' AND lower bound not set (invalid configuration).");
      KG_CHECK(cfg->upper_bound && std::isfinite(cfg->upper_bound[d]),
               "Prior of variable " + std::to_string(d) + " is not 'Univariate/Uniform' AND upper bound not set (invalid configuration).");
      width[d] = cfg->upper_bound[d] - cfg->lower_bound[d];
      lower[d] = cfg->lower_bound[d];
    }
  }
  KG_HIP(hipSetDevice(cfg->device));
  upload_dd_tables();  // log_cr of the polar normals and the priors, exp_cr / pow_cr of the ellipse
  auto *h = new kg_nested_s();
  h->cfg = *cfg;
  h->cfg.prior_min = h->cfg.prior_max = h->cfg.lower_bound = h->cfg.upper_bound = nullptr;
  h->cfg.prior_kind = nullptr;
  h->N = (int)N;
  h->L = (int)L;
  h->B = (int)B;
  h->ellipse = cfg->resampling_method == KG_NESTED_ELLIPSE;
  h->hLower = lower;
  h->hWidth = width;
  h->expectedLogShrinkage = std::log(((double)L + 1.) / (double)L);  // :121
  // :863, once: sqrt(pi^N) 2 / (N Gamma(N / 2))
  h->K = std::sqrt(std::pow(M_PI, (double)N)) * 2. / ((double)N * ns_gamma_half(N));
  // a window holds a few batches of tries; one that does not finish the batch doubles it up to windowMax
  const size_t w0 = cfg->window_tries ? cfg->window_tries : std::max<size_t>(2 * B, 256);
  h->window = w0;
  h->windowMax = std::max<size_t>(w0, std::min<size_t>(65536, ((size_t)1 << 20) / N));
  h->maxWindows = cfg->max_windows ? cfg->max_windows : 4096;
  const size_t W = h->windowMax, rows = std::max(L, B);
  const size_t ucap = std::max(L * N, h->ellipse ? W : W * N);
  const size_t outN = 4 + 2 * B + B * (N + 4);
  h->hout.resize(outN);
  auto fail = [&]() {
    kg_nested_destroy(h);
    return 1;
  };
  if (stream_acquire(&h->stream) != hipSuccess) {
    set_error("kg_nested_create: no stream");
    return fail();
  }
  if (dalloc(&h->live, L * N) || dalloc(&h->liveLL, L) || dalloc(&h->liveLP, L) || dalloc(&h->liveLPW, L) ||
      dalloc(&h->cand, B * N) || dalloc(&h->candLL, B) || dalloc(&h->candLP, B) || dalloc(&h->candLPW, B) ||
      dalloc(&h->rank[0], L) || dalloc(&h->rank[1], L) || dalloc(&h->cur, 1) || dalloc(&h->boxLo, N) ||
      dalloc(&h->boxUp, N) || dalloc(&h->mean, N) || dalloc(&h->cov, N * N) || dalloc(&h->invCov, N * N) ||
      dalloc(&h->axes, N * N) || dalloc(&h->el, 1) || dalloc(&h->lower, N) || dalloc(&h->width, N) ||
      dalloc(&h->logWidth, N) || dalloc(&h->pmin, N) || dalloc(&h->pmax, N) || dalloc(&h->cst, N) ||
      dalloc(&h->kind, N) || dalloc(&h->theta, rows * N) || dalloc(&h->tryX, W * N) || dalloc(&h->ubuf, ucap) ||
      dalloc(&h->out, outN) || dalloc(&h->lstar, 2) || dalloc(&h->tmp, L) || dalloc(&h->flag, W) ||
      dalloc(&h->sel, B) || dalloc(&h->chain, 1))
    return fail();
  if (h->ellipse && (dalloc(&h->z, W * N) || dalloc(&h->blockEnd, W))) return fail();
  if (hipMemcpy(h->lower, lower.data(), N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->width, width.data(), N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->pmin, cfg->prior_min, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->pmax, cfg->prior_max, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->kind, kind.data(), N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_nested_create: upload failed");
    return fail();
  }
  if (h->ellipse &&
      allow_dynamic_lds((const void *)k_ns_factor, N * N * sizeof(double)) != hipSuccess) {
    set_error("kg_nested_create: kernel LDS");
    return fail();
  }
  hipLaunchKernelGGL(k_ns_prior_const, dim3(1), dim3(NS_MAXN), 0, h->stream, h->N, (const double *)h->pmin,
                     (const double *)h->pmax, (const int *)h->kind, (const double *)h->width, h->cst, h->logWidth);
  if (hipGetLastError() != hipSuccess || ns_push_lstar(h)) {
    set_error("kg_nested_create: prior constants");
    return fail();
  }
  if (h->ellipse && h->normal.init(4 * h->normal.words_for_normals(W * N) + 16384)) return fail();
  if (h->uniform.init(4 * ucap + 16384)) return fail();
  unsigned char st[5000];
  gsl_seed_state(cfg->uniform_seed, st);
  if (h->uniform.import_gsl(st, h->stream)) return fail();
  if (h->ellipse) {
    gsl_seed_state(cfg->normal_seed, st);
    if (h->normal.import_gsl(st, h->stream)) return fail();
  }
  *out = h;
  return 0;
}

int kg_nested_destroy(kg_nested_t h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->normal.drain();
  h->uniform.drain();
  for (void *p : {(void *)h->live,    (void *)h->liveLL,  (void *)h->liveLP,   (void *)h->liveLPW, (void *)h->cand,
                  (void *)h->candLL,  (void *)h->candLP,  (void *)h->candLPW,  (void *)h->rank[0], (void *)h->rank[1],
                  (void *)h->cur,     (void *)h->boxLo,   (void *)h->boxUp,    (void *)h->mean,    (void *)h->cov,
                  (void *)h->invCov,  (void *)h->axes,    (void *)h->el,       (void *)h->lower,   (void *)h->width,
                  (void *)h->logWidth, (void *)h->pmin,   (void *)h->pmax,     (void *)h->cst,     (void *)h->kind,
                  (void *)h->theta,   (void *)h->z,       (void *)h->tryX,     (void *)h->ubuf,    (void *)h->out,
                  (void *)h->lstar,   (void *)h->tmp,     (void *)h->flag,     (void *)h->blockEnd, (void *)h->sel,
                  (void *)h->chain})
    if (p) dev_release(p);
  h->times.release();
  if (h->stream) stream_release(h->stream);
  delete h;
  return 0;
}

int kg_nested_prepare(kg_nested_t h, size_t generation) {
  KG_CHECK(h, "kg_nested_prepare: null handle");
  KG_CHECK(generation >= 1, "kg_nested_prepare: generations count from 1");
  const size_t N = h->N, L = h->L, B = h->B;
  if (generation == 1) {
    // runFirstGeneration's draws (:208-210) and the priors of the live set
    {
      Stage st(h->times, h->stream, "draw");
      if (h->uniform.uniforms(h->live, L * N, h->stream)) return 1;
    }
    if (ns_evaluate_rows(h, h->live, L, h->liveLL, h->liveLP, h->liveLPW)) return 1;
    h->pendingRows = L;
    h->pendingLive = true;
    h->stage = h->cfg.likelihood < 0 ? 1 : 2;
    return 0;
  }
  h->pendingLive = false;
  KG_CHECK(h->started, "kg_nested_prepare: the handle holds no live set (the first generation, or a restored state, first)");
  if (h->acceptedLast) h->lastAccepted = 0;  // :161
  h->acceptedLast = false;
  if (ns_update_bounds(h)) return 1;
  if (ns_draw(h)) return 1;
  if (ns_evaluate_rows(h, h->cand, B, h->candLL, h->candLP, h->candLPW)) return 1;
  h->pendingRows = B;
  h->stage = h->cfg.likelihood < 0 ? 1 : 2;
  return 0;
}

int kg_nested_get_candidates(kg_nested_t h, double *X, size_t ld) {
  KG_CHECK(h, "kg_nested_get_candidates: null handle");
  KG_CHECK(X, "kg_nested_get_candidates: null output");
  KG_CHECK(ld == 0 || ld >= (size_t)h->N, "kg_nested_get_candidates: ld is smaller than the variable count");
  KG_CHECK(h->stage >= 1, "kg_nested_get_candidates: nothing prepared");
  const size_t N = h->N;
  if (ld == 0) ld = N;
  KG_HIP(hipMemcpy2DAsync(X, ld * sizeof(double), h->theta, N * sizeof(double), N * sizeof(double), h->pendingRows,
                          hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_nested_set_evaluations(kg_nested_t h, const double *loglik) {
  KG_CHECK(h, "kg_nested_set_evaluations: null handle");
  KG_CHECK(loglik, "kg_nested_set_evaluations: null log-likelihoods");
  KG_CHECK(h->stage >= 1, "kg_nested_set_evaluations: nothing prepared");
  const size_t n = h->pendingRows;
  for (size_t i = 0; i < n; i++)  // bayesian.cpp.base:73
    KG_CHECK(!std::isnan(loglik[i]), "Sample " + std::to_string(i) + " returned NaN logLikelihood evaluation.\n");
  Stage st(h->times, h->stream, "evaluate");
  double *LL = h->pendingLive ? h->liveLL : h->candLL;
  const double *LP = LL == h->liveLL ? h->liveLP : h->candLP;
  KG_HIP(hipMemcpyAsync(LL, loglik, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_ns_mask_ll, dim3((unsigned)((n + NS_TPB - 1) / NS_TPB)), dim3(NS_TPB), 0, h->stream, (int)n, LP,
                     LL);
  KG_HIP(hipGetLastError());
  KG_HIP(hipStreamSynchronize(h->stream));  // loglik is the caller's
  h->stage = 2;
  return 0;
}

int kg_nested_eval_builtin(kg_nested_t h) {
  KG_CHECK(h, "kg_nested_eval_builtin: null handle");
  KG_CHECK(h->cfg.likelihood == KG_LIK_GAUSSIAN, "kg_nested_eval_builtin: the handle has no builtin likelihood");
  KG_CHECK(h->stage >= 1, "kg_nested_eval_builtin: nothing prepared");
  return 0;  // k_ns_evaluate wrote it with the priors
}

int kg_nested_process(kg_nested_t h, size_t generation, int *accepted, int *terminated_by) {
  KG_CHECK(h, "kg_nested_process: null handle");
  KG_CHECK(h->stage == 2, "kg_nested_process: the candidates have no log-likelihoods yet");
  const int N = h->N, L = h->L, B = h->B;
  h->stage = 0;
  if (h->pendingLive) {
    h->pendingLive = false;
    h->modelEvaluationCount += L;
    h->generatedSamples += L;
    Stage st(h->times, h->stream, "select");
    KG_HIP(hipMemsetAsync(h->cur, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_ns_sort, dim3((L + NS_TPB - 1) / NS_TPB), dim3(NS_TPB), 0, h->stream, L,
                       (const double *)h->liveLPW, (const double *)h->liveLL, h->rank[0]);
    KG_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_ns_first_stats, dim3(1), dim3(1), 0, h->stream, L, (const double *)h->liveLPW,
                       (const double *)h->liveLL, (const int *)h->rank[0], h->lstar, h->out);
    KG_HIP(hipGetLastError());
    KG_HIP(hipMemcpyAsync(h->hout.data(), h->out, 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    h->maxEvaluation = h->hout[1];
    h->lStar = h->hout[2];
    h->started = true;
    h->acceptedLast = true;
    if (accepted) *accepted = 1;
    if (terminated_by) *terminated_by = ns_terminated(h, generation);
    return 0;
  }
  KG_CHECK(h->started, "kg_nested_process: the handle holds no live set");
  h->modelEvaluationCount += B;  // :181-182
  h->generatedSamples += B;
  h->lastAccepted += 1;  // :199
  {
    Stage st(h->times, h->stream, "select");
    hipLaunchKernelGGL(k_ns_select, dim3(1), dim3(NS_TPB), 0, h->stream, N, L, B, h->live, h->liveLL, h->liveLP,
                       h->liveLPW, (const double *)h->cand, (const double *)h->candLL, (const double *)h->candLP,
                       (const double *)h->candLPW, h->rank[0], h->rank[1], h->cur, h->lstar, h->out);
    KG_HIP(hipGetLastError());
    KG_HIP(hipMemcpyAsync(h->hout.data(), h->out, h->hout.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
  }
  const int nacc = (int)h->hout[0];
  const double *pairs = h->hout.data() + 4, *rows = h->hout.data() + 4 + 2 * (size_t)B;
  for (int a = 0; a < nacc; a++) {
    // :308-327, with lStar / lStarOld as they stood before this candidate
    h->acceptedSamples += 1;
    const double logVolumeOld = h->logVolume, informationOld = h->information, logEvidenceOld = h->logEvidence;
    h->logVolume -= h->expectedLogShrinkage;
    const double dLogVol = std::log(0.5 * std::exp(logVolumeOld) - 0.5 * std::exp(h->logVolume));
    h->logWeight = ns_safe_log_plus(h->lStar, h->lStarOld) + dLogVol;
    h->logEvidence = ns_safe_log_plus(h->logEvidence, h->logWeight);
    const double evidenceTerm = std::exp(h->lStarOld - h->logEvidence) * h->lStarOld +
                                std::exp(h->lStar - h->logEvidence) * h->lStar;
    if (std::isfinite(evidenceTerm)) {
      h->information = std::exp(dLogVol) * evidenceTerm +
                       std::exp(logEvidenceOld - h->logEvidence) * (informationOld + logEvidenceOld) - h->logEvidence;
      h->logEvidenceVar += 2. * (h->information - informationOld) * h->expectedLogShrinkage;
    }
    const double *row = rows + (size_t)a * (N + 4);
    if (row[N + 3] != 0.0) ns_dead(h, row, row[N], row[N + 1], row[N + 2]);  // :330-333
    h->lStar = pairs[2 * a];
    h->lStarOld = pairs[2 * a + 1];
  }
  // :355-363
  h->maxEvaluation = h->hout[1];
  h->remainingLogEvidence = h->maxEvaluation + h->logVolume;
  h->logEvidenceDifference = ns_safe_log_plus(h->logEvidence, h->remainingLogEvidence) - h->logEvidence;
  if (ns_bounds_volume(h)) return 1;
  h->lastAccepted += 1;
  h->acceptedLast = nacc > 0;
  if (accepted) *accepted = nacc > 0 ? 1 : 0;
  if (terminated_by) *terminated_by = ns_terminated(h, generation);
  return 0;
}

int kg_nested_first_generation(kg_nested_t h) {
  KG_CHECK(h, "kg_nested_first_generation: null handle");
  KG_CHECK(h->cfg.likelihood == KG_LIK_GAUSSIAN, "kg_nested_first_generation: the handle has no builtin likelihood");
  if (kg_nested_prepare(h, 1)) return 1;
  return kg_nested_process(h, 1, nullptr, nullptr);
}

int kg_nested_generation(kg_nested_t h, size_t generation, int *terminated_by) {
  KG_CHECK(h, "kg_nested_generation: null handle");
  KG_CHECK(h->cfg.likelihood == KG_LIK_GAUSSIAN, "kg_nested_generation: the handle has no builtin likelihood");
  if (generation == 1) {
    if (kg_nested_first_generation(h)) return 1;
    if (terminated_by) *terminated_by = ns_terminated(h, 1);
    return 0;
  }
  // :167-201
  for (int accepted = 0; !accepted;) {
    if (kg_nested_prepare(h, generation)) return 1;
    if (kg_nested_process(h, generation, &accepted, terminated_by)) return 1;
  }
  return 0;
}

int kg_nested_finalize(kg_nested_t h) {
  KG_CHECK(h, "kg_nested_finalize: null handle");
  KG_CHECK(h->started, "kg_nested_finalize: the handle holds no live set");
  const size_t N = h->N, L = h->L;
  if (h->cfg.add_live_points) {
    // consumeLiveSamples (:532-578)
    std::vector<double> live(L * N), ll(L), lp(L), lpw(L);
    int cur = 0;
    KG_HIP(hipMemcpyAsync(&cur, h->cur, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    std::vector<int> rank(L);
    KG_HIP(hipMemcpyAsync(rank.data(), h->rank[cur ? 1 : 0], L * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipMemcpyAsync(live.data(), h->live, L * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipMemcpyAsync(ll.data(), h->liveLL, L * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipMemcpyAsync(lp.data(), h->liveLP, L * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipMemcpyAsync(lpw.data(), h->liveLPW, L * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> logvols(L + 1, h->logVolume), logdvols(L), dlvs(L);
    for (size_t i = 0; i < L; ++i) {
      logvols[i + 1] += std::log(1. - ((double)i + 1.) / ((double)L + 1.));
      if (ns_safe_log_minus(logvols[i], logvols[i + 1], &logdvols[i])) return 1;
      dlvs[i] = logvols[i] - logvols[i + 1];
    }
    // (:547 runs one entry past logdvols; the entries that exist get the term)
    for (size_t i = 0; i < L; ++i) logdvols[i] += std::log(0.5);
    for (size_t i = 0; i < L; ++i) {
      const size_t s = (size_t)rank[i];
      const double logEvidenceOld = h->logEvidence, informationOld = h->information;
      const double key = lpw[s] + ll[s];
      if (std::isfinite(key)) {
        h->lStarOld = h->lStar;
        h->lStar = key;
        ns_dead(h, live.data() + s * N, lp[s], lpw[s], ll[s]);
      }
      const double dLogVol = logdvols[i];
      if (ns_safe_log_minus(h->logVolume, dLogVol, &h->logVolume)) return 1;
      h->logWeight = ns_safe_log_plus(h->lStar, h->lStarOld) + dLogVol;
      h->logEvidence = ns_safe_log_plus(h->logEvidence, h->logWeight);
      const double evidenceTerm = std::exp(h->lStarOld - h->logEvidence) * h->lStarOld +
                                  std::exp(h->lStar - h->logEvidence) * h->lStar;
      h->information = std::exp(dLogVol) * evidenceTerm +
                       std::exp(logEvidenceOld - h->logEvidence) * (informationOld + logEvidenceOld) - h->logEvidence;
      h->logEvidenceVar += 2. * (h->information - informationOld) * dlvs[i];
    }
    if (ns_push_lstar(h)) return 1;
  }
  // generatePosterior (:580-612)
  const size_t nd = h->deadLW.size();
  KG_CHECK(nd > 0, "Nested: no dead samples to build the posterior from");
  const double maxLogWtDb = *std::max_element(h->deadLW.begin(), h->deadLW.end());
  std::vector<size_t> permutation(nd);
  if (kg_nested_permutation(h->cfg.shuffle_seed, nd, permutation.data())) return 1;
  double sum = 0.0;
  if (h->uniform.uniforms(h->ubuf, 1, h->stream)) return 1;
  KG_HIP(hipMemcpyAsync(&sum, h->ubuf, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->postSamples.clear();
  h->postLP.clear();
  h->postLL.clear();
  double k = 1.;
  for (size_t i = 0; i < nd; ++i) {
    const size_t r = permutation[i];
    sum += std::exp(h->deadLW[r] - maxLogWtDb);
    if (sum > k) {
      h->postSamples.insert(h->postSamples.end(), h->deadSamples.begin() + r * N, h->deadSamples.begin() + (r + 1) * N);
      h->postLP.push_back(h->deadLP[r]);
      h->postLL.push_back(h->deadLL[r]);
      k++;
    }
  }
  return 0;
}

int kg_nested_permutation(uint64_t seed, size_t n, size_t *out) {
  KG_CHECK(out || n == 0, "kg_nested_permutation: null output");
  std::vector<size_t> permutation(n);
  std::iota(std::begin(permutation), std::end(permutation), 0);
  std::shuffle(permutation.begin(), permutation.end(), std::default_random_engine(seed));
  for (size_t i = 0; i < n; i++) out[i] = permutation[i];
  return 0;
}

int kg_nested_synchronize(kg_nested_t h) {
  KG_CHECK(h, "kg_nested_synchronize: null handle");
  KG_HIP(hipStreamSynchronize(h->stream));
  StreamState s;
  for (MtStream *m : {&h->normal, &h->uniform}) {
    if (!m->state()) continue;
    KG_HIP(hipMemcpy(&s, m->state(), sizeof(s), hipMemcpyDeviceToHost));
    KG_CHECK(!(s.errors & KG_ERR_RNG_UNDERRUN), "Nested: a random stream was consumed past its generated words");
    KG_CHECK(s.errors == 0, "Nested: random stream error");
  }
  if (h->ellipse) {
    NsEllipse e;
    KG_HIP(hipMemcpy(&e, h->el, sizeof(e), hipMemcpyDeviceToHost));
    KG_CHECK(!(e.errors & KG_ERR_CHOLESKY),
             "Nested: the covariance of the live samples is not positive definite (non-positive Cholesky pivot)");
  }
  return 0;
}

int kg_nested_field_size(kg_nested_t h, const char *name, size_t *n) {
  KG_CHECK(h, "kg_nested_field_size: null handle");
  KG_CHECK(n, "kg_nested_field_size: null output");
  NsField f;
  KG_CHECK(ns_field(h, name, f), std::string("unknown Nested field: ") + (name ? name : "(null)"));
  *n = f.n;
  return 0;
}

int kg_nested_get_field(kg_nested_t h, const char *name, double *out, size_t n) {
  KG_CHECK(h, "kg_nested_get_field: null handle");
  KG_CHECK(out || n == 0, "kg_nested_get_field: null output");
  NsField f;
  KG_CHECK(ns_field(h, name, f), std::string("unknown Nested field: ") + (name ? name : "(null)"));
  KG_CHECK(n == f.n, std::string("Nested field size mismatch: ") + name);
  if (n == 0) return 0;
  switch (f.where) {
    case NS_HOST: memcpy(out, f.host, n * sizeof(double)); return 0;
    case NS_VEC:
    case NS_DEAD: memcpy(out, f.vec->data(), n * sizeof(double)); return 0;
    case NS_RANK: {
      int cur = 0;
      KG_HIP(hipMemcpyAsync(&cur, h->cur, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      KG_HIP(hipStreamSynchronize(h->stream));
      hipLaunchKernelGGL(k_ns_rank_to_double, dim3((unsigned)((n + NS_TPB - 1) / NS_TPB)), dim3(NS_TPB), 0, h->stream,
                         (int)n, (const int *)h->rank[cur ? 1 : 0], h->tmp);
      KG_HIP(hipGetLastError());
      f.dev = h->tmp;
      break;
    }
    default: break;
  }
  KG_HIP(hipMemcpyAsync(out, f.dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_nested_set_field(kg_nested_t h, const char *name, const double *in, size_t n) {
  KG_CHECK(h, "kg_nested_set_field: null handle");
  KG_CHECK(in || n == 0, "kg_nested_set_field: null input");
  NsField f;
  KG_CHECK(ns_field(h, name, f), std::string("unknown Nested field: ") + (name ? name : "(null)"));
  const std::string k = name;
  if (f.where == NS_DEAD || f.where == NS_VEC) {
    if (k == "Dead Samples") {
      KG_CHECK(n % (size_t)h->N == 0, "Nested field size mismatch: Dead Samples");
      h->numberDeadSamples = (double)(n / (size_t)h->N);
    } else if (f.where == NS_DEAD) {
      KG_CHECK(n == (size_t)h->numberDeadSamples, std::string("Nested field size mismatch: ") + name);
    } else {
      KG_CHECK(n % f.rowWidth == 0, std::string("Nested field size mismatch: ") + name);
    }
    f.vec->assign(in, in + n);
    return 0;
  }
  KG_CHECK(n == f.n, std::string("Nested field size mismatch: ") + name);
  if (f.where == NS_HOST) {
    KG_CHECK(k != "Prior Lower Bound" && k != "Prior Width", "Nested: the prior transform is fixed at create");
    memcpy(f.host, in, n * sizeof(double));
    if (k == "LStar" || k == "LStarOld") return ns_push_lstar(h);
    return 0;
  }
  if (f.where == NS_RANK) {
    KG_HIP(hipMemcpyAsync(h->tmp, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    KG_HIP(hipMemsetAsync(h->cur, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_ns_rank_from_double, dim3((unsigned)((n + NS_TPB - 1) / NS_TPB)), dim3(NS_TPB), 0, h->stream,
                       (int)n, (const double *)h->tmp, h->rank[0]);
    KG_HIP(hipGetLastError());
  } else {
    KG_HIP(hipMemcpyAsync(f.dev, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  KG_HIP(hipStreamSynchronize(h->stream));
  h->started = true;  // a restored state replaces the first generation
  return 0;
}

int kg_nested_get_rng(kg_nested_t h, int which, void *state5000) {
  KG_CHECK(h, "kg_nested_get_rng: null handle");
  KG_CHECK(state5000, "kg_nested_get_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  if (which == 0 && !h->ellipse) {
    // the Box method never draws from the Normal Generator: its seeded state
    gsl_seed_state(h->cfg.normal_seed, (unsigned char *)state5000);
    return 0;
  }
  return (which == 0 ? h->normal : h->uniform).export_gsl(state5000, h->stream);
}

int kg_nested_set_rng(kg_nested_t h, int which, const void *state5000) {
  KG_CHECK(h, "kg_nested_set_rng: null handle");
  KG_CHECK(state5000, "kg_nested_set_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  KG_CHECK(which == 1 || h->ellipse, "Nested: the Box method holds no Normal Generator stream");
  return (which == 0 ? h->normal : h->uniform).import_gsl(state5000, h->stream);
}

int kg_nested_diagnostics(kg_nested_t h, size_t *last_windows, size_t *last_tries, size_t *window_tries) {
  KG_CHECK(h, "kg_nested_diagnostics: null handle");
  if (last_windows) *last_windows = h->windowsLast;
  if (last_tries) *last_tries = h->triesLast;
  if (window_tries) *window_tries = h->window;
  return 0;
}

int kg_nested_profile(kg_nested_t h, int enable) {
  KG_CHECK(h, "kg_nested_profile: null handle");
  h->times.on = enable != 0;
  return 0;
}

int kg_nested_profile_read(kg_nested_t h, const char *stage, double *ms_total, size_t *count) {
  KG_CHECK(h, "kg_nested_profile_read: null handle");
  KG_CHECK(ms_total && count, "kg_nested_profile_read: null output");
  return h->times.read(h->stream, stage, ms_total, count);
}

}  // extern "C"
