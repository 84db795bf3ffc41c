// kg_mocmaes.hip — multi-objective CMA-ES on the MI355X (MOCMAES.cpp.base, see
// include/korali_amd.h for the per-entry-point reference map).
//
// HBM layout per handle (all FP64, sample-major as the reference's vectors):
//   X, V, Sg, Cm, Pa, Sr  [2]   the Current* and Previous* arrays (P x N, P x K,
//                               P, P x N*N, P x N, P); prepareGeneration's copy
//                               Previous* = Current* (:176-181) is a swap of the
//                               two buffer sets
//   pX, pSg, pC, pPa, pSr       the Parent* arrays (mu rows)
//   parentIdx                   "Parent Index" (P, stored as doubles)
//   LT                          mu factors sigma_p * chol(C_p), stored transposed
//   A, AV [2]                   "Sample Collection" / "Sample Value Collection"
//   two MtStreams               the Multinormal and the Uniform Generator
//
// What differs from the reference's loop structure, and why it is exact:
// * sampleSingle (:186-228) factors the parent's covariance for every sample;
//   the factor depends on the parent alone, so each parent drawn at least
//   once is factored once (k_mo_factor, one workgroup per parent).
// * The draw is a chain over the samples: sample i takes blocks of N normals
//   from one sequential stream until one is feasible, and sample i + 1
//   starts after sample i's last block.  k_mo_draw_spec first tries block i
//   for sample i, all samples in parallel (right up to the first rejection);
//   k_mo_draw_chain, one workgroup, takes over at that rejection and walks the
//   rest in order.  A launch sees a window of blocks; the host relaunches with
//   the next window until the chain is through (max_windows bounds it).
// * The copy from the parent (:220-227) is fused into the update: k_mo_update
//   reads the parent's row and writes the offspring's, so Current Covariance
//   Matrix, Sigma, Evolution Paths and Success Probabilities hold the
//   offspring's values after kg_mocmaes_update, not between prepare and update.
// * sortSampleIndices (:230-332): see k_mo_peel_* and k_mo_hv.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/korali_amd.h"
#include "kg_common.hpp"
#include "kg_gsl.hpp"
#include "kg_profile.hpp"
#include "kg_rng.hpp"

namespace kg {

constexpr int MO_TPB = 256;
constexpr int MO_MAXK = 8;
constexpr int MO_MAXN = 128;
constexpr int MO_1WG_MAX = 2048;   // merged values the one-workgroup sort holds in LDS
constexpr int MO_PEEL_BATCH = 16;  // peeling rounds queued per host read (multi-workgroup path)

struct MoScalars {
  double nonDominatedCount, infeasibleSampleCount, modelEvaluationCount, finishedSampleCount;
  double archiveCount;  // rows of the Sample Collection
  unsigned int errors;
  int failedParent;  // a parent whose covariance has a non-positive pivot
};

struct MoChain {
  unsigned long long used;  // blocks of this window consumed
  int sample;               // the sample the next block belongs to
  int done;
};

struct MoSort {
  int rounds;              // peeling rounds that ranked something
  double reference[MO_MAXK];
};

struct MoConst {
  int N, P, mu, K, n;  // n = 2P
  double cc, ccov, cp, target;
  double pathFactor, damp, chiN;
};

// ---------------------------------------------------------------- helpers
// exclusive prefix count of `flag` over the workgroup (MO_TPB threads), in
// thread order; *total receives the workgroup's count
__device__ inline int block_scan_flag(bool flag, int *total) {
  __shared__ int wsum[MO_TPB / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int pre = __popcll(b & ((1ULL << lane) - 1ULL));
  __syncthreads();  // wsum free
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
  for (int q = 0; q < MO_TPB / 64; q++) {
    if (q < w) off += wsum[q];
    tot += wsum[q];
  }
  *total = tot;
  return off + pre;
}

// value k of merged sample i: Current Values first, then Previous Values (:336-337)
__device__ inline double merged(const double *__restrict__ Vc, const double *__restrict__ Vp, int P, int K, int i,
                                int k) {
  return i < P ? Vc[(size_t)i * K + k] : Vp[(size_t)(i - P) * K + k];
}

// setInitialConfiguration's parents (:110-124): sigma = sqrt(trace / N), the
// covariance diag(sdev_d^2 / sigma^2), everything else 0
__global__ void k_mo_init_parents(int N, int mu, const double *__restrict__ sdev, double sigma, double target,
                                  double *__restrict__ pC, double *__restrict__ pSg, double *__restrict__ pSr) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t NN = (size_t)N * N;
  if (e >= (size_t)mu * NN) return;
  const size_t r = e % NN;
  const int d = (int)(r / N), c = (int)(r % N);
  pC[e] = d == c ? sdev[d] * sdev[d] / (sigma * sigma) : 0.0;
  if (r == 0) {
    pSg[e / NN] = sigma;
    pSr[e / NN] = target;
  }
}

// ------------------------------------------------------------- parent pick
// sampleSingle :188-195.  mu == P: parentIdx = i and the uniform stream is not
// touched (u == nullptr); else floor(min(mu, nd) * u_i).
__global__ void __launch_bounds__(MO_TPB) k_mo_pick(int P, int mu, const double *__restrict__ u, const MoScalars *sc,
                                                    double *__restrict__ parentIdx, int *__restrict__ used) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  int p = i;
  if (u) {
    const double nd = sc->nonDominatedCount;
    const double m = (double)mu < nd ? (double)mu : (nd > 0.0 ? nd : 0.0);  // std::min of two size_t
    const double f = floor(m * u[i]);
    p = (int)f;
  }
  if (p < 0) p = 0;  // (a restored state cannot index outside the parents)
  if (p >= mu) p = mu - 1;
  parentIdx[i] = (double)p;
  used[p] = 1;
}

// ------------------------------------------------------------------ factor
// sampleSingle :198-207: gsl_linalg_cholesky_decomp1 in place on a copy of the
// parent's covariance (block_cholesky_gsl), then gsl_matrix_scale by the
// parent's sigma.
// One workgroup per parent that was drawn; the matrix lives in LDS, N x (N+1).
// The lower triangle is written transposed (LT[j * N + r] = sigma * L[r][j]) so
// that the draw's threads, one per row r, read consecutive addresses.
// A non-positive pivot: the reference ignores decomp1's status (:203-206 test
// gsl_matrix_scale's) and draws from the partially factored matrix; here it
// is an error (KG_ERR_CHOLESKY, reported by kg_mocmaes_prepare).
__global__ void __launch_bounds__(MO_TPB) k_mo_factor(int N, const double *__restrict__ pC,
                                                      const double *__restrict__ pSg, const int *__restrict__ used,
                                                      double *__restrict__ LT, MoScalars *sc) {
  extern __shared__ double A[];  // N x (N+1)
  const int p = blockIdx.x;
  if (!used[p]) return;
  const int S = N + 1;
  const double *cov = pC + (size_t)p * N * N;
  for (int e = threadIdx.x; e < N * N; e += blockDim.x) A[(e / N) * S + e % N] = cov[e];
  __syncthreads();
  if (block_cholesky_gsl(A, N, S) && threadIdx.x == 0) {
    atomicOr(&sc->errors, KG_ERR_CHOLESKY);
    sc->failedParent = p;
  }
  const double sigma = pSg[p];
  double *out = LT + (size_t)p * N * N;
  for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
    const int j = e / N, r = e % N;  // out[j][r] = L[r][j]
    out[e] = r >= j ? A[r * S + j] * sigma : 0.0;
  }
}

// -------------------------------------------------------------------- draw
// One trial: x = mean_p + L_p z (gsl_ran_multivariate_gaussian,
// multivariate/normal/normal.cpp.base:30-35: dtrmv Lower/NoTrans/NonUnit in
// gslcblas order -- row r: temp = sum_{j<r} z_j L_rj from 0, then
// temp + z_r L_rr -- then gsl_vector_add of the mean), and
// Optimizer::isSampleFeasible (optimizer.cpp.base:5-14).  Thread r < N owns
// row r; zs is the block of N normals in LDS.  Returns this thread's verdict.
__device__ inline bool mo_trial(int N, int r, const double *zs, const double *__restrict__ LTp,
                                const double *__restrict__ mean, const double *__restrict__ lb,
                                const double *__restrict__ ub, double *x) {
  if (r >= N) return true;
  double temp = 0.0;
  for (int j = 0; j < r; j++) temp += zs[j] * LTp[(size_t)j * N + r];
  double v = temp + zs[r] * LTp[(size_t)r * N + r];
  v = v + mean[r];
  *x = v;
  return isfinite(v) && !(v < lb[r]) && !(v > ub[r]);
}

// sample i tries block i (window 0 only): exact for every sample before the
// first rejection, which k_mo_draw_chain finds in ok[]
__global__ void __launch_bounds__(MO_MAXN) k_mo_draw_spec(int N, int P, int mu, const double *__restrict__ z,
                                                          const double *__restrict__ LT,
                                                          const double *__restrict__ pX,
                                                          const double *__restrict__ parentIdx,
                                                          const double *__restrict__ lb, const double *__restrict__ ub,
                                                          double *__restrict__ X, int *__restrict__ ok) {
  __shared__ double zs[MO_MAXN];
  const int i = blockIdx.x, r = threadIdx.x;
  if (i >= P) return;
  int p = (int)parentIdx[i];
  p = p < 0 ? 0 : (p >= mu ? mu - 1 : p);
  if (r < N) zs[r] = z[(size_t)i * N + r];
  __syncthreads();
  double x = 0.0;
  const bool good = mo_trial(N, r, zs, LT + (size_t)p * N * N, pX + (size_t)p * N, lb, ub, &x);
  const int all = __syncthreads_and(good ? 1 : 0);
  if (r < N) X[(size_t)i * N + r] = x;
  if (r == 0) ok[i] = all;
}

// the chain (:209-217): one workgroup walks the samples in order from where
// the previous launch (or the speculative pass) stopped, one block per trial,
// until the samples or the window's W blocks run out
__global__ void __launch_bounds__(MO_TPB) k_mo_draw_chain(int N, int P, int mu, int spec, const double *__restrict__ z,
                                                          unsigned long long W, const double *__restrict__ LT,
                                                          const double *__restrict__ pX,
                                                          const double *__restrict__ parentIdx,
                                                          const double *__restrict__ lb, const double *__restrict__ ub,
                                                          double *__restrict__ X, const int *__restrict__ ok,
                                                          MoChain *ch) {
  __shared__ double zs[MO_MAXN];
  __shared__ int firstBad;
  const int tid = threadIdx.x;
  int i = ch->sample;
  unsigned long long b = 0;
  if (spec) {
    if (tid == 0) firstBad = P;
    __syncthreads();
    for (int s = tid; s < P; s += MO_TPB)
      if (!ok[s]) atomicMin(&firstBad, s);
    __syncthreads();
    i = firstBad;
    // samples 0..i-1 took blocks 0..i-1; sample i's block i was rejected
    b = i < P ? (unsigned long long)i + 1ULL : (unsigned long long)P;
  }
  while (i < P && b < W) {
    int p = (int)parentIdx[i];
    p = p < 0 ? 0 : (p >= mu ? mu - 1 : p);
    __syncthreads();  // zs free
    if (tid < N) zs[tid] = z[b * (unsigned long long)N + tid];
    __syncthreads();
    double x = 0.0;
    const bool good = mo_trial(N, tid, zs, LT + (size_t)p * N * N, pX + (size_t)p * N, lb, ub, &x);
    const int all = __syncthreads_and(good ? 1 : 0);
    b++;
    if (all) {
      if (tid < N) X[(size_t)i * N + tid] = x;
      i++;
    }
  }
  if (tid == 0) {
    ch->used = b;
    ch->sample = i;
    ch->done = i >= P ? 1 : 0;
  }
}

// -------------------------------------------------------------- objectives
// examples/optimization/multiobjective/_model/model.py term by term, x*x for
// **2, sums left to right; one thread per sample.  Non-finite values are an
// error (Optimization::evaluateMultiple, optimization.cpp.base:42-44).
__global__ void __launch_bounds__(MO_TPB) k_mo_objective(int N, int P, int K, const double *__restrict__ X,
                                                         double *__restrict__ V, MoScalars *sc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) sc->modelEvaluationCount += (double)P;  // MOCMAES.cpp.base:156
  if (i >= P) return;
  const double *x = X + (size_t)i * N;
  double one = 0.0, two = 0.0, three = 0.0;
  for (int d = 0; d + 1 < N; d++) {
    const double sq = x[d] * x[d];
    const double t = x[d + 1] - sq;
    const double t2 = t * t;
    const double h = 100.0 * t2;
    const double u = 1.0 - x[d];
    const double u2 = u * u;
    const double s = h + u2;
    one += s;
  }
  for (int d = 0; d < N; d++) {
    const double sq = x[d] * x[d];
    two += sq;
  }
  V[(size_t)i * K + 0] = -one;
  V[(size_t)i * K + 1] = -two;
  bool bad = !isfinite(one) || !isfinite(two);
  if (K == 3) {
    for (int d = 0; d < N; d++) {
      const double t = x[d] - 2.0;
      const double t2 = t * t;
      three += t2;
    }
    V[(size_t)i * K + 2] = -three;
    bad = bad || !isfinite(three);
  }
  if (bad) atomicOr(&sc->errors, KG_ERR_NONFINITE_F);
}

__global__ void k_mo_add_evals(MoScalars *sc, double n) { sc->modelEvaluationCount += n; }

// -------------------------------------------------------------------- sort
// sortSampleIndices, first half (:234-268), over the n = 2P merged values.
// A round computes, for every unranked i, maxNBetter[i] = max over unranked
// j != i of #{k : v_ik < v_jk} (the reference's criterion, not textbook
// dominance), and ranks the unranked i whose maxNBetter equals the minimum.
// Every round with something unranked ranks at least the minimum's owner, so
// the reference's r = n, n-1, ... are consecutive rounds and its remaining
// rounds are empty; after the offset (:266-268) round t has rank
// rounds - 1 - t.  rnd[i] = the round that ranked i.
//
// One workgroup, values and round numbers in LDS (n <= MO_1WG_MAX).
__global__ void __launch_bounds__(MO_TPB) k_mo_peel_1wg(int P, int K, const double *__restrict__ Vc,
                                                        const double *__restrict__ Vp, int *__restrict__ rndOut,
                                                        MoSort *so) {
  extern __shared__ double lds[];
  __shared__ int redA[MO_TPB], redB[MO_TPB];
  const int n = 2 * P, tid = threadIdx.x;
  double *v = lds;                   // n x K
  int *rnd = (int *)(lds + (size_t)n * K);  // n
  int *mx = rnd + n;                 // n
  for (int e = tid; e < n * K; e += MO_TPB) v[e] = merged(Vc, Vp, P, K, e / K, e % K);
  for (int i = tid; i < n; i += MO_TPB) rnd[i] = -1;
  __syncthreads();
  int t = 0;
  for (;; t++) {
    int cnt = 0, mn = K;  // minMaxNBetter starts at _numObjectives (:239)
    for (int i = tid; i < n; i += MO_TPB) {
      if (rnd[i] >= 0) continue;
      cnt++;
      int m = 0;
      for (int j = 0; j < n; j++) {
        if (rnd[j] >= 0) continue;  // (j == i counts 0: v_ik < v_ik never holds)
        int nb = 0;
        for (int k = 0; k < K; k++) nb += v[i * K + k] < v[j * K + k] ? 1 : 0;
        m = nb > m ? nb : m;
      }
      mx[i] = m;
      mn = m < mn ? m : mn;
    }
    redA[tid] = cnt;
    redB[tid] = mn;
    __syncthreads();
    for (int s = MO_TPB / 2; s > 0; s >>= 1) {
      if (tid < s) {
        redA[tid] += redA[tid + s];
        redB[tid] = redB[tid + s] < redB[tid] ? redB[tid + s] : redB[tid];
      }
      __syncthreads();
    }
    const int left = redA[0], minMax = redB[0];
    __syncthreads();  // redA / redB free
    if (left == 0) break;
    for (int i = tid; i < n; i += MO_TPB)
      if (rnd[i] < 0 && mx[i] == minMax) rnd[i] = t;
    __syncthreads();
  }
  for (int i = tid; i < n; i += MO_TPB) rndOut[i] = rnd[i];
  if (tid == 0) so->rounds = t;
}

// The same round over several workgroups (n > MO_1WG_MAX), two launches per
// round: `a` computes maxNBetter and the minimum, `b` ranks and counts what is
// left for round t + 1.  left[t] = unranked samples before round t; both
// launches exit at once when it is 0, so a batch queued past the last round
// costs empty launches only.
__global__ void __launch_bounds__(MO_TPB) k_mo_peel_a(int P, int K, int t, const double *__restrict__ Vc,
                                                      const double *__restrict__ Vp, const int *__restrict__ rnd,
                                                      int *__restrict__ mx, const int *__restrict__ left,
                                                      int *__restrict__ minMax) {
  if (left[t] == 0) return;
  const int n = 2 * P, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || rnd[i] >= 0) return;
  double vi[MO_MAXK];  // (indexed by unrolled constants only: no runtime-indexed registers)
#pragma unroll
  for (int k = 0; k < MO_MAXK; k++) vi[k] = k < K ? merged(Vc, Vp, P, K, i, k) : 0.0;
  int m = 0;
  for (int j = 0; j < n; j++) {
    if (rnd[j] >= 0) continue;
    int nb = 0;
#pragma unroll
    for (int k = 0; k < MO_MAXK; k++)
      if (k < K) nb += vi[k] < merged(Vc, Vp, P, K, j, k) ? 1 : 0;
    m = nb > m ? nb : m;
  }
  mx[i] = m;
  atomicMin(&minMax[t], m);
}

__global__ void __launch_bounds__(MO_TPB) k_mo_peel_b(int n, int t, int *__restrict__ rnd, const int *__restrict__ mx,
                                                      int *__restrict__ left, const int *__restrict__ minMax) {
  if (left[t] == 0) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || rnd[i] >= 0) return;
  if (mx[i] == minMax[t])
    rnd[i] = t;
  else
    atomicAdd(&left[t + 1], 1);
}

// left[0] = n, left[t > 0] = 0, minMax[t] = K (:239), rnd = -1
__global__ void k_mo_peel_init(int n, int K, int *rnd, int *left, int *minMax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  left[i] = i == 0 ? n : 0;
  minMax[i] = K;
  if (i < n) rnd[i] = -1;
}

// the reference point (:270-275): the minimum per objective, from +Inf with <
__global__ void __launch_bounds__(MO_TPB) k_mo_reference(int P, int K, int rounds, const double *__restrict__ Vc,
                                                         const double *__restrict__ Vp, MoSort *so) {
  __shared__ double red[MO_TPB];
  const int n = 2 * P, tid = threadIdx.x;
  for (int k = 0; k < K; k++) {
    double m = INFINITY;
    for (int i = tid; i < n; i += MO_TPB) {
      const double x = merged(Vc, Vp, P, K, i, k);
      if (x < m) m = x;
    }
    red[tid] = m;
    __syncthreads();
    for (int s = MO_TPB / 2; s > 0; s >>= 1) {
      if (tid < s && red[tid + s] < red[tid]) red[tid] = red[tid + s];
      __syncthreads();
    }
    if (tid == 0) so->reference[k] = red[0];
    __syncthreads();
  }
  if (tid == 0 && rounds >= 0) so->rounds = rounds;
}

// sortSampleIndices, second half (:277-329): within a rank group the samples
// are picked one by one, each time the first strict maximum (in ascending
// index) of the contribution sum_k (max_{j != i, unsorted} v_jk - reference_k),
// summed over k from 0.0 in order, and recomputed after every pick.  The
// exclusive upper bound max_{j != i} needs only the group's largest value,
// its multiplicity and the largest value below it, per objective: it is the
// largest value unless i alone holds it, then the next one (-Inf when the
// group has no other value, as the reference's initial -Inf).  Rank groups
// are independent: workgroup g orders the group of round g, whose first order
// is the number of samples in later rounds (lower ranks, :281).
struct MoTop {
  double t1, t2;
  int c;
};
__device__ inline MoTop mo_top_merge(MoTop a, MoTop b) {
  if (a.c == 0) return b;
  if (b.c == 0) return a;
  MoTop r;
  if (a.t1 == b.t1) {
    r.t1 = a.t1;
    r.c = a.c + b.c;
    r.t2 = a.t2 > b.t2 ? a.t2 : b.t2;
  } else if (a.t1 > b.t1) {
    r.t1 = a.t1;
    r.c = a.c;
    r.t2 = a.t2 > b.t1 ? a.t2 : b.t1;
  } else {
    r.t1 = b.t1;
    r.c = b.c;
    r.t2 = b.t2 > a.t1 ? b.t2 : a.t1;
  }
  return r;
}

__global__ void __launch_bounds__(MO_TPB) k_mo_hv(int P, int K, const double *__restrict__ Vc,
                                                  const double *__restrict__ Vp, const int *__restrict__ rnd,
                                                  const MoSort *so, int *__restrict__ members,
                                                  int *__restrict__ order) {
  __shared__ MoTop red[MO_TPB];
  __shared__ double redV[MO_TPB];
  __shared__ int redI[MO_TPB];
  __shared__ MoTop top[MO_MAXK];
  __shared__ int firstAlive;
  const int n = 2 * P, tid = threadIdx.x, g = blockIdx.x;
  if (g >= so->rounds) return;
  // the group's members in ascending index at members[offset ...), offset =
  // samples of later rounds
  int offset = 0;
  for (int i = tid; i < n; i += MO_TPB) offset += rnd[i] > g ? 1 : 0;
  redI[tid] = offset;
  __syncthreads();
  for (int s = MO_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) redI[tid] += redI[tid + s];
    __syncthreads();
  }
  offset = redI[0];
  __syncthreads();
  int size = 0;
  for (int base = 0; base < n; base += MO_TPB) {
    const int i = base + tid;
    const bool mine = i < n && rnd[i] == g;
    int tot;
    const int at = block_scan_flag(mine, &tot);
    if (mine) members[offset + size + at] = i;
    size += tot;
  }
  __syncthreads();
  int *mem = members + offset;  // a picked member becomes -1 - index
  __shared__ double ref[MO_MAXK];
  if (tid < K) ref[tid] = so->reference[tid];
  __syncthreads();
  for (int pick = 0; pick < size; pick++) {
    // per objective: largest value, its multiplicity, the next value; and the
    // first unsorted member
    int fa = size;
    for (int k = 0; k < K; k++) {
      MoTop a{-INFINITY, -INFINITY, 0};
      for (int m = tid; m < size; m += MO_TPB) {
        const int i = mem[m];
        if (i < 0) continue;
        if (k == 0 && m < fa) fa = m;
        a = mo_top_merge(a, MoTop{merged(Vc, Vp, P, K, i, k), -INFINITY, 1});
      }
      red[tid] = a;
      if (k == 0) redI[tid] = fa;
      __syncthreads();
      for (int s = MO_TPB / 2; s > 0; s >>= 1) {
        if (tid < s) {
          red[tid] = mo_top_merge(red[tid], red[tid + s]);
          if (k == 0 && redI[tid + s] < redI[tid]) redI[tid] = redI[tid + s];
        }
        __syncthreads();
      }
      if (tid == 0) {
        top[k] = red[0];
        if (k == 0) firstAlive = redI[0];
      }
      __syncthreads();
    }
    const int first = firstAlive;
    // contributions and the first strict maximum: the reference starts from
    // the first unsorted member and replaces it only when contribution >
    // current holds, so a NaN first contribution ((-Inf) - (-Inf), the first
    // generation's Previous Values) stays and a later NaN never wins
    double bestV = -INFINITY;
    int bestM = size;
    for (int m = tid; m < size; m += MO_TPB) {
      const int i = mem[m];
      if (i < 0) continue;
      double c = 0.0;
      for (int k = 0; k < K; k++) {
        const double x = merged(Vc, Vp, P, K, i, k);
        const double ubk = (x == top[k].t1 && top[k].c == 1) ? top[k].t2 : top[k].t1;
        c += (ubk - ref[k]);
      }
      if (isnan(c)) c = m == first ? INFINITY : -INFINITY;
      if (bestM == size || c > bestV) {  // ascending m per thread: ties keep the lower
        bestV = c;
        bestM = m;
      }
    }
    redV[tid] = bestV;
    redI[tid] = bestM;
    __syncthreads();
    for (int s = MO_TPB / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const int om = redI[tid + s];
        const double ov = redV[tid + s];
        if (om < size && (redI[tid] == size || ov > redV[tid] || (ov == redV[tid] && om < redI[tid]))) {
          redV[tid] = ov;
          redI[tid] = om;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const int m = redI[0];
      const int i = mem[m];
      order[i] = offset + pick;  // :322
      mem[m] = -1 - i;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ update
// updateDistribution :343-378 for offspring i, fused with the copy from its
// parent (:220-227): reads the parent's covariance once, writes the
// offspring's once.
__global__ void __launch_bounds__(MO_TPB) k_mo_update(MoConst c, const int *__restrict__ order,
                                                      const double *__restrict__ parentIdx,
                                                      const double *__restrict__ X, const double *__restrict__ pX,
                                                      const double *__restrict__ pSg, const double *__restrict__ pC,
                                                      const double *__restrict__ pPa, const double *__restrict__ pSr,
                                                      double *__restrict__ Sg, double *__restrict__ Cm,
                                                      double *__restrict__ Pa, double *__restrict__ Sr) {
  __shared__ double path[MO_MAXN];
  __shared__ double lenS;
  const int i = blockIdx.x, tid = threadIdx.x, N = c.N;
  int p = (int)parentIdx[i];
  p = p < 0 ? 0 : (p >= c.mu ? c.mu - 1 : p);
  const double *Cp = pC + (size_t)p * N * N;
  const double sigma = pSg[p];
  // success rate (:350-352)
  double sr = pSr[p] * (1. - c.cp);
  if (order[i] >= c.n - c.mu) sr += c.cp;
  sr = 1.0 < sr ? 1.0 : sr;
  // evolution path (:355-359)
  if (tid < N) {
    const int d = tid;
    double e = (1. - c.cc) * pPa[(size_t)p * N + d];
    const double a = c.pathFactor / sqrt(Cp[(size_t)d * N + d]);
    const double diff = X[(size_t)i * N + d] - pX[(size_t)p * N + d];
    const double b = a * diff;
    const double q = b / sigma;
    e += q;
    path[d] = e;
    Pa[(size_t)i * N + d] = e;
  }
  __syncthreads();
  if (tid == 0) {
    const double l2 = ordered_sum(0.0, N, [&](int d) { return path[d] * path[d]; });  // :360-362
    lenS = sqrt(l2);
  }
  __syncthreads();
  // covariance (:365-374)
  const bool boost = sr >= c.target;
  const double g = c.ccov * c.pathFactor * c.pathFactor;
  double *Co = Cm + (size_t)i * N * N;
  for (int e = tid; e < N * N; e += MO_TPB) {
    const int d = e / N, f = e % N;
    const double keep = (1. - c.ccov) * Cp[e];
    const double r1 = c.ccov * path[d] * path[f];
    double v = keep + r1;
    if (boost) {
      const double extra = g * v;
      v += extra;
    }
    Co[e] = v;
  }
  if (tid == 0) {
    Sr[i] = sr;
    Sg[i] = sigma * exp_cr(c.cc / c.damp * (lenS / c.chiN - 1.0));  // :377
  }
}

// ------------------------------------------------------------ parent gather
// :381-407.  Merged sample i is a parent when its order is among the last mu.
// descending (the snapshot): slot n - order - 1.  recorded: the ordinal among
// the selected in ascending merged index (the reference's committed 2021
// result files were written that way).  Rows come from Current (i < P) or
// Previous (i >= P).
__global__ void __launch_bounds__(MO_TPB) k_mo_gather(MoConst c, int recorded, const int *__restrict__ order,
                                                      const double *__restrict__ Xc, const double *__restrict__ Xp,
                                                      const double *__restrict__ Sgc, const double *__restrict__ Sgp,
                                                      const double *__restrict__ Cc, const double *__restrict__ Cp,
                                                      const double *__restrict__ Pac, const double *__restrict__ Pap,
                                                      const double *__restrict__ Src, const double *__restrict__ Srp,
                                                      double *__restrict__ pX, double *__restrict__ pSg,
                                                      double *__restrict__ pC, double *__restrict__ pPa,
                                                      double *__restrict__ pSr) {
  __shared__ int red[MO_TPB];
  const int i = blockIdx.x, tid = threadIdx.x, N = c.N, first = c.n - c.mu;
  if (order[i] < first) return;
  int slot = c.n - order[i] - 1;
  if (recorded) {
    int before = 0;
    for (int j = tid; j < i; j += MO_TPB) before += order[j] >= first ? 1 : 0;
    red[tid] = before;
    __syncthreads();
    for (int s = MO_TPB / 2; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    slot = red[0];
  }
  if (slot < 0 || slot >= c.mu) return;  // (cannot happen: order is a permutation of 0..n-1)
  const bool cur = i < c.P;
  const size_t j = cur ? i : i - c.P;
  const double *X = cur ? Xc : Xp, *Sg = cur ? Sgc : Sgp, *C = cur ? Cc : Cp, *Pa = cur ? Pac : Pap,
               *Sr = cur ? Src : Srp;
  for (int e = tid; e < N * N; e += MO_TPB) pC[(size_t)slot * N * N + e] = C[j * N * N + e];
  if (tid < N) {
    pX[(size_t)slot * N + tid] = X[j * N + tid];
    pPa[(size_t)slot * N + tid] = Pa[j * N + tid];
  }
  if (tid == 0) {
    pSg[slot] = Sg[j];
    pSr[slot] = Sr[j];
  }
}

// -------------------------------------------------------------- statistics
// updateStatistics :412-448, one workgroup per objective k: Previous Best =
// Current Best, then the first strict maximum over the samples in index
// order; the differences follow the last maximum taken, which is that one.
__global__ void __launch_bounds__(MO_TPB) k_mo_best(int N, int P, int K, const double *__restrict__ V,
                                                    const double *__restrict__ X, double *__restrict__ bestEverV,
                                                    double *__restrict__ bestEverX, double *__restrict__ prevBestV,
                                                    double *__restrict__ prevBestX, double *__restrict__ curBestV,
                                                    double *__restrict__ curBestX, double *__restrict__ dV,
                                                    double *__restrict__ dX) {
  __shared__ double rv[MO_TPB];
  __shared__ int ri[MO_TPB];
  __shared__ double diff[MO_MAXN];
  const int k = blockIdx.x, tid = threadIdx.x;
  const int chunk = (P + MO_TPB - 1) / MO_TPB, i0 = tid * chunk, i1 = min(P, i0 + chunk);
  double bv = -INFINITY;
  int bi = -1;
  for (int i = i0; i < i1; i++) {
    const double v = V[(size_t)i * K + k];
    if (v > bv) {  // from -Inf (:416), strict (:425)
      bv = v;
      bi = i;
    }
  }
  rv[tid] = bv;
  ri[tid] = bi;
  __syncthreads();
  for (int s = MO_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) {
      // strictly larger wins; of equal values the lower index (a slot holds
      // indices of both halves after the first step)
      const int oi = ri[tid + s];
      const double ov = rv[tid + s];
      if (oi >= 0 && (ri[tid] < 0 || ov > rv[tid] || (ov == rv[tid] && oi < ri[tid]))) {
        rv[tid] = ov;
        ri[tid] = oi;
      }
    }
    __syncthreads();
  }
  const int best = ri[0];
  const double cur = rv[0];
  const double prev = curBestV[k];
  __syncthreads();
  double px = 0.0, cx = 0.0;
  if (tid < N) {
    px = curBestX[(size_t)k * N + tid];
    prevBestX[(size_t)k * N + tid] = px;  // :413-414
    if (best >= 0) {
      cx = X[(size_t)best * N + tid];
      curBestX[(size_t)k * N + tid] = cx;  // :428
      const double t = px - cx;
      diff[tid] = t * t;  // std::pow(., 2.) (:433)
    }
  }
  __syncthreads();
  if (tid == 0) {
    prevBestV[k] = prev;  // :412
    curBestV[k] = cur;    // :416, :427
    if (best >= 0) {
      dV[k] = cur - prev;  // :429
      const double l2 = ordered_sum(0.0, N, [&](int d) { return diff[d]; });
      dX[k] = sqrt(l2);  // :435
    }
  }
  // :441-448
  if (best >= 0 && cur > bestEverV[k]) {
    __syncthreads();
    if (tid < N) bestEverX[(size_t)k * N + tid] = cx;
    if (tid == 0) bestEverV[k] = cur;
  }
}

// :451-459 with _currentSigma[d] as written (the offspring index of the
// covariance, the VARIABLE index of sigma: N <= P is checked at create), and
// the non-dominated candidates (:462-477): i is dominated when some j != i is
// strictly larger in all K objectives
__global__ void __launch_bounds__(MO_TPB) k_mo_sdev_nondom(int N, int P, int K, const double *__restrict__ Sg,
                                                           const double *__restrict__ Cm,
                                                           const double *__restrict__ V, double *__restrict__ minSd,
                                                           double *__restrict__ maxSd, int *__restrict__ cand) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  double mx = -INFINITY, mn = INFINITY;
  for (int d = 0; d < N; d++) {
    const double sdev = Sg[d] * sqrt(Cm[(size_t)i * N * N + (size_t)d * N + d]);
    if (sdev > mx) mx = sdev;
    if (sdev < mn) mn = sdev;
  }
  maxSd[i] = mx;
  minSd[i] = mn;
  double vi[MO_MAXK];
#pragma unroll
  for (int k = 0; k < MO_MAXK; k++) vi[k] = k < K ? V[(size_t)i * K + k] : 0.0;
  bool dominated = false;
  for (int j = 0; j < P && !dominated; j++) {
    int numdom = 0;  // (j == i counts 0)
#pragma unroll
    for (int k = 0; k < MO_MAXK; k++)
      if (k < K) numdom += V[(size_t)j * K + k] > vi[k] ? 1 : 0;
    dominated = numdom == K;
  }
  cand[i] = dominated ? 0 : 1;
}

// the archive merge's flags (:481-500): entry e < count is an archive row
// (kept unless a candidate is larger in all K), entry count + i is sample i
// (kept when it is a candidate and no archive row is larger in all K)
__global__ void __launch_bounds__(MO_TPB) k_mo_archive_flags(int P, int K, int count, const double *__restrict__ V,
                                                             const int *__restrict__ cand,
                                                             const double *__restrict__ AV, int *__restrict__ keep) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count + P) return;
  double me[MO_MAXK];
  bool kept = true;
  if (e < count) {
#pragma unroll
    for (int k = 0; k < MO_MAXK; k++) me[k] = k < K ? AV[(size_t)e * K + k] : 0.0;
    for (int i = 0; i < P && kept; i++) {
      if (!cand[i]) continue;
      int cdom = 0;
#pragma unroll
      for (int k = 0; k < MO_MAXK; k++)
        if (k < K) cdom += V[(size_t)i * K + k] > me[k] ? 1 : 0;
      kept = cdom != K;
    }
  } else {
    const int i = e - count;
    kept = cand[i] != 0;
#pragma unroll
    for (int k = 0; k < MO_MAXK; k++) me[k] = k < K ? V[(size_t)i * K + k] : 0.0;
    for (int j = 0; j < count && kept; j++) {
      int sdom = 0;
#pragma unroll
      for (int k = 0; k < MO_MAXK; k++)
        if (k < K) sdom += me[k] < AV[(size_t)j * K + k] ? 1 : 0;
      kept = sdom != K;
    }
  }
  keep[e] = kept ? 1 : 0;
}

// the stable compaction (:502-519): kept archive rows in order, then kept
// candidates in order, into the other archive buffer (capacity >= count + P,
// the host grows it before the launch).  One workgroup.
__global__ void __launch_bounds__(MO_TPB) k_mo_archive_compact(int N, int P, int K, int count,
                                                               const int *__restrict__ keep,
                                                               const int *__restrict__ cand,
                                                               const double *__restrict__ X,
                                                               const double *__restrict__ V,
                                                               const double *__restrict__ A,
                                                               const double *__restrict__ AV, double *__restrict__ B,
                                                               double *__restrict__ BV, MoScalars *sc) {
  const int tid = threadIdx.x, tot = count + P;
  int out = 0, nd = 0;
  for (int base = 0; base < tot; base += MO_TPB) {
    const int e = base + tid;
    const bool k = e < tot && keep[e] != 0;
    int t, t2;
    const int at = block_scan_flag(k, &t);
    (void)block_scan_flag(e >= count && e < tot && cand[e - count] != 0, &t2);
    nd += t2;
    if (k) {
      const double *x = e < count ? A + (size_t)e * N : X + (size_t)(e - count) * N;
      const double *v = e < count ? AV + (size_t)e * K : V + (size_t)(e - count) * K;
      for (int d = 0; d < N; d++) B[(size_t)(out + at) * N + d] = x[d];
      for (int q = 0; q < K; q++) BV[(size_t)(out + at) * K + q] = v[q];
    }
    out += t;
  }
  if (tid == 0) {
    sc->archiveCount = (double)out;
    sc->nonDominatedCount = (double)nd;  // :479
  }
}

}  // namespace kg

using namespace kg;

struct kg_mocmaes_s {
  kg_mocmaes_cfg cfg;
  MoConst c{};
  int N = 0, P = 0, mu = 0, K = 0;
  hipStream_t stream = nullptr;
  int cur = 0;  // which buffer set holds Current*
  double *X[2] = {}, *V[2] = {}, *Sg[2] = {}, *Cm[2] = {}, *Pa[2] = {}, *Sr[2] = {};
  double *pX = nullptr, *pSg = nullptr, *pC = nullptr, *pPa = nullptr, *pSr = nullptr;
  double *parentIdx = nullptr, *LT = nullptr, *lb = nullptr, *ub = nullptr, *sdev0 = nullptr;
  double *bestEverV = nullptr, *bestEverX = nullptr, *prevBestV = nullptr, *prevBestX = nullptr, *curBestV = nullptr,
         *curBestX = nullptr, *dV = nullptr, *dX = nullptr, *minSd = nullptr, *maxSd = nullptr;
  double *A[2] = {}, *AV[2] = {};
  int arc = 0;  // which archive buffer is current
  size_t archiveCap = 0, archiveCount = 0;
  double *z = nullptr, *ubuf = nullptr;
  unsigned long long *blockEnd = nullptr;
  int *used = nullptr, *ok = nullptr, *rnd = nullptr, *mx = nullptr, *left = nullptr, *minMax = nullptr,
      *members = nullptr, *order = nullptr, *cand = nullptr, *keep = nullptr;
  size_t keepCap = 0;
  MoScalars *sc = nullptr;
  MoChain *chain = nullptr;
  MoSort *so = nullptr;
  double sigma0 = 0, minSdev0 = 0, maxSdev0 = 0;
  size_t window = 0, maxWindows = 0, windowsLast = 0, roundsLast = 0;
  bool initialized = false;
  MtStream normal, uniform;
  StageTimes times;
};

namespace {

struct MoField {
  void *dev = nullptr;
  size_t n = 0;
  bool archive = false;
};

bool mo_field(kg_mocmaes_s *h, const char *name, MoField &f) {
  const std::string k = name ? name : "";
  const size_t N = h->N, P = h->P, mu = h->mu, K = h->K;
  const int c = h->cur, p = 1 - h->cur;
  auto vec = [&](double *ptr, size_t n) {
    f.dev = ptr;
    f.n = n;
    return true;
  };
  if (k == "Current Sample Population") return vec(h->X[c], P * N);
  if (k == "Previous Sample Population") return vec(h->X[p], P * N);
  if (k == "Parent Sample Population") return vec(h->pX, mu * N);
  if (k == "Current Values") return vec(h->V[c], P * K);
  if (k == "Previous Values") return vec(h->V[p], P * K);
  if (k == "Parent Index") return vec(h->parentIdx, P);
  if (k == "Current Sigma") return vec(h->Sg[c], P);
  if (k == "Previous Sigma") return vec(h->Sg[p], P);
  if (k == "Parent Sigma") return vec(h->pSg, mu);
  if (k == "Current Covariance Matrix") return vec(h->Cm[c], P * N * N);
  if (k == "Previous Covariance Matrix") return vec(h->Cm[p], P * N * N);
  if (k == "Parent Covariance Matrix") return vec(h->pC, mu * N * N);
  if (k == "Current Evolution Paths") return vec(h->Pa[c], P * N);
  if (k == "Previous Evolution Paths") return vec(h->Pa[p], P * N);
  if (k == "Parent Evolution Paths") return vec(h->pPa, mu * N);
  if (k == "Current Success Probabilities") return vec(h->Sr[c], P);
  if (k == "Previous Success Probabilities") return vec(h->Sr[p], P);
  if (k == "Parent Success Probabilities") return vec(h->pSr, mu);
  if (k == "Best Ever Values") return vec(h->bestEverV, K);
  if (k == "Best Ever Variables Vector") return vec(h->bestEverX, K * N);
  if (k == "Previous Best Values") return vec(h->prevBestV, K);
  if (k == "Previous Best Variables Vector") return vec(h->prevBestX, K * N);
  if (k == "Current Best Values") return vec(h->curBestV, K);
  if (k == "Current Best Variables Vector") return vec(h->curBestX, K * N);
  if (k == "Current Best Value Differences") return vec(h->dV, K);
  if (k == "Current Best Variable Differences") return vec(h->dX, K);
  if (k == "Current Min Standard Deviations") return vec(h->minSd, P);
  if (k == "Current Max Standard Deviations") return vec(h->maxSd, P);
  if (k == "Current Non Dominated Sample Count") return vec(&h->sc->nonDominatedCount, 1);
  if (k == "Infeasible Sample Count") return vec(&h->sc->infeasibleSampleCount, 1);
  if (k == "Finished Sample Count") return vec(&h->sc->finishedSampleCount, 1);
  if (k == "Model Evaluation Count") return vec(&h->sc->modelEvaluationCount, 1);
  f.archive = true;
  if (k == "Sample Collection") return vec(h->A[h->arc], h->archiveCount * N);
  if (k == "Sample Value Collection") return vec(h->AV[h->arc], h->archiveCount * K);
  f.archive = false;
  return false;
}

// both archive buffers hold at least `rows` rows; the current one keeps its content
int mo_archive_reserve(kg_mocmaes_s *h, size_t rows) {
  if (rows <= h->archiveCap) return 0;
  const size_t cap = std::max(rows, 2 * h->archiveCap);
  const size_t N = h->N, K = h->K;
  double *a[2] = {}, *av[2] = {};
  for (int q = 0; q < 2; q++)
    if (dalloc(&a[q], cap * N) || dalloc(&av[q], cap * K)) return 1;
  // on the handle's stream: a copy on the null stream would not order against it
  if (h->archiveCount) {
    KG_HIP(hipMemcpyAsync(a[h->arc], h->A[h->arc], h->archiveCount * N * sizeof(double), hipMemcpyDeviceToDevice,
                          h->stream));
    KG_HIP(hipMemcpyAsync(av[h->arc], h->AV[h->arc], h->archiveCount * K * sizeof(double), hipMemcpyDeviceToDevice,
                          h->stream));
  }
  for (int q = 0; q < 2; q++) {
    if (h->A[q]) dev_release(h->A[q], h->stream);
    if (h->AV[q]) dev_release(h->AV[q], h->stream);
    h->A[q] = a[q];
    h->AV[q] = av[q];
  }
  h->archiveCap = cap;
  return 0;
}

int mo_fill(kg_mocmaes_s *h, double *p, size_t n, double v) {
  if (!n) return 0;
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, p, n, v);
  KG_HIP(hipGetLastError());
  return 0;
}

size_t peel_lds_bytes(int n, int K) { return (size_t)n * K * sizeof(double) + 2 * (size_t)n * sizeof(int); }

// sortSampleIndices over Current Values ++ Previous Values -> h->order
int mo_sort(kg_mocmaes_s *h) {
  const int P = h->P, K = h->K, n = 2 * P;
  const double *Vc = h->V[h->cur], *Vp = h->V[1 - h->cur];
  int grid = n, rounds = -1;
  if (n <= MO_1WG_MAX) {
    hipLaunchKernelGGL(k_mo_peel_1wg, dim3(1), dim3(MO_TPB), peel_lds_bytes(n, K), h->stream, P, K, Vc, Vp, h->rnd,
                       h->so);
    KG_HIP(hipGetLastError());
  } else {
    const unsigned blocks = (unsigned)((n + MO_TPB) / MO_TPB);
    hipLaunchKernelGGL(k_mo_peel_init, dim3(blocks), dim3(MO_TPB), 0, h->stream, n, K, h->rnd, h->left, h->minMax);
    KG_HIP(hipGetLastError());
    int t = 0;
    std::vector<int> left(MO_PEEL_BATCH + 1);
    for (;;) {
      const int t1 = std::min(n, t + MO_PEEL_BATCH);
      for (int r = t; r < t1; r++) {
        hipLaunchKernelGGL(k_mo_peel_a, dim3(blocks), dim3(MO_TPB), 0, h->stream, P, K, r, Vc, Vp,
                           (const int *)h->rnd, h->mx, (const int *)h->left, h->minMax);
        KG_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_mo_peel_b, dim3(blocks), dim3(MO_TPB), 0, h->stream, n, r, h->rnd, (const int *)h->mx,
                           h->left, (const int *)h->minMax);
        KG_HIP(hipGetLastError());
      }
      // one read per batch: left[t+1 .. t1]
      KG_HIP(hipMemcpyAsync(left.data(), h->left + t + 1, (size_t)(t1 - t) * sizeof(int), hipMemcpyDeviceToHost,
                            h->stream));
      KG_HIP(hipStreamSynchronize(h->stream));
      rounds = -1;
      for (int r = t; r < t1 && rounds < 0; r++)
        if (left[r - t] == 0) rounds = r + 1;
      if (rounds >= 0) break;
      KG_CHECK(t1 < n, "MOCMAES: the rank peeling did not finish");  // (every round ranks at least one sample)
      t = t1;
    }
    grid = rounds;
  }
  hipLaunchKernelGGL(k_mo_reference, dim3(1), dim3(MO_TPB), 0, h->stream, P, K, rounds, Vc, Vp, h->so);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mo_hv, dim3(grid), dim3(MO_TPB), 0, h->stream, P, K, Vc, Vp, (const int *)h->rnd,
                     (const MoSort *)h->so, h->members, h->order);
  KG_HIP(hipGetLastError());
  h->roundsLast = rounds < 0 ? 0 : (size_t)rounds;
  return 0;
}

// updateStatistics (:410-520)
int mo_statistics(kg_mocmaes_s *h) {
  const int N = h->N, P = h->P, K = h->K, c = h->cur;
  hipLaunchKernelGGL(k_mo_best, dim3(K), dim3(MO_TPB), 0, h->stream, N, P, K, (const double *)h->V[c],
                     (const double *)h->X[c], h->bestEverV, h->bestEverX, h->prevBestV, h->prevBestX, h->curBestV,
                     h->curBestX, h->dV, h->dX);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mo_sdev_nondom, dim3((P + MO_TPB - 1) / MO_TPB), dim3(MO_TPB), 0, h->stream, N, P, K,
                     (const double *)h->Sg[c], (const double *)h->Cm[c], (const double *)h->V[c], h->minSd, h->maxSd,
                     h->cand);
  KG_HIP(hipGetLastError());
  const size_t count = h->archiveCount, tot = count + P;
  if (mo_archive_reserve(h, tot)) return 1;
  if (tot > h->keepCap) {
    int *nk = nullptr;
    if (dalloc(&nk, 2 * tot)) return 1;
    if (h->keep) dev_release(h->keep, h->stream);
    h->keep = nk;
    h->keepCap = 2 * tot;
  }
  const int a = h->arc;
  hipLaunchKernelGGL(k_mo_archive_flags, dim3((unsigned)((tot + MO_TPB - 1) / MO_TPB)), dim3(MO_TPB), 0, h->stream, P,
                     K, (int)count, (const double *)h->V[c], (const int *)h->cand, (const double *)h->AV[a], h->keep);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mo_archive_compact, dim3(1), dim3(MO_TPB), 0, h->stream, N, P, K, (int)count,
                     (const int *)h->keep, (const int *)h->cand, (const double *)h->X[c], (const double *)h->V[c],
                     (const double *)h->A[a], (const double *)h->AV[a], h->A[1 - a], h->AV[1 - a], h->sc);
  KG_HIP(hipGetLastError());
  h->arc = 1 - a;
  // the one read per generation: the archive's new size
  double cnt = 0;
  KG_HIP(hipMemcpyAsync(&cnt, &h->sc->archiveCount, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->archiveCount = (size_t)cnt;
  return 0;
}

}  // namespace

extern "C" {

int kg_mocmaes_create(const kg_mocmaes_cfg *cfg, kg_mocmaes_t *out) {
  KG_CHECK(cfg && out, "kg_mocmaes_create: null argument");
  KG_CHECK(cfg->variable_count >= 1, "'Variable Count' must be >= 1");
  const size_t N = cfg->variable_count;
  // setInitialConfiguration :24-27
  const size_t P = cfg->population_size ? cfg->population_size
                                        : (size_t)std::ceil(4. + std::floor(3. * std::log((double)N)));
  const size_t mu = cfg->mu_value ? cfg->mu_value : (size_t)(P / 2.);
  const size_t K = cfg->num_objectives;
  KG_CHECK(K >= 2, "Problem requires multiple objectives, 'Num Objectives' is set to " + std::to_string(K));  // :20-21
  KG_CHECK(K <= MO_MAXK, "MOCMAES: 'Num Objectives' above 8 is not supported on the device");
  KG_CHECK(P < (1u << 22), "MOCMAES: 'Population Size' too large");
  KG_CHECK(mu <= P, "Number of parents ('Mu Value' " + std::to_string(mu) +
                        ") must be smaller or equal with population size (" + std::to_string(P) + ").");  // :26-27
  KG_CHECK(mu >= 1, "MOCMAES: 'Mu Value' must be at least 1");
  KG_CHECK(N <= MO_MAXN, "MOCMAES: more than 128 variables are not supported on the device (the covariance factor "
                         "is kept in LDS)");
  KG_CHECK(N <= P, "MOCMAES: 'Population Size' must be at least the variable count: updateStatistics reads "
                   "_currentSigma[d] for every variable d (MOCMAES.cpp.base:455), out of bounds otherwise");
  KG_CHECK(cfg->success_learning_rate > 0. && cfg->success_learning_rate <= 1.,
           "Invalid Global Success Learning Rate, must be greater than 0.0 and less or equal to 1.0");  // :129-130
  KG_CHECK(cfg->target_success_rate > 0. && cfg->target_success_rate <= 1.,
           "Invalid Target Success Rate, must be greater than 0.0 and less or equal to 1.0");  // :131-132
  KG_CHECK(cfg->parent_order == KG_MOCMAES_PARENTS_DESCENDING || cfg->parent_order == KG_MOCMAES_PARENTS_RECORDED,
           "unknown MOCMAES parent order");
  KG_CHECK(cfg->lower_bound && cfg->upper_bound, "MOCMAES needs the variables' 'Lower Bound' and 'Upper Bound'");
  std::vector<double> sdev(N);
  double trace = 0., minSdev = INFINITY, maxSdev = -INFINITY;
  for (size_t d = 0; d < N; d++) {
    const double lo = cfg->lower_bound[d], hi = cfg->upper_bound[d];
    KG_CHECK(!std::isnan(lo) && !std::isnan(hi), "MOCMAES needs the variables' 'Lower Bound' and 'Upper Bound' (a bound is NaN)");
    const bool needValue = !(cfg->initial_value && std::isfinite(cfg->initial_value[d]));
    const bool needSdev = !(cfg->initial_sdev && std::isfinite(cfg->initial_sdev[d]));
    // :73-85
    KG_CHECK(!(needValue || needSdev) || (std::isfinite(lo) && std::isfinite(hi)),
             "Initial (Mean) Value or Initial Standard Deviation of variable " + std::to_string(d) +
                 " not defined, and cannot be inferred because a variable bound is not finite.");
    sdev[d] = needSdev ? (hi - lo) * 0.3 : cfg->initial_sdev[d];
    trace += sdev[d] * sdev[d];
    if (sdev[d] < minSdev) minSdev = sdev[d];
    if (sdev[d] > maxSdev) maxSdev = sdev[d];
  }
  KG_HIP(hipSetDevice(cfg->device));
  upload_dd_tables();  // log_cr of the polar normals, exp_cr of the step size
  auto *h = new kg_mocmaes_s();
  h->cfg = *cfg;
  h->cfg.lower_bound = h->cfg.upper_bound = h->cfg.initial_value = h->cfg.initial_sdev = nullptr;
  h->N = (int)N;
  h->P = (int)P;
  h->mu = (int)mu;
  h->K = (int)K;
  h->sigma0 = std::sqrt(trace / N);
  h->minSdev0 = minSdev;
  h->maxSdev0 = maxSdev;
  MoConst &c = h->c;
  c.N = (int)N;
  c.P = (int)P;
  c.mu = (int)mu;
  c.K = (int)K;
  c.n = 2 * (int)P;
  // :127-128, :343-345
  c.cc = cfg->evolution_path_adaption_strength < 0. ? 2. / (N + 2.) : cfg->evolution_path_adaption_strength;
  c.ccov = cfg->covariance_learning_rate < 0. ? 2. / (N * N + 6.) : cfg->covariance_learning_rate;
  c.cp = cfg->success_learning_rate;
  c.target = cfg->target_success_rate;
  c.pathFactor = std::sqrt(c.cc * (2. - c.cc));
  c.damp = 1.0 + 2.0 * std::max(0.0, std::sqrt((mu - 1.) / (N + 1.)) - 1.0) + c.cc;
  c.chiN = std::sqrt((double)N) * (1. - 1. / (4. * N) + 1. / (21. * N * N));
  // the first window holds one block per sample (the speculative pass) and some more
  h->window = std::max<size_t>(cfg->window_blocks, P + 64);
  h->maxWindows = cfg->max_windows ? cfg->max_windows : 1024;
  auto fail = [&]() {
    kg_mocmaes_destroy(h);
    return 1;
  };
  if (stream_acquire(&h->stream) != hipSuccess) {
    set_error("kg_mocmaes_create: no stream");
    return fail();
  }
  const size_t NN = N * N, n = 2 * P;
  for (int q = 0; q < 2; q++)
    if (dalloc(&h->X[q], P * N) || dalloc(&h->V[q], P * K) || dalloc(&h->Sg[q], P) || dalloc(&h->Cm[q], P * NN) ||
        dalloc(&h->Pa[q], P * N) || dalloc(&h->Sr[q], P))
      return fail();
  if (dalloc(&h->pX, mu * N) || dalloc(&h->pSg, mu) || dalloc(&h->pC, mu * NN) || dalloc(&h->pPa, mu * N) ||
      dalloc(&h->pSr, mu) || dalloc(&h->parentIdx, P) || dalloc(&h->LT, mu * NN) || dalloc(&h->lb, N) ||
      dalloc(&h->ub, N) || dalloc(&h->sdev0, N) || dalloc(&h->bestEverV, K) || dalloc(&h->bestEverX, K * N) ||
      dalloc(&h->prevBestV, K) || dalloc(&h->prevBestX, K * N) || dalloc(&h->curBestV, K) ||
      dalloc(&h->curBestX, K * N) || dalloc(&h->dV, K) || dalloc(&h->dX, K) || dalloc(&h->minSd, P) ||
      dalloc(&h->maxSd, P) || dalloc(&h->z, h->window * N) || dalloc(&h->ubuf, P) ||
      dalloc(&h->blockEnd, h->window) || dalloc(&h->used, mu) || dalloc(&h->ok, P) || dalloc(&h->rnd, n) ||
      dalloc(&h->mx, n) || dalloc(&h->left, n + 1) || dalloc(&h->minMax, n + 1) || dalloc(&h->members, n) ||
      dalloc(&h->order, n) || dalloc(&h->cand, P) || dalloc(&h->sc, 1) || dalloc(&h->chain, 1) || dalloc(&h->so, 1))
    return fail();
  if (mo_archive_reserve(h, cfg->archive_rows ? cfg->archive_rows : std::max<size_t>(4 * P, 1024))) return fail();
  if (hipMemcpy(h->lb, cfg->lower_bound, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->ub, cfg->upper_bound, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->sdev0, sdev.data(), N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_mocmaes_create: upload failed");
    return fail();
  }
  MoScalars sc{};
  if (hipMemcpy(h->sc, &sc, sizeof(sc), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_mocmaes_create: scalar upload failed");
    return fail();
  }
  if (allow_dynamic_lds((const void *)k_mo_factor, N * (N + 1) * sizeof(double)) != hipSuccess ||
      (n <= (size_t)MO_1WG_MAX &&
       allow_dynamic_lds((const void *)k_mo_peel_1wg, peel_lds_bytes((int)n, (int)K)) != hipSuccess)) {
    set_error("kg_mocmaes_create: kernel LDS");
    return fail();
  }
  if (h->normal.init(4 * h->normal.words_for_normals(h->window * N) + 16384)) return fail();
  if (h->uniform.init(8 * P + 16384)) return fail();
  unsigned char st[5000];
  gsl_seed_state(cfg->multinormal_seed, st);
  if (h->normal.import_gsl(st, h->stream)) return fail();
  gsl_seed_state(cfg->uniform_seed, st);
  if (h->uniform.import_gsl(st, h->stream)) return fail();
  *out = h;
  return 0;
}

int kg_mocmaes_destroy(kg_mocmaes_t h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->normal.drain();
  h->uniform.drain();
  for (int q = 0; q < 2; q++)
    for (void *p : {(void *)h->X[q], (void *)h->V[q], (void *)h->Sg[q], (void *)h->Cm[q], (void *)h->Pa[q],
                    (void *)h->Sr[q], (void *)h->A[q], (void *)h->AV[q]})
      if (p) dev_release(p);
  for (void *p : {(void *)h->pX,        (void *)h->pSg,       (void *)h->pC,        (void *)h->pPa,
                  (void *)h->pSr,       (void *)h->parentIdx, (void *)h->LT,        (void *)h->lb,
                  (void *)h->ub,        (void *)h->sdev0,     (void *)h->bestEverV, (void *)h->bestEverX,
                  (void *)h->prevBestV, (void *)h->prevBestX, (void *)h->curBestV,  (void *)h->curBestX,
                  (void *)h->dV,        (void *)h->dX,        (void *)h->minSd,     (void *)h->maxSd,
                  (void *)h->z,         (void *)h->ubuf,      (void *)h->blockEnd,  (void *)h->used,
                  (void *)h->ok,        (void *)h->rnd,       (void *)h->mx,        (void *)h->left,
                  (void *)h->minMax,    (void *)h->members,   (void *)h->order,     (void *)h->cand,
                  (void *)h->keep,      (void *)h->sc,        (void *)h->chain,     (void *)h->so})
    if (p) dev_release(p);
  h->times.release();
  if (h->stream) stream_release(h->stream);
  delete h;
  return 0;
}

int kg_mocmaes_initialize(kg_mocmaes_t h) {
  KG_CHECK(h, "kg_mocmaes_initialize: null handle");
  const size_t N = h->N, P = h->P, mu = h->mu, K = h->K, NN = N * N;
  // :29-61, :92-108: Current and Previous zero, their values -Inf
  for (int q = 0; q < 2; q++) {
    KG_HIP(hipMemsetAsync(h->X[q], 0, P * N * sizeof(double), h->stream));
    KG_HIP(hipMemsetAsync(h->Sg[q], 0, P * sizeof(double), h->stream));
    KG_HIP(hipMemsetAsync(h->Cm[q], 0, P * NN * sizeof(double), h->stream));
    KG_HIP(hipMemsetAsync(h->Pa[q], 0, P * N * sizeof(double), h->stream));
    KG_HIP(hipMemsetAsync(h->Sr[q], 0, P * sizeof(double), h->stream));
    if (mo_fill(h, h->V[q], P * K, -INFINITY)) return 1;
  }
  KG_HIP(hipMemsetAsync(h->parentIdx, 0, P * sizeof(double), h->stream));
  // :110-124 (the parents start at 0: the inferred 'Initial Value' is never read again)
  KG_HIP(hipMemsetAsync(h->pX, 0, mu * N * sizeof(double), h->stream));
  KG_HIP(hipMemsetAsync(h->pPa, 0, mu * N * sizeof(double), h->stream));
  hipLaunchKernelGGL(k_mo_init_parents, dim3((unsigned)((mu * NN + 255) / 256)), dim3(256), 0, h->stream, h->N, h->mu,
                     (const double *)h->sdev0, h->sigma0, h->c.target, h->pC, h->pSg, h->pSr);
  KG_HIP(hipGetLastError());
  for (double *p : {h->bestEverV, h->prevBestV, h->curBestV})
    if (mo_fill(h, p, K, -INFINITY)) return 1;
  for (double *p : {h->bestEverX, h->prevBestX, h->curBestX})
    KG_HIP(hipMemsetAsync(p, 0, K * N * sizeof(double), h->stream));
  // :135-139
  if (mo_fill(h, h->dV, K, INFINITY) || mo_fill(h, h->dX, K, INFINITY) || mo_fill(h, h->minSd, P, h->minSdev0) ||
      mo_fill(h, h->maxSd, P, h->maxSdev0))
    return 1;
  MoScalars sc{};
  sc.nonDominatedCount = 1.0;  // :29
  KG_HIP(hipMemcpyAsync(h->sc, &sc, sizeof(sc), hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));  // sc is on this stack
  h->archiveCount = 0;
  h->cur = 0;
  h->initialized = true;
  return 0;
}

int kg_mocmaes_prepare(kg_mocmaes_t h, size_t generation) {
  KG_CHECK(h, "kg_mocmaes_prepare: null handle");
  KG_CHECK(generation >= 1, "kg_mocmaes_prepare: generations count from 1");
  if (generation == 1 && !h->initialized && kg_mocmaes_initialize(h)) return 1;
  KG_CHECK(h->initialized,
           "kg_mocmaes_prepare: the handle holds no state (kg_mocmaes_initialize, or a restored state, first)");
  Stage st(h->times, h->stream, "draw");
  const int N = h->N, P = h->P, mu = h->mu;
  h->cur = 1 - h->cur;  // Previous* = Current* (:176-181)
  const int c = h->cur;
  KG_HIP(hipMemsetAsync(h->used, 0, (size_t)mu * sizeof(int), h->stream));
  const double *u = nullptr;
  if (mu != P) {
    if (h->uniform.uniforms(h->ubuf, P, h->stream)) return 1;
    u = h->ubuf;
  }
  hipLaunchKernelGGL(k_mo_pick, dim3((P + MO_TPB - 1) / MO_TPB), dim3(MO_TPB), 0, h->stream, P, mu, u,
                     (const MoScalars *)h->sc, h->parentIdx, h->used);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_mo_factor, dim3(mu), dim3(MO_TPB), (size_t)N * (N + 1) * sizeof(double), h->stream, N,
                     (const double *)h->pC, (const double *)h->pSg, (const int *)h->used, h->LT, h->sc);
  KG_HIP(hipGetLastError());
  KG_HIP(hipMemsetAsync(h->chain, 0, sizeof(MoChain), h->stream));
  h->windowsLast = 0;
  for (size_t w = 0;; w++) {
    MoChain ch{};
    if (w >= h->maxWindows) {
      KG_HIP(hipMemcpyAsync(&ch, h->chain, sizeof(ch), hipMemcpyDeviceToHost, h->stream));
      KG_HIP(hipStreamSynchronize(h->stream));
      set_error("MOCMAES: sample " + std::to_string(ch.sample) + " of generation " + std::to_string(generation) +
                " has no feasible draw after " + std::to_string(w) + " windows of " + std::to_string(h->window) +
                " draws: the reference would redraw forever");
      return 1;
    }
    if (h->normal.polar_normals(h->z, h->window * N, N, h->blockEnd, h->stream)) return 1;
    if (w == 0) {
      hipLaunchKernelGGL(k_mo_draw_spec, dim3(P), dim3(MO_MAXN), 0, h->stream, N, P, mu, (const double *)h->z,
                         (const double *)h->LT, (const double *)h->pX, (const double *)h->parentIdx,
                         (const double *)h->lb, (const double *)h->ub, h->X[c], h->ok);
      KG_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mo_draw_chain, dim3(1), dim3(MO_TPB), 0, h->stream, N, P, mu, w == 0 ? 1 : 0,
                       (const double *)h->z, (unsigned long long)h->window, (const double *)h->LT,
                       (const double *)h->pX, (const double *)h->parentIdx, (const double *)h->lb,
                       (const double *)h->ub, h->X[c], (const int *)h->ok, h->chain);
    KG_HIP(hipGetLastError());
    if (h->normal.consume_normals_dev(&h->chain->used, N, h->blockEnd, h->stream)) return 1;
    h->windowsLast++;
    KG_HIP(hipMemcpyAsync(&ch, h->chain, sizeof(ch), hipMemcpyDeviceToHost, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    if (ch.done) break;
  }
  MoScalars sc{};
  KG_HIP(hipMemcpy(&sc, h->sc, sizeof(sc), hipMemcpyDeviceToHost));
  KG_CHECK(!(sc.errors & KG_ERR_CHOLESKY),
           "MOCMAES: the covariance matrix of parent " + std::to_string(sc.failedParent) +
               " is not positive definite (non-positive Cholesky pivot)");
  return 0;
}

int kg_mocmaes_eval_builtin(kg_mocmaes_t h, int objective) {
  KG_CHECK(h, "kg_mocmaes_eval_builtin: null handle");
  KG_CHECK(h->initialized, "kg_mocmaes_eval_builtin: the handle holds no state");
  KG_CHECK(objective == KG_MOCMAES_OBJ_ROSENBROCK_SPHERE || objective == KG_MOCMAES_OBJ_ROSENBROCK_TWO_SPHERES,
           "unknown builtin multi-objective kernel");
  KG_CHECK(h->K == (objective == KG_MOCMAES_OBJ_ROSENBROCK_SPHERE ? 2 : 3),
           "the builtin objective's number of objectives differs from 'Num Objectives'");
  Stage st(h->times, h->stream, "evaluate");
  hipLaunchKernelGGL(k_mo_objective, dim3((h->P + MO_TPB - 1) / MO_TPB), dim3(MO_TPB), 0, h->stream, h->N, h->P, h->K,
                     (const double *)h->X[h->cur], h->V[h->cur], h->sc);
  KG_HIP(hipGetLastError());
  return 0;
}

int kg_mocmaes_get_candidates(kg_mocmaes_t h, double *X, size_t ld) {
  KG_CHECK(h, "kg_mocmaes_get_candidates: null handle");
  KG_CHECK(X, "kg_mocmaes_get_candidates: null output");
  KG_CHECK(ld == 0 || ld >= (size_t)h->N, "kg_mocmaes_get_candidates: ld is smaller than the variable count");
  const size_t N = h->N;
  if (ld == 0) ld = N;
  KG_HIP(hipMemcpy2DAsync(X, ld * sizeof(double), h->X[h->cur], N * sizeof(double), N * sizeof(double), h->P,
                          hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mocmaes_set_values(kg_mocmaes_t h, const double *V) {
  KG_CHECK(h, "kg_mocmaes_set_values: null handle");
  KG_CHECK(V, "kg_mocmaes_set_values: null values");
  // Optimization::evaluateMultiple (optimization.cpp.base:42-44)
  for (size_t e = 0; e < (size_t)h->P * h->K; e++)
    KG_CHECK(std::isfinite(V[e]), "Non finite value of function evaluation detected for sample " +
                                      std::to_string(e / h->K) + ", objective " + std::to_string(e % h->K));
  Stage st(h->times, h->stream, "evaluate");
  KG_HIP(hipMemcpyAsync(h->V[h->cur], V, (size_t)h->P * h->K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_mo_add_evals, dim3(1), dim3(1), 0, h->stream, h->sc, (double)h->P);
  KG_HIP(hipGetLastError());
  KG_HIP(hipStreamSynchronize(h->stream));  // V is the caller's
  return 0;
}

int kg_mocmaes_update(kg_mocmaes_t h, size_t generation) {
  KG_CHECK(h, "kg_mocmaes_update: null handle");
  KG_CHECK(h->initialized, "kg_mocmaes_update: the handle holds no state");
  (void)generation;
  const int c = h->cur, p = 1 - h->cur;
  {
    Stage st(h->times, h->stream, "sort");
    if (mo_sort(h)) return 1;
  }
  {
    Stage st(h->times, h->stream, "update");
    hipLaunchKernelGGL(k_mo_update, dim3(h->P), dim3(MO_TPB), 0, h->stream, h->c, (const int *)h->order,
                       (const double *)h->parentIdx, (const double *)h->X[c], (const double *)h->pX,
                       (const double *)h->pSg, (const double *)h->pC, (const double *)h->pPa, (const double *)h->pSr,
                       h->Sg[c], h->Cm[c], h->Pa[c], h->Sr[c]);
    KG_HIP(hipGetLastError());
  }
  {
    Stage st(h->times, h->stream, "parents");
    hipLaunchKernelGGL(k_mo_gather, dim3(2 * h->P), dim3(MO_TPB), 0, h->stream, h->c,
                       h->cfg.parent_order == KG_MOCMAES_PARENTS_RECORDED ? 1 : 0, (const int *)h->order,
                       (const double *)h->X[c], (const double *)h->X[p], (const double *)h->Sg[c],
                       (const double *)h->Sg[p], (const double *)h->Cm[c], (const double *)h->Cm[p],
                       (const double *)h->Pa[c], (const double *)h->Pa[p], (const double *)h->Sr[c],
                       (const double *)h->Sr[p], h->pX, h->pSg, h->pC, h->pPa, h->pSr);
    KG_HIP(hipGetLastError());
  }
  Stage st(h->times, h->stream, "statistics");
  return mo_statistics(h);
}

int kg_mocmaes_generation(kg_mocmaes_t h, size_t generation, int objective) {
  KG_CHECK(h, "kg_mocmaes_generation: null handle");
  if (kg_mocmaes_prepare(h, generation)) return 1;
  if (kg_mocmaes_eval_builtin(h, objective)) return 1;
  return kg_mocmaes_update(h, generation);
}

int kg_mocmaes_synchronize(kg_mocmaes_t h) {
  KG_CHECK(h, "kg_mocmaes_synchronize: null handle");
  KG_HIP(hipStreamSynchronize(h->stream));
  MoScalars o;
  StreamState s;
  KG_HIP(hipMemcpy(&o, h->sc, sizeof(o), hipMemcpyDeviceToHost));
  KG_CHECK(!(o.errors & KG_ERR_NONFINITE_F), "Non finite value of function evaluation detected");
  KG_CHECK(!(o.errors & KG_ERR_CHOLESKY), "MOCMAES: a parent's covariance matrix is not positive definite");
  for (MtStream *m : {&h->normal, &h->uniform}) {
    KG_HIP(hipMemcpy(&s, m->state(), sizeof(s), hipMemcpyDeviceToHost));
    KG_CHECK(!(s.errors & KG_ERR_RNG_UNDERRUN), "MOCMAES: a random stream was consumed past its generated words");
    KG_CHECK(s.errors == 0, "MOCMAES: random stream error");
  }
  return 0;
}

int kg_mocmaes_field_size(kg_mocmaes_t h, const char *name, size_t *n) {
  KG_CHECK(h, "kg_mocmaes_field_size: null handle");
  KG_CHECK(n, "kg_mocmaes_field_size: null output");
  MoField f;
  KG_CHECK(mo_field(h, name, f), std::string("unknown MOCMAES field: ") + (name ? name : "(null)"));
  *n = f.n;
  return 0;
}

int kg_mocmaes_get_field(kg_mocmaes_t h, const char *name, double *out, size_t n) {
  KG_CHECK(h, "kg_mocmaes_get_field: null handle");
  KG_CHECK(out || n == 0, "kg_mocmaes_get_field: null output");
  MoField f;
  KG_CHECK(mo_field(h, name, f), std::string("unknown MOCMAES field: ") + (name ? name : "(null)"));
  KG_CHECK(n == f.n, std::string("MOCMAES field size mismatch: ") + name);
  if (n) KG_HIP(hipMemcpyAsync(out, f.dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mocmaes_set_field(kg_mocmaes_t h, const char *name, const double *in, size_t n) {
  KG_CHECK(h, "kg_mocmaes_set_field: null handle");
  KG_CHECK(in || n == 0, "kg_mocmaes_set_field: null input");
  MoField f;
  KG_CHECK(mo_field(h, name, f), std::string("unknown MOCMAES field: ") + (name ? name : "(null)"));
  if (f.archive && std::string(name) == "Sample Collection") {
    // the archive's size comes with its rows; its values follow with the same row count
    KG_CHECK(n % (size_t)h->N == 0, "MOCMAES field size mismatch: Sample Collection");
    const size_t rows = n / (size_t)h->N;
    h->archiveCount = 0;  // (nothing to keep)
    if (mo_archive_reserve(h, rows + (size_t)h->P)) return 1;
    h->archiveCount = rows;
    const double cnt = (double)rows;
    KG_HIP(hipMemcpyAsync(&h->sc->archiveCount, &cnt, sizeof(double), hipMemcpyHostToDevice, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));
    mo_field(h, name, f);
  }
  KG_CHECK(n == f.n, std::string("MOCMAES field size mismatch: ") + name);
  if (n) KG_HIP(hipMemcpyAsync(f.dev, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->initialized = true;  // a restored state replaces setInitialConfiguration
  return 0;
}

int kg_mocmaes_get_rng(kg_mocmaes_t h, int which, void *state5000) {
  KG_CHECK(h, "kg_mocmaes_get_rng: null handle");
  KG_CHECK(state5000, "kg_mocmaes_get_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Multinormal) or 1 (Uniform)");
  return (which == 0 ? h->normal : h->uniform).export_gsl(state5000, h->stream);
}

int kg_mocmaes_set_rng(kg_mocmaes_t h, int which, const void *state5000) {
  KG_CHECK(h, "kg_mocmaes_set_rng: null handle");
  KG_CHECK(state5000, "kg_mocmaes_set_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Multinormal) or 1 (Uniform)");
  return (which == 0 ? h->normal : h->uniform).import_gsl(state5000, h->stream);
}

int kg_mocmaes_diagnostics(kg_mocmaes_t h, size_t *last_windows, size_t *window_blocks, size_t *archive_capacity,
                           size_t *last_rounds) {
  KG_CHECK(h, "kg_mocmaes_diagnostics: null handle");
  if (last_windows) *last_windows = h->windowsLast;
  if (window_blocks) *window_blocks = h->window;
  if (archive_capacity) *archive_capacity = h->archiveCap;
  if (last_rounds) *last_rounds = h->roundsLast;
  return 0;
}

int kg_mocmaes_profile(kg_mocmaes_t h, int enable) {
  KG_CHECK(h, "kg_mocmaes_profile: null handle");
  h->times.on = enable != 0;
  return 0;
}

int kg_mocmaes_profile_read(kg_mocmaes_t h, const char *stage, double *ms_total, size_t *count) {
  KG_CHECK(h, "kg_mocmaes_profile_read: null handle");
  KG_CHECK(ms_total && count, "kg_mocmaes_profile_read: null output");
  return h->times.read(h->stream, stage, ms_total, count);
}

}  // extern "C"
