// kg_mcmc.hip — Metropolis-Hastings with delayed rejection and adaptive
// sampling on the MI355X (MCMC.cpp.base; see include/korali_amd.h for the
// per-entry-point reference map and DESIGN.md §24).
//
// HBM per handle (FP64, row-major as the reference's vectors):
//   leader N, mean N, cand R x N, candEval R           "Chain Leader", "Chain Mean", "Chain Candidate", ...
//   Linit, Lchain, cov, placeholder  N x N             the two factors, "Chain Covariance" and its placeholder
//   sc[]   the scalars (counts as doubles)             db maxSamples x N, dbEval maxSamples
//   z      W x N^2  the window's normals               u  W  the window's uniforms
//   two MtStreams: the Normal and the Uniform Generator.
//
// A Markov chain is serial: generation g + 1 starts from what g accepted.
// k_mcmc_chain is therefore ONE workgroup that walks many generations per
// launch over a window of stream the host side produced beforehand: candidate
// c of a window is normals [c N^2, (c + 1) N^2), and the k-th uniform drawn is
// uniform k.  The chain starts a generation only if the window still holds
// the worst case it may need (R candidates, R uniforms); otherwise it stops
// before it.  The streams are then advanced by exactly what was consumed and
// the next launch sees fresh windows, so neither the window size nor how the
// caller cuts a run into calls changes a bit of the result.
//
// Inside a generation every stage is workgroup-parallel with uniform control
// flow (the accept and level decisions travel through LDS): N lanes own one
// row's ordered add chain each, one lane evaluates logP and alpha, the
// placeholder and covariance update run one thread per entry, the Cholesky is
// block_cholesky_gsl, the database append is by N lanes.  The two factors and
// the covariance stay in LDS for the whole launch.
#include <algorithm>
#include <cmath>
#include <cstdio>
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

constexpr int MC_TPB = 256;
constexpr int MC_MAXN = 64;
constexpr int MC_MAXR = 8;
constexpr int MC_T = MC_MAXR + 1;  // entries of the path (leader, candidate 0, ..., candidate R - 1)
constexpr size_t MC_MAX_DB = (size_t)1 << 27;

// the scalars of MCMC.config's Internal Settings, counts as doubles
enum McScalar {
  MC_ACCEPT = 0,   // "Acceptance Count"
  MC_PROPOSED,     // "Proposed Sample Count"
  MC_LENGTH,       // "Chain Length"
  MC_EVALS,        // "Model Evaluation Count"
  MC_CHOL_FAIL,    // "Cholesky Failures"
  MC_RATE,         // "Acceptance Rate"
  MC_LEADER_EVAL,  // "Chain Leader Evaluation"
  MC_DB_ROWS,      // rows of the "Sample Database"
  MC_NSC
};

struct McCfg {
  int N, R, adaptive, kernel, priors;
  double burnIn, nap, scaling;
  unsigned long long leap, maxSamples;
};

// recursiveAlpha's values for the current generation: the path is y[0] = the
// leader's evaluation, y[j + 1] = candidate j's.  Every call of the recursion
// is the alpha of a contiguous sub-path walked up or down; the upward ones
// (a -> b, a < b) are reused by later levels, the downward ones (from the
// newest entry) are not.
struct McAlpha {
  double y[MC_T], E[MC_T];                 // E[j] = exp(y[j])
  double fa[MC_T * MC_T], fd[MC_T * MC_T];  // alpha and denominator of (a -> b), a < b
  double ra[MC_T], rd[MC_T];               // ... of (newest -> a)
};

// where the chain's state is while a kernel runs: LDS in k_mcmc_chain, HBM
// in the stepping kernels
struct McView {
  double *Linit, *Lchain, *cov, *scr;  // N rows, S doubles apart; scr: normals of a proposal, Cholesky workspace
  int S;
  double *leader, *mean, *cand, *candEval, *sc;
  McAlpha *al;
  int *bc;  // [0] accepted, [1] uniforms drawn: the decision every thread reads
};

// what a launch hands the host
struct McRun {
  unsigned long long usedBlocks;  // candidates (blocks of N^2 normals) consumed from the window
  unsigned long long usedWords;   // uniforms consumed
  unsigned long long generations; // completed
  int windowEnd;                  // stopped for lack of stream
  int stoppedBy;                  // enum kg_mcmc_stop
  int accepted;
  unsigned int errors;
};

struct McPriors {
  const int *kind;
  const double *a, *b, *cst;
};

__global__ void k_mcmc_prior_const(int N, const double *__restrict__ a, const double *__restrict__ b,
                                   const int *__restrict__ kind, double *__restrict__ cst) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d < N) cst[d] = prior_const(kind[d], a[d], b[d]);
}

// std::min(1.0, x): a NaN gives 1.0
__device__ __forceinline__ double mc_min1(double x) { return (x < 1.0) ? x : 1.0; }

// alpha of level n (:134-168), y[0 .. n + 1] given; one lane
__device__ __forceinline__ double mc_alpha(McAlpha *t, int n, int R) {
  const int top = n + 1;
  if (R == 1) return mc_min1(exp_cr(t->y[1] - t->y[0]));
  if (n == 0) t->E[0] = exp_cr(t->y[0]);
  t->E[top] = exp_cr(t->y[top]);
  for (int a = n; a >= 1; a--) {  // (top -> a)
    if (a == n) {
      t->rd[a] = t->E[top];
      t->ra[a] = mc_min1(exp_cr(t->y[a] - t->y[top]));
    } else {
      double num = t->E[a];
      for (int b = a + 1; b <= n; b++) num *= (1.0 - t->fa[a * MC_T + b]);
      const double den = t->rd[a + 1] * (1.0 - t->ra[a + 1]);
      t->rd[a] = den;
      t->ra[a] = (num == 0.0) ? 0.0 : mc_min1(num / den);
    }
  }
  for (int a = n; a >= 0; a--) {  // (a -> top)
    if (a == n) {
      t->fd[a * MC_T + top] = t->E[a];
      t->fa[a * MC_T + top] = mc_min1(exp_cr(t->y[top] - t->y[a]));
    } else {
      double num = t->E[top];
      for (int b = n; b >= a + 1; b--) num *= (1.0 - t->ra[b]);
      const double den = t->fd[a * MC_T + top - 1] * (1.0 - t->fa[a * MC_T + top - 1]);
      t->fd[a * MC_T + top] = den;
      t->fa[a * MC_T + top] = (num == 0.0) ? 0.0 : mc_min1(num / den);
    }
  }
  return t->fa[top];
}

// generateCandidate (:170-185); zblk: the candidate's N^2 normals
__device__ __forceinline__ void mc_propose(const McCfg &c, const McView &v, int level,
                                           const double *__restrict__ zblk) {
  const int tid = threadIdx.x, N = c.N, S = v.S;
  const bool chain = c.adaptive && v.sc[MC_DB_ROWS] > c.nap + c.burnIn;  // :179
  const double *L = chain ? v.Lchain : v.Linit;
  for (int e = tid; e < N * N; e += MC_TPB) v.scr[(e / N) * S + e % N] = zblk[e];
  __syncthreads();
  if (tid < N) {
    double x = level == 0 ? v.leader[tid] : v.cand[(level - 1) * N + tid];
    for (int e = 0; e < N; e++) {
      const double p = L[tid * S + e] * v.scr[tid * S + e];
      x += p;
    }
    v.cand[level * N + tid] = x;
  }
  if (tid == 0) v.sc[MC_PROPOSED] += 1.0;
  __syncthreads();
}

// the evaluation and :76-90; u: the next uniform of the window.  hostLogp is
// read with KG_MCMC_HOST only.  On return bc[] holds the decision.
__device__ __forceinline__ void mc_decide(const McCfg &c, const McView &v, const McPriors &pr, int level,
                                          double hostLogp, const double *__restrict__ u) {
  const int tid = threadIdx.x, N = c.N;
  if (tid == 0) {
    const double *x = v.cand + level * N;
    double lp = 0.0;
    if (c.priors)
      for (int d = 0; d < N; d++) lp += prior_logdens(pr.kind[d], x[d], pr.a[d], pr.b[d], pr.cst[d]);
    double ev;
    if (c.priors && lp == -INFINITY) {
      ev = -INFINITY;  // no model evaluation behind a -inf prior
    } else {
      double ll = hostLogp;
      if (c.kernel == KG_MCMC_GAUSSIAN) {
        double ss = 0.0;
        for (int d = 0; d < N; d++) ss += x[d] * x[d];
        ll = -0.5 * ss;
      }
      ev = c.priors ? lp + ll : ll;
    }
    v.sc[MC_EVALS] += 1.0;
    v.candEval[level] = ev;
    if (level == 0) v.al->y[0] = v.sc[MC_LEADER_EVAL];
    v.al->y[level + 1] = ev;
    const double alpha = mc_alpha(v.al, level, c.R);
    int acc = alpha == 1.0, drawn = 0;
    if (!acc) {  // :84: no uniform is drawn behind alpha == 1.0
      drawn = 1;
      acc = alpha > u[0];
    }
    if (acc) {
      v.sc[MC_ACCEPT] += 1.0;
      v.sc[MC_LEADER_EVAL] = ev;
    }
    v.bc[0] = acc;
    v.bc[1] = drawn;
  }
  __syncthreads();
  if (v.bc[0] && tid < N) v.leader[tid] = v.cand[level * N + tid];
  __syncthreads();
}

// :93-100: the database push, updateState (:187-219), _chainLength++
__device__ __forceinline__ void mc_end_generation(const McCfg &c, const McView &v, unsigned long long generation,
                                                  double *__restrict__ placeholder, double *__restrict__ db,
                                                  double *__restrict__ dbEval) {
  const int tid = threadIdx.x, N = c.N, S = v.S;
  const double rows0 = v.sc[MC_DB_ROWS];
  const bool push = v.sc[MC_LENGTH] >= c.burnIn && generation % c.leap == 0 && rows0 < (double)c.maxSamples;
  const double n = push ? rows0 + 1.0 : rows0;
  __syncthreads();  // every thread has read the row count
  if (push) {
    const size_t r = (size_t)rows0;
    if (tid < N) db[r * N + tid] = v.leader[tid];
    if (tid == 0) {
      dbEval[r] = v.sc[MC_LEADER_EVAL];
      v.sc[MC_DB_ROWS] = n;
    }
  }
  if (tid == 0) v.sc[MC_RATE] = v.sc[MC_ACCEPT] / v.sc[MC_LENGTH];  // :189, the length before its increment
  if (n == 1.0) {
    if (tid < N) v.mean[tid] = v.leader[tid];
  } else if (n >= 2.0) {
    const double f = (n - 2.0) / (n - 1.0), s = c.scaling / n;
    for (int e = tid; e < N * N; e += MC_TPB) {
      const int d = e / N, k = e % N;
      if (k > d) continue;
      const double p = (v.mean[d] - v.leader[d]) * (v.mean[k] - v.leader[k]);  // :201-204, from the old mean
      placeholder[d * N + k] = p;
      const double fc = f * v.cov[d * S + k], sp = s * p;
      const double lower = fc + sp;  // :212, :216
      v.cov[d * S + k] = lower;
      if (k < d) {
        placeholder[k * N + d] = p;
        const double fl = f * lower;  // :213 reads the element :212 just wrote
        v.cov[k * S + d] = fl + sp;
      }
    }
    __syncthreads();
    if (tid < N) {  // :207
      const double t = v.mean[tid] * (n - 1.0);
      v.mean[tid] = (t + v.leader[tid]) / n;
    }
    if (c.adaptive && n > c.nap) {  // :218, choleskyDecomp :103-132
      for (int e = tid; e < N * N; e += MC_TPB) {
        const int d = e / N, k = e % N;
        if (k <= d) v.scr[d * S + k] = v.cov[d * S + k];
      }
      __syncthreads();
      const bool failed = block_cholesky_gsl(v.scr, N, S);
      if (failed) {
        if (tid == 0) v.sc[MC_CHOL_FAIL] += 1.0;  // the reference warns; the old factor stays
      } else {
        for (int e = tid; e < N * N; e += MC_TPB) {
          const int d = e / N, k = e % N;
          if (k <= d) v.Lchain[d * S + k] = v.scr[d * S + k];
        }
      }
    }
  }
  if (tid == 0) v.sc[MC_LENGTH] += 1.0;
  __syncthreads();
}

// `count` generations from `first`, or as many as the windows (W candidates:
// z W x N^2, u W) allow
__global__ void __launch_bounds__(MC_TPB) k_mcmc_chain(McCfg c, McPriors pr, unsigned long long first,
                                                       unsigned long long count, double maxEvals,
                                                       unsigned long long W, const double *__restrict__ z,
                                                       const double *__restrict__ u, double *gLeader, double *gMean,
                                                       double *gCand, double *gCandEval, double *gLinit,
                                                       double *gLchain, double *gCov, double *gPlaceholder,
                                                       double *gSc, double *db, double *dbEval, McRun *run) {
  extern __shared__ double mats[];  // Linit, Lchain, cov, scr: N x S each
  __shared__ double sLeader[MC_MAXN], sMean[MC_MAXN], sCand[MC_MAXR * MC_MAXN], sCandEval[MC_MAXR], sSc[MC_NSC];
  __shared__ McAlpha sAl;
  __shared__ int sBc[2];
  const int tid = threadIdx.x, N = c.N, R = c.R, S = N | 1;  // an odd row distance: the lanes' rows in distinct banks
  McView v;
  v.S = S;
  v.Linit = mats;
  v.Lchain = mats + (size_t)N * S;
  v.cov = mats + 2 * (size_t)N * S;
  v.scr = mats + 3 * (size_t)N * S;
  v.leader = sLeader;
  v.mean = sMean;
  v.cand = sCand;
  v.candEval = sCandEval;
  v.sc = sSc;
  v.al = &sAl;
  v.bc = sBc;
  for (int e = tid; e < N * N; e += MC_TPB) {
    const int o = (e / N) * S + e % N;
    v.Linit[o] = gLinit[e];
    v.Lchain[o] = gLchain[e];
    v.cov[o] = gCov[e];
  }
  for (int e = tid; e < R * N; e += MC_TPB) sCand[e] = gCand[e];
  if (tid < N) {
    sLeader[tid] = gLeader[tid];
    sMean[tid] = gMean[tid];
  }
  if (tid < R) sCandEval[tid] = gCandEval[tid];
  if (tid < MC_NSC) sSc[tid] = gSc[tid];
  __syncthreads();
  unsigned long long nb = 0, nu = 0, done = 0;
  int windowEnd = 0, stoppedBy = 0;
  for (unsigned long long i = 0; i < count; i++) {
    if (sSc[MC_DB_ROWS] >= (double)c.maxSamples) {
      stoppedBy |= KG_MCMC_MAX_SAMPLES;
      break;
    }
    if (W - nb < (unsigned long long)R || W - nu < (unsigned long long)R) {
      windowEnd = 1;
      break;
    }
    int accepted = 0;
    for (int level = 0; level < R && !accepted; level++) {
      mc_propose(c, v, level, z + nb * (unsigned long long)(N * N));
      nb++;
      mc_decide(c, v, pr, level, 0.0, u + nu);
      accepted = sBc[0];
      nu += (unsigned long long)sBc[1];
      __syncthreads();  // the decision is read before the next level overwrites it
    }
    mc_end_generation(c, v, first + i, gPlaceholder, db, dbEval);
    done++;
    if (maxEvals > 0.0 && sSc[MC_EVALS] >= maxEvals) {
      stoppedBy |= KG_MCMC_MAX_MODEL_EVALUATIONS;
      break;
    }
  }
  if (sSc[MC_DB_ROWS] >= (double)c.maxSamples) stoppedBy |= KG_MCMC_MAX_SAMPLES;
  __syncthreads();
  for (int e = tid; e < N * N; e += MC_TPB) {
    const int o = (e / N) * S + e % N;
    gLchain[e] = v.Lchain[o];
    gCov[e] = v.cov[o];
  }
  for (int e = tid; e < R * N; e += MC_TPB) gCand[e] = sCand[e];
  if (tid < N) {
    gLeader[tid] = sLeader[tid];
    gMean[tid] = sMean[tid];
  }
  if (tid < R) gCandEval[tid] = sCandEval[tid];
  if (tid < MC_NSC) gSc[tid] = sSc[tid];
  if (tid == 0) {
    run->usedBlocks = nb;
    run->usedWords = nu;
    run->generations = done;
    run->windowEnd = windowEnd;
    run->stoppedBy = stoppedBy;
    run->accepted = 0;
  }
}

// the stepping kernels: the same device code on the state in HBM
__device__ __forceinline__ McView mc_hbm_view(int N, double *leader, double *mean, double *cand, double *candEval,
                                              double *Linit, double *Lchain, double *cov, double *scr, double *sc,
                                              McAlpha *al, int *bc) {
  McView v;
  v.S = N;
  v.Linit = Linit;
  v.Lchain = Lchain;
  v.cov = cov;
  v.scr = scr;
  v.leader = leader;
  v.mean = mean;
  v.cand = cand;
  v.candEval = candEval;
  v.sc = sc;
  v.al = al;
  v.bc = bc;
  return v;
}

__global__ void __launch_bounds__(MC_TPB) k_mcmc_propose(McCfg c, int level, const double *__restrict__ z,
                                                         double *leader, double *cand, double *Linit, double *Lchain,
                                                         double *scr, double *sc) {
  const McView v = mc_hbm_view(c.N, leader, nullptr, cand, nullptr, Linit, Lchain, nullptr, scr, sc, nullptr, nullptr);
  mc_propose(c, v, level, z);
}

__global__ void __launch_bounds__(MC_TPB) k_mcmc_decide(McCfg c, McPriors pr, int level, double logp,
                                                        const double *__restrict__ u, double *leader, double *cand,
                                                        double *candEval, double *sc, McAlpha *al, McRun *run) {
  __shared__ int sBc[2];
  const McView v = mc_hbm_view(c.N, leader, nullptr, cand, candEval, nullptr, nullptr, nullptr, nullptr, sc, al, sBc);
  mc_decide(c, v, pr, level, logp, u);
  if (threadIdx.x == 0) {
    run->accepted = sBc[0];
    run->usedWords = (unsigned long long)sBc[1];
  }
}

__global__ void __launch_bounds__(MC_TPB) k_mcmc_end(McCfg c, unsigned long long generation, double *leader,
                                                     double *mean, double *Lchain, double *cov, double *scr,
                                                     double *placeholder, double *sc, double *db, double *dbEval) {
  const McView v = mc_hbm_view(c.N, leader, mean, nullptr, nullptr, nullptr, Lchain, cov, scr, sc, nullptr, nullptr);
  mc_end_generation(c, v, generation, placeholder, db, dbEval);
}

}  // namespace kg

using namespace kg;

struct kg_mcmc_s {
  kg_mcmc_cfg cfg;
  McCfg c;
  int N = 0, R = 0;
  hipStream_t stream = nullptr;
  double *leader = nullptr, *mean = nullptr, *cand = nullptr, *candEval = nullptr, *Linit = nullptr, *Lchain = nullptr,
         *cov = nullptr, *placeholder = nullptr, *scr = nullptr, *sc = nullptr, *db = nullptr, *dbEval = nullptr;
  double *pmin = nullptr, *pmax = nullptr, *cst = nullptr;
  int *kind = nullptr;
  double *z = nullptr, *u = nullptr;
  unsigned long long *blockEnd = nullptr;
  McAlpha *al = nullptr;
  McRun *run = nullptr;
  size_t window = 0;  // candidates per window
  size_t windowsLast = 0, relaunchesLast = 0;
  int nextLevel = 0;      // the level kg_mcmc_propose expects
  bool proposed = false;  // ... and whether its candidate waits for kg_mcmc_decide
  MtStream normal, uniform;
  StageTimes times;
};

namespace {

McPriors mc_priors(kg_mcmc_s *h) { return McPriors{h->kind, h->pmin, h->pmax, h->cst}; }

size_t mc_lds_bytes(int N) { return 4 * (size_t)N * (size_t)(N | 1) * sizeof(double); }

struct McField {
  double *dev = nullptr;
  size_t n = 0;
  int scalar = -1;  // index into sc
  int database = 0; // 1: "Sample Database", 2: "Sample Evaluation Database"
};

int mc_db_rows(kg_mcmc_s *h, size_t *rows) {
  double r = 0;
  KG_HIP(hipMemcpyAsync(&r, h->sc + MC_DB_ROWS, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  *rows = (size_t)r;
  return 0;
}

bool mc_field(kg_mcmc_s *h, const char *name, McField &f) {
  const std::string k = name ? name : "";
  const size_t N = h->N, R = h->R;
  auto dev = [&](double *p, size_t n) {
    f.dev = p;
    f.n = n;
    return true;
  };
  auto scalar = [&](int i) {
    f.dev = h->sc + i;
    f.n = 1;
    f.scalar = i;
    return true;
  };
  if (k == "Chain Leader") return dev(h->leader, N);
  if (k == "Chain Leader Evaluation") return scalar(MC_LEADER_EVAL);
  if (k == "Chain Candidate") return dev(h->cand, R * N);
  if (k == "Chain Candidates Evaluations") return dev(h->candEval, R);
  if (k == "Cholesky Decomposition Covariance") return dev(h->Linit, N * N);
  if (k == "Cholesky Decomposition Chain Covariance") return dev(h->Lchain, N * N);
  if (k == "Chain Mean") return dev(h->mean, N);
  if (k == "Chain Covariance") return dev(h->cov, N * N);
  if (k == "Chain Covariance Placeholder") return dev(h->placeholder, N * N);
  if (k == "Acceptance Rate") return scalar(MC_RATE);
  if (k == "Acceptance Count") return scalar(MC_ACCEPT);
  if (k == "Proposed Sample Count") return scalar(MC_PROPOSED);
  if (k == "Chain Length") return scalar(MC_LENGTH);
  if (k == "Model Evaluation Count") return scalar(MC_EVALS);
  if (k == "Cholesky Failures") return scalar(MC_CHOL_FAIL);
  if (k == "Sample Database") {
    f.dev = h->db;
    f.database = 1;
    return true;
  }
  if (k == "Sample Evaluation Database") {
    f.dev = h->dbEval;
    f.database = 2;
    return true;
  }
  return false;
}

// the windows of one launch: W candidates' normals with their block ends, W uniforms
int mc_fill_windows(kg_mcmc_s *h, size_t W) {
  Stage st(h->times, h->stream, "window");
  const size_t NN = (size_t)h->N * h->N;
  if (h->normal.polar_normals(h->z, W * NN, NN, h->blockEnd, h->stream)) return 1;
  if (h->uniform.peek_uniforms(h->u, W, h->stream)) return 1;
  return 0;
}

}  // namespace

extern "C" {

int kg_mcmc_create(const kg_mcmc_cfg *cfg, kg_mcmc_t *out) {
  KG_CHECK(cfg && out, "kg_mcmc_create: null argument");
  char buf[160];
  // MCMC.cpp.base:23-27
  if (cfg->chain_covariance_scaling <= 0.0) {
    snprintf(buf, sizeof buf, "Chain Covariance Scaling must be larger 0.0 (is %lf).\n", cfg->chain_covariance_scaling);
    set_error(buf);
    return 1;
  }
  if (cfg->leap < 1) {
    snprintf(buf, sizeof buf, "Leap must be larger 0 (is %zu).\n", (size_t)cfg->leap);
    set_error(buf);
    return 1;
  }
  if (cfg->burn_in < 0) {
    snprintf(buf, sizeof buf, "Burn In must be larger equal 0 (is %zu).\n", (size_t)cfg->burn_in);
    set_error(buf);
    return 1;
  }
  if (cfg->rejection_levels < 1) {
    snprintf(buf, sizeof buf, "Rejection Levels must be larger 0 (is %zu).\n", (size_t)cfg->rejection_levels);
    set_error(buf);
    return 1;
  }
  if (cfg->non_adaption_period < 0) {
    snprintf(buf, sizeof buf, "Non Adaption Period must be larger equal 0 (is %zu).\n", (size_t)cfg->non_adaption_period);
    set_error(buf);
    return 1;
  }
  KG_CHECK(cfg->variable_count >= 1, "MCMC: 'Variable Count' must be >= 1");
  KG_CHECK(cfg->variable_count <= (size_t)MC_MAXN, "MCMC: more than 64 variables are not supported on the device");
  KG_CHECK(cfg->rejection_levels <= MC_MAXR,
           "MCMC: more than 8 'Rejection Levels' are not supported on the device (the reference's recursion grows "
           "about 2.6x per level)");
  KG_CHECK(cfg->max_samples >= 1, "MCMC: 'Max Samples' must be at least 1");
  KG_CHECK(cfg->max_samples <= MC_MAX_DB / cfg->variable_count,
           "MCMC: 'Max Samples' x 'Variable Count' exceeds the database's capacity on the device (2^27 values)");
  KG_CHECK(cfg->initial_mean && cfg->initial_sdev,
           "MCMC needs the 'Initial Mean' and 'Initial Standard Deviation' of every variable");
  KG_CHECK(cfg->probability_kernel == KG_MCMC_HOST || cfg->probability_kernel == KG_MCMC_GAUSSIAN,
           "unknown builtin probability kernel");
  KG_CHECK(!cfg->prior_kind || (cfg->prior_min && cfg->prior_max), "MCMC needs the parameters of every variable's prior");
  const size_t N = cfg->variable_count, R = (size_t)cfg->rejection_levels, NN = N * N;
  for (size_t d = 0; cfg->prior_kind && d < N; d++)
    KG_CHECK(cfg->prior_kind[d] >= KG_PRIOR_UNIFORM && cfg->prior_kind[d] <= KG_PRIOR_LOGNORMAL,
             "prior_kind entries must be KG_PRIOR_UNIFORM .. KG_PRIOR_LOGNORMAL");
  KG_HIP(hipSetDevice(cfg->device));
  upload_dd_tables();  // log_cr of the polar normals and the priors, exp_cr of alpha
  auto *h = new kg_mcmc_s();
  h->cfg = *cfg;
  h->cfg.initial_mean = h->cfg.initial_sdev = h->cfg.prior_min = h->cfg.prior_max = nullptr;
  h->cfg.prior_kind = nullptr;
  h->N = (int)N;
  h->R = (int)R;
  h->c.N = (int)N;
  h->c.R = (int)R;
  h->c.adaptive = cfg->use_adaptive_sampling ? 1 : 0;
  h->c.kernel = cfg->probability_kernel;
  h->c.priors = cfg->prior_kind ? 1 : 0;
  h->c.burnIn = (double)cfg->burn_in;
  h->c.nap = (double)cfg->non_adaption_period;
  h->c.scaling = cfg->chain_covariance_scaling;
  h->c.leap = (unsigned long long)cfg->leap;
  h->c.maxSamples = cfg->max_samples;
  // a window holds about 2^20 normals, at least one generation's worst case, at most 65536 candidates
  const size_t w0 = cfg->window_candidates ? cfg->window_candidates : std::min<size_t>(65536, ((size_t)1 << 20) / NN);
  h->window = std::max(w0, R);
  const size_t W = h->window, rows = cfg->max_samples;
  auto fail = [&]() {
    kg_mcmc_destroy(h);
    return 1;
  };
  if (stream_acquire(&h->stream) != hipSuccess) {
    set_error("kg_mcmc_create: no stream");
    return fail();
  }
  if (dalloc(&h->leader, N) || dalloc(&h->mean, N) || dalloc(&h->cand, R * N) || dalloc(&h->candEval, R) ||
      dalloc(&h->Linit, NN) || dalloc(&h->Lchain, NN) || dalloc(&h->cov, NN) || dalloc(&h->placeholder, NN) ||
      dalloc(&h->scr, NN) || dalloc(&h->sc, MC_NSC) || dalloc(&h->db, rows * N) || dalloc(&h->dbEval, rows) ||
      dalloc(&h->pmin, N) || dalloc(&h->pmax, N) || dalloc(&h->cst, N) || dalloc(&h->kind, N) ||
      dalloc(&h->z, W * NN) || dalloc(&h->u, W) || dalloc(&h->blockEnd, W) || dalloc(&h->al, 1) ||
      dalloc(&h->run, 1))
    return fail();
  // setInitialConfiguration (:42-53)
  std::vector<double> L0(NN, 0.0), sc(MC_NSC, 0.0);
  for (size_t d = 0; d < N; d++) L0[d * N + d] = cfg->initial_sdev[d];
  sc[MC_LEADER_EVAL] = -INFINITY;
  sc[MC_RATE] = 1.0;
  if (hipMemcpy(h->leader, cfg->initial_mean, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->Linit, L0.data(), NN * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->sc, sc.data(), MC_NSC * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_mcmc_create: upload failed");
    return fail();
  }
  if (cfg->prior_kind) {
    if (hipMemcpy(h->pmin, cfg->prior_min, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->pmax, cfg->prior_max, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(h->kind, cfg->prior_kind, N * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("kg_mcmc_create: upload failed");
      return fail();
    }
    hipLaunchKernelGGL(k_mcmc_prior_const, dim3(1), dim3(MC_MAXN), 0, h->stream, h->N, (const double *)h->pmin,
                       (const double *)h->pmax, (const int *)h->kind, h->cst);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
      set_error("kg_mcmc_create: prior constants");
      return fail();
    }
  }
  if (allow_dynamic_lds((const void *)k_mcmc_chain, mc_lds_bytes(h->N)) != hipSuccess) {
    set_error("kg_mcmc_create: kernel LDS");
    return fail();
  }
  if (h->normal.init(4 * h->normal.words_for_normals(W * NN) + 16384)) return fail();
  if (h->uniform.init(4 * W + 16384)) return fail();
  unsigned char st[5000];
  gsl_seed_state(cfg->normal_seed, st);
  if (h->normal.import_gsl(st, h->stream)) return fail();
  gsl_seed_state(cfg->uniform_seed, st);
  if (h->uniform.import_gsl(st, h->stream)) return fail();
  *out = h;
  return 0;
}

int kg_mcmc_destroy(kg_mcmc_t h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->normal.drain();
  h->uniform.drain();
  for (void *p : {(void *)h->leader, (void *)h->mean, (void *)h->cand, (void *)h->candEval, (void *)h->Linit,
                  (void *)h->Lchain, (void *)h->cov, (void *)h->placeholder, (void *)h->scr, (void *)h->sc,
                  (void *)h->db, (void *)h->dbEval, (void *)h->pmin, (void *)h->pmax, (void *)h->cst, (void *)h->kind,
                  (void *)h->z, (void *)h->u, (void *)h->blockEnd, (void *)h->al, (void *)h->run})
    if (p) dev_release(p);
  h->times.release();
  if (h->stream) stream_release(h->stream);
  delete h;
  return 0;
}

int kg_mcmc_run(kg_mcmc_t h, size_t first_generation, size_t count, size_t max_model_evaluations, size_t *done,
                int *stopped_by) {
  KG_CHECK(h, "kg_mcmc_run: null handle");
  KG_CHECK(h->cfg.probability_kernel == KG_MCMC_GAUSSIAN, "kg_mcmc_run: the handle has no builtin probability kernel");
  KG_CHECK(first_generation >= 1, "kg_mcmc_run: generations count from 1");
  KG_CHECK(!h->proposed && h->nextLevel == 0, "kg_mcmc_run: a generation of the stepping entry points is open");
  const size_t R = h->R;
  size_t total = 0;
  int stopped = 0;
  h->windowsLast = h->relaunchesLast = 0;
  while (total < count) {
    const size_t remaining = count - total;
    const size_t W = remaining < h->window / R ? remaining * R : h->window;
    if (mc_fill_windows(h, W)) return 1;
    {
      Stage st(h->times, h->stream, "chain");
      hipLaunchKernelGGL(k_mcmc_chain, dim3(1), dim3(MC_TPB), mc_lds_bytes(h->N), h->stream, h->c, mc_priors(h),
                         (unsigned long long)(first_generation + total), (unsigned long long)remaining,
                         (double)max_model_evaluations, (unsigned long long)W, (const double *)h->z,
                         (const double *)h->u, h->leader, h->mean, h->cand, h->candEval, h->Linit, h->Lchain, h->cov,
                         h->placeholder, h->sc, h->db, h->dbEval, h->run);
      KG_HIP(hipGetLastError());
    }
    McRun r{};
    {
      Stage st(h->times, h->stream, "consume");
      if (h->normal.consume_normals_dev(&h->run->usedBlocks, (size_t)h->N * h->N, h->blockEnd, h->stream)) return 1;
      if (h->uniform.consume_words_dev(&h->run->usedWords, h->stream)) return 1;
      KG_HIP(hipMemcpyAsync(&r, h->run, sizeof(r), hipMemcpyDeviceToHost, h->stream));
    }
    KG_HIP(hipStreamSynchronize(h->stream));
    h->windowsLast++;
    total += r.generations;
    stopped = r.stoppedBy;
    if (!r.windowEnd) break;
    KG_CHECK(r.generations > 0, "MCMC: a stream window did not hold one generation (internal)");
    h->relaunchesLast++;
  }
  if (count == 0) {
    size_t rows = 0;
    if (mc_db_rows(h, &rows)) return 1;
    if (rows >= h->cfg.max_samples) stopped |= KG_MCMC_MAX_SAMPLES;
  }
  if (done) *done = total;
  if (stopped_by) *stopped_by = stopped;
  return 0;
}

int kg_mcmc_propose(kg_mcmc_t h, size_t level) {
  KG_CHECK(h, "kg_mcmc_propose: null handle");
  KG_CHECK(level < (size_t)h->R, "kg_mcmc_propose: level is not below 'Rejection Levels'");
  KG_CHECK(!h->proposed && level == (size_t)h->nextLevel,
           "kg_mcmc_propose: levels follow one another from 0, each decided before the next");
  const size_t NN = (size_t)h->N * h->N;
  if (mc_fill_windows(h, 1)) return 1;
  hipLaunchKernelGGL(k_mcmc_propose, dim3(1), dim3(MC_TPB), 0, h->stream, h->c, (int)level, (const double *)h->z,
                     h->leader, h->cand, h->Linit, h->Lchain, h->scr, h->sc);
  KG_HIP(hipGetLastError());
  if (h->normal.consume_normals(NN, NN, h->blockEnd, h->stream)) return 1;
  h->proposed = true;
  return 0;
}

int kg_mcmc_get_candidate(kg_mcmc_t h, double *x) {
  KG_CHECK(h, "kg_mcmc_get_candidate: null handle");
  KG_CHECK(x, "kg_mcmc_get_candidate: null output");
  KG_CHECK(h->proposed, "kg_mcmc_get_candidate: nothing proposed");
  KG_HIP(hipMemcpyAsync(x, h->cand + (size_t)h->nextLevel * h->N, h->N * sizeof(double), hipMemcpyDeviceToHost,
                        h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mcmc_decide(kg_mcmc_t h, size_t level, double logp, int *accepted) {
  KG_CHECK(h, "kg_mcmc_decide: null handle");
  KG_CHECK(h->proposed && level == (size_t)h->nextLevel, "kg_mcmc_decide: this level has no proposed candidate");
  KG_CHECK(h->cfg.probability_kernel != KG_MCMC_HOST || !std::isnan(logp),
           "Sample " + std::to_string(level) + " returned NaN logP(x) evaluation.\n");
  hipLaunchKernelGGL(k_mcmc_decide, dim3(1), dim3(MC_TPB), 0, h->stream, h->c, mc_priors(h), (int)level, logp,
                     (const double *)h->u, h->leader, h->cand, h->candEval, h->sc, h->al, h->run);
  KG_HIP(hipGetLastError());
  if (h->uniform.consume_words_dev(&h->run->usedWords, h->stream)) return 1;
  McRun r{};
  KG_HIP(hipMemcpyAsync(&r, h->run, sizeof(r), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->proposed = false;
  h->nextLevel = (r.accepted || level + 1 == (size_t)h->R) ? -1 : (int)level + 1;  // -1: end_generation next
  if (accepted) *accepted = r.accepted;
  return 0;
}

int kg_mcmc_end_generation(kg_mcmc_t h, size_t generation) {
  KG_CHECK(h, "kg_mcmc_end_generation: null handle");
  KG_CHECK(generation >= 1, "kg_mcmc_end_generation: generations count from 1");
  KG_CHECK(h->nextLevel == -1, "kg_mcmc_end_generation: the generation's levels are not decided yet");
  hipLaunchKernelGGL(k_mcmc_end, dim3(1), dim3(MC_TPB), 0, h->stream, h->c, (unsigned long long)generation, h->leader,
                     h->mean, h->Lchain, h->cov, h->scr, h->placeholder, h->sc, h->db, h->dbEval);
  KG_HIP(hipGetLastError());
  h->nextLevel = 0;
  return 0;
}

int kg_mcmc_database(kg_mcmc_t h, double *X, double *logp, size_t *rows) {
  KG_CHECK(h, "kg_mcmc_database: null handle");
  KG_CHECK(rows, "kg_mcmc_database: null row count");
  size_t n = 0;
  if (mc_db_rows(h, &n)) return 1;
  const size_t cap = *rows;
  *rows = n;
  if (!X && !logp) return 0;
  KG_CHECK(cap >= n, "kg_mcmc_database: the output holds fewer rows than the database");
  if (X && n) KG_HIP(hipMemcpyAsync(X, h->db, n * h->N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (logp && n) KG_HIP(hipMemcpyAsync(logp, h->dbEval, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mcmc_synchronize(kg_mcmc_t h) {
  KG_CHECK(h, "kg_mcmc_synchronize: null handle");
  KG_HIP(hipStreamSynchronize(h->stream));
  StreamState s;
  for (MtStream *m : {&h->normal, &h->uniform}) {
    KG_HIP(hipMemcpy(&s, m->state(), sizeof(s), hipMemcpyDeviceToHost));
    KG_CHECK(!(s.errors & KG_ERR_RNG_UNDERRUN), "MCMC: a random stream was consumed past its generated words");
    KG_CHECK(s.errors == 0, "MCMC: random stream error");
  }
  return 0;
}

int kg_mcmc_field_size(kg_mcmc_t h, const char *name, size_t *n) {
  KG_CHECK(h, "kg_mcmc_field_size: null handle");
  KG_CHECK(n, "kg_mcmc_field_size: null output");
  McField f;
  KG_CHECK(mc_field(h, name, f), std::string("unknown MCMC field: ") + (name ? name : "(null)"));
  if (f.database) {
    size_t rows = 0;
    if (mc_db_rows(h, &rows)) return 1;
    f.n = f.database == 1 ? rows * h->N : rows;
  }
  *n = f.n;
  return 0;
}

int kg_mcmc_get_field(kg_mcmc_t h, const char *name, double *out, size_t n) {
  KG_CHECK(h, "kg_mcmc_get_field: null handle");
  KG_CHECK(out || n == 0, "kg_mcmc_get_field: null output");
  McField f;
  KG_CHECK(mc_field(h, name, f), std::string("unknown MCMC field: ") + (name ? name : "(null)"));
  if (f.database) {
    size_t rows = 0;
    if (mc_db_rows(h, &rows)) return 1;
    f.n = f.database == 1 ? rows * h->N : rows;
  }
  KG_CHECK(n == f.n, std::string("MCMC field size mismatch: ") + name);
  if (n == 0) return 0;
  KG_HIP(hipMemcpyAsync(out, f.dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mcmc_set_field(kg_mcmc_t h, const char *name, const double *in, size_t n) {
  KG_CHECK(h, "kg_mcmc_set_field: null handle");
  KG_CHECK(in || n == 0, "kg_mcmc_set_field: null input");
  McField f;
  KG_CHECK(mc_field(h, name, f), std::string("unknown MCMC field: ") + (name ? name : "(null)"));
  if (f.database == 1) {
    KG_CHECK(n % (size_t)h->N == 0 && n / (size_t)h->N <= h->cfg.max_samples, "MCMC field size mismatch: Sample Database");
    const double rows = (double)(n / (size_t)h->N);
    KG_HIP(hipMemcpyAsync(h->sc + MC_DB_ROWS, &rows, sizeof(double), hipMemcpyHostToDevice, h->stream));
    KG_HIP(hipStreamSynchronize(h->stream));  // rows is a local
    f.n = n;
  } else if (f.database == 2) {
    size_t rows = 0;
    if (mc_db_rows(h, &rows)) return 1;
    f.n = rows;
  }
  KG_CHECK(n == f.n, std::string("MCMC field size mismatch: ") + name);
  if (n == 0) return 0;
  KG_HIP(hipMemcpyAsync(f.dev, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_mcmc_get_rng(kg_mcmc_t h, int which, void *state5000) {
  KG_CHECK(h, "kg_mcmc_get_rng: null handle");
  KG_CHECK(state5000, "kg_mcmc_get_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  return (which == 0 ? h->normal : h->uniform).export_gsl(state5000, h->stream);
}

int kg_mcmc_set_rng(kg_mcmc_t h, int which, const void *state5000) {
  KG_CHECK(h, "kg_mcmc_set_rng: null handle");
  KG_CHECK(state5000, "kg_mcmc_set_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  return (which == 0 ? h->normal : h->uniform).import_gsl(state5000, h->stream);
}

int kg_mcmc_diagnostics(kg_mcmc_t h, size_t *last_windows, size_t *last_relaunches, size_t *window_candidates) {
  KG_CHECK(h, "kg_mcmc_diagnostics: null handle");
  if (last_windows) *last_windows = h->windowsLast;
  if (last_relaunches) *last_relaunches = h->relaunchesLast;
  if (window_candidates) *window_candidates = h->window;
  return 0;
}

int kg_mcmc_profile(kg_mcmc_t h, int enable) {
  KG_CHECK(h, "kg_mcmc_profile: null handle");
  h->times.on = enable != 0;
  return 0;
}

int kg_mcmc_profile_read(kg_mcmc_t h, const char *stage, double *ms_total, size_t *count) {
  KG_CHECK(h, "kg_mcmc_profile_read: null handle");
  KG_CHECK(ms_total && count, "kg_mcmc_profile_read: null output");
  return h->times.read(h->stream, stage, ms_total, count);
}

}  // extern "C"
