// kg_dea.hip — differential evolution on the MI355X (DEA.cpp.base, see
// include/korali_amd.h for the per-entry-point reference map).
//
// HBM layout per handle (all FP64, sample-major as the reference's vectors):
//   X     P x N  "Sample Population"      cand  P x N  "Candidate Population"
//   F     P      "Value Vector"           Fprev P      "Previous Value Vector"
//   mean, prevMean, bestEverVars, currBestVars, maxDist   N
//   sc    scalar block (best values, rates, counters)
//   one MtStream: the Uniform Generator.  The Normal Generator is seeded and
//   exported but never drawn from (DEA.cpp.base draws uniforms only).
//
// The proposal is a chain (DEA.cpp.base:99-190): every draw comes from ONE
// sequential stream, a sample consumes a data-dependent number of words (the
// rejection loops for a, b, c; a whole re-mutation + N fixInfeasible draws
// per infeasible attempt; two to four more words per Self Adaptive attempt),
// and whether an attempt is the sample's last depends on the candidate it
// produced.  So the first word of sample i+1 is known only after sample i's
// last attempt has been evaluated.  k_dea_propose is that chain: ONE
// workgroup walks the samples in order; inside an attempt the index draws
// are uniform over the workgroup, the rows X[a], X[b], parent, X[i] are
// gathered with lanes over d (coalesced 8-byte loads), and feasibility is a
// workgroup AND.  No attempts are evaluated speculatively.
//
// Window protocol (no unbounded loop on the device): the kernel reads a
// window of W peeked uniforms.  An attempt either fits in what is left of
// the window and is completed, or the kernel stops BEFORE it and records
// (sample, retry flag, words used by the completed attempts).  The host
// consumes exactly those words, peeks the next window from there and
// relaunches.  A window too small for one attempt is doubled; a generation
// that needs more than `max_windows` windows is an error (the reference would
// loop forever on a configuration that cannot become feasible).
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

constexpr int DEA_TPB = 256;
constexpr int DEA_HEAD = 64;  // words of the window staged in LDS per attempt (the index draws)

struct DeaScalars {
  double bestEverValue, previousBestEverValue, currentBestValue, previousBestValue;
  double mutationRate, crossoverRate, currentMinimumStepSize;
  double bestSampleIndex, infeasibleSampleCount;
};

// where the chain stands between two launches of k_dea_propose
struct DeaChain {
  unsigned long long used;  // words of this window consumed by completed attempts
  int sample;               // the sample the next attempt belongs to
  int retry;                // that sample already had an infeasible attempt
  int done;                 // every sample has its feasible candidate
  int attempts;             // attempts completed by this launch
};

// initSamples (DEA.cpp.base:87-97): lower + width * u, one word per element
// in sample-major order; the product and the sum are two roundings
__global__ void __launch_bounds__(256) k_dea_init(int N, size_t tot, const double *__restrict__ lb,
                                                  const double *__restrict__ ub, const double *__restrict__ u,
                                                  double *__restrict__ X, double *__restrict__ cand) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= tot) return;
  const int d = (int)(e % (size_t)N);
  const double width = ub[d] - lb[d];
  const double wu = width * u[e];
  const double v = lb[d] + wu;
  cand[e] = v;
  X[e] = v;
}

// setInitialConfiguration's scalars (DEA.cpp.base:41-48); the two rates keep
// their configured values
__global__ void k_dea_init_scalars(DeaScalars *sc) {
  sc->infeasibleSampleCount = 0.0;
  sc->bestSampleIndex = 0.0;
  sc->previousBestValue = -INFINITY;
  sc->currentBestValue = -INFINITY;
  sc->previousBestEverValue = -INFINITY;
  sc->bestEverValue = -INFINITY;
  sc->currentMinimumStepSize = INFINITY;
}

// prepareGeneration for generations > 1 (DEA.cpp.base:99-190): the chain
// over samples, one workgroup.  Every thread follows the same control flow
// on the same words; lanes split only over d.
__global__ void __launch_bounds__(DEA_TPB) k_dea_propose(int N, int P, int parentBest, int selfAdaptive, int fix,
                                                         const double *__restrict__ X, double *__restrict__ cand,
                                                         const double *__restrict__ lb, const double *__restrict__ ub,
                                                         const double *__restrict__ u, unsigned long long W,
                                                         DeaScalars *sc, DeaChain *ch) {
  __shared__ double head[DEA_HEAD];
  const int tid = threadIdx.x;
  int i = ch->sample, retry = ch->retry;
  double F = sc->mutationRate, CR = sc->crossoverRate;
  int best = (int)sc->bestSampleIndex;
  if (best < 0 || best >= P) best = 0;  // (a restored state cannot index outside the population)
  const double Pd = (double)P, Nd = (double)N;
  unsigned long long o = 0;  // window offset of the next attempt
  double infeasible = 0.0;
  int attempts = 0;
  __syncthreads();
  // at most W attempts per launch: each one consumes at least one word
  while (i < P) {
    if (tid < DEA_HEAD) head[tid] = (o + tid < W) ? u[o + tid] : 0.0;
    __syncthreads();
    unsigned long long q = o;
    bool fits = true;  // false: the window ends inside this attempt
    auto word = [&](unsigned long long at) -> double { return at - o < DEA_HEAD ? head[at - o] : u[at]; };
    // mutateSingle's rejection loops (:121-128): (size_t)(u * P)
    int a = 0, b = 0, c = 0;
    for (;;) {
      if (q >= W) {
        fits = false;
        break;
      }
      a = (int)(unsigned long long)(word(q++) * Pd);
      if (a != i) break;
    }
    while (fits) {
      if (q >= W) {
        fits = false;
        break;
      }
      b = (int)(unsigned long long)(word(q++) * Pd);
      if (b != i && b != a) break;
    }
    // Self Adaptive (Brest 2006, :130-151): rd2 and rd3 always, rd1 / rd4 on demand
    double Fn = F, CRn = CR;
    if (fits && selfAdaptive) {
      if (q + 2 > W) {
        fits = false;
      } else {
        const double rd2 = word(q++);
        const double rd3 = word(q++);
        if (rd2 < 0.1) {
          if (q >= W) {
            fits = false;
          } else {
            const double t = word(q++) * 0.9;
            Fn = 0.1 + t;
          }
        }
        if (fits && rd3 < 0.1) {
          if (q >= W)
            fits = false;
          else
            CRn = word(q++);
        }
      }
    }
    // the parent (:153-166): "Best" draws no c
    int par = best;
    if (!parentBest) {
      while (fits) {
        if (q >= W) {
          fits = false;
          break;
        }
        c = (int)(unsigned long long)(word(q++) * Pd);
        if (c != i && c != a && c != b) break;
      }
      par = c;
    }
    // rn, N crossover words, and N fixInfeasible words on a retry (:168-189)
    const bool fixing = fix && retry;
    const unsigned long long need = 1ULL + (unsigned long long)N + (fixing ? (unsigned long long)N : 0ULL);
    if (fits && q + need > W) fits = false;
    if (!fits) break;  // (uniform) the attempt starts the next window
    const int rn = (int)(unsigned long long)(word(q++) * Nd);
    bool ok = true;
    const size_t ri = (size_t)i * N, ra = (size_t)a * N, rb = (size_t)b * N, rp = (size_t)par * N;
    for (int d = tid; d < N; d += DEA_TPB) {
      const double xi = X[ri + d], xa = X[ra + d], xb = X[rb + d], xp = X[rp + d];
      const double lo = lb[d], hi = ub[d];
      const double uc = u[q + d];
      const double diff = xa - xb;
      const double step = Fn * diff;
      const double mut = xp + step;
      double v = (uc < CRn || d == rn) ? mut : xi;
      if (fixing) {
        // fixInfeasible (:178-190): always one word per component
        double len = 0.0;
        if (v < lo) len = v - lo;
        if (v > hi) len = v - hi;
        const double back = len * u[q + N + d];
        v = xi - back;
      }
      cand[ri + d] = v;
      // Optimizer::isSampleFeasible (optimizer.cpp.base:5-14)
      if (!isfinite(v) || v < lo || v > hi) ok = false;
    }
    q += need - 1ULL;
    const int feasible = __syncthreads_and(ok ? 1 : 0);
    F = Fn;
    CR = CRn;
    o = q;
    attempts++;
    if (feasible) {
      i++;
      retry = 0;
    } else {
      infeasible += 1.0;  // :112
      retry = 1;
    }
  }
  if (tid == 0) {
    ch->used = o;
    ch->sample = i;
    ch->retry = retry;
    ch->done = i >= P ? 1 : 0;
    ch->attempts = attempts;
    sc->mutationRate = F;
    sc->crossoverRate = CR;
    sc->infeasibleSampleCount += infeasible;
  }
}

// updateSolver up to the accept decisions (DEA.cpp.base:198-256), one
// workgroup: the first index of the maximum (std::max_element), the shifted
// best values, the best variables, and accept[i] for the configured rule.
__global__ void __launch_bounds__(DEA_TPB) k_dea_select(int N, int P, int rule, const double *__restrict__ F,
                                                        const double *__restrict__ Fprev,
                                                        const double *__restrict__ cand, double *__restrict__ mean,
                                                        double *__restrict__ prevMean,
                                                        double *__restrict__ bestEverVars,
                                                        double *__restrict__ currBestVars, int *__restrict__ accept,
                                                        DeaScalars *sc) {
  __shared__ double rv[DEA_TPB];
  __shared__ int ri[DEA_TPB];
  __shared__ double cmax[DEA_TPB];
  const int tid = threadIdx.x;
  // first maximum: contiguous chunks, ties keep the lower index
  const int chunk = (P + DEA_TPB - 1) / DEA_TPB, i0 = tid * chunk, i1 = min(P, i0 + chunk);
  double bv = -INFINITY, run = -INFINITY;
  int bi = -1;
  for (int i = i0; i < i1; i++) {
    const double v = F[i];
    if (bi < 0 || bv < v) {
      bv = v;
      bi = i;
    }
    if (v > run) run = v;
  }
  rv[tid] = bv;
  ri[tid] = bi;
  cmax[tid] = run;
  __syncthreads();
  for (int s = DEA_TPB / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const int oi = ri[tid + s];
      const double ov = rv[tid + s];
      // the other half holds higher indices: it wins only when strictly larger
      if (oi >= 0 && (ri[tid] < 0 || rv[tid] < ov)) {
        rv[tid] = ov;
        ri[tid] = oi;
      }
    }
    __syncthreads();
  }
  const int best = ri[0];
  const double currentBest = rv[0];
  const double bestEverOld = sc->bestEverValue;
  const double currentBestOld = sc->currentBestValue;
  const bool improved = currentBest > bestEverOld;
  __syncthreads();
  if (tid == 0) {
    sc->bestSampleIndex = (double)best;
    sc->previousBestEverValue = bestEverOld;  // :199
    sc->previousBestValue = currentBestOld;   // :200
    sc->currentBestValue = currentBest;       // :201
    // every rule leaves max(best ever, current best): Best / Greedy /
    // Improved assign it when the current best improves (:214-242), and
    // Iterative's running maximum (:246-255) ends there as well
    if (improved) sc->bestEverValue = currentBest;
    // :276-277: the reference resets the step size to +Inf and then discards
    // the result of std::min, so "Current Minimum Step Size" stays +Inf
    sc->currentMinimumStepSize = INFINITY;
  }
  for (int d = tid; d < N; d += DEA_TPB) {
    const double x = cand[(size_t)best * N + d];
    currBestVars[d] = x;                 // :203
    prevMean[d] = mean[d];               // :205
    if (improved) bestEverVars[d] = x;   // :208, before the accept rule
  }
  if (rule == KG_DEA_ACCEPT_ITERATIVE) {
    // accept i when F[i] exceeds the running maximum of (best ever, F[0..i-1]):
    // a prefix maximum, chunk maxima first
    double pre = bestEverOld;
    for (int t = 0; t < tid; t++) {
      const double m = cmax[t];
      if (m > pre) pre = m;
    }
    for (int i = i0; i < i1; i++) {
      const double v = F[i];
      const int acc = v > pre ? 1 : 0;
      if (acc) pre = v;
      accept[i] = acc;
    }
    return;
  }
  // Best, Greedy and Improved in one straight-line body (the rule is uniform):
  // both thresholds are read, the rule selects
  for (int i = tid; i < P; i += DEA_TPB) {
    const double f = F[i];
    const double prev = Fprev[i];
    // Greedy (:222-232) compares with the previous generation's candidate
    // value, Improved (:234-244) with the best-ever value from before
    const double threshold = rule == KG_DEA_ACCEPT_GREEDY ? prev : bestEverOld;
    int acc = f > threshold ? 1 : 0;
    if (rule == KG_DEA_ACCEPT_BEST) acc = (i == best && improved) ? 1 : 0;  // :212-220
    accept[i] = acc;
  }
}

__global__ void __launch_bounds__(256) k_dea_apply(int N, size_t tot, const int *__restrict__ accept,
                                                   const double *__restrict__ cand, double *__restrict__ X) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= tot) return;
  if (accept[e / (size_t)N]) X[e] = cand[e];
}

// Current Mean (:58-60, :260-262): mean[d] += X[i][d] / (double)P in order
// over i, a true division per element; Max Distances (:264-274).  One lane
// per d, rows read coalesced.
__global__ void __launch_bounds__(64) k_dea_stats(int N, int P, int distances, const double *__restrict__ X,
                                                  double *__restrict__ mean, double *__restrict__ maxDist) {
  const int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= N) return;
  const double Pd = (double)P;
  mean[d] = ordered_sum(0.0, P, [&](int i) { return X[(size_t)i * N + d] / Pd; });
  if (!distances) return;
  double mx = -INFINITY, mn = INFINITY;
  for (int i = 0; i < P; i++) {
    const double x = X[(size_t)i * N + d];
    if (x > mx) mx = x;
    if (x < mn) mn = x;
  }
  maxDist[d] = mx - mn;
}

}  // namespace kg

using namespace kg;

struct kg_dea_s {
  kg_dea_cfg cfg;
  int N = 0, P = 0;
  hipStream_t stream = nullptr;
  double *X = nullptr, *cand = nullptr, *F = nullptr, *Fprev = nullptr;
  double *mean = nullptr, *prevMean = nullptr, *bestEverVars = nullptr, *currBestVars = nullptr, *maxDist = nullptr;
  double *lb = nullptr, *ub = nullptr, *ubuf = nullptr;
  int *accept = nullptr;
  DeaScalars *sc = nullptr;
  DeaChain *chain = nullptr;
  CmaesScalars *osc = nullptr;  // the objective kernels' block: evaluation count and error flags
  size_t window = 0, ucap = 0, maxWindows = 0;
  size_t windowsLast = 0;  // windows the last kg_dea_prepare used
  bool initialized = false;
  MtStream uniform;
  unsigned char normalState[5000];  // the Normal Generator: seeded, saved, never drawn from
  StageTimes times;
};

namespace {

struct DeaField {
  void *dev = nullptr;
  size_t n = 0;
};

bool dea_field(kg_dea_s *h, const char *name, DeaField &f) {
  const std::string k = name ? name : "";
  const size_t N = h->N, P = h->P;
  auto vec = [&](double *p, size_t n) {
    f.dev = p;
    f.n = n;
    return true;
  };
  if (k == "Sample Population") return vec(h->X, P * N);
  if (k == "Candidate Population") return vec(h->cand, P * N);
  if (k == "Value Vector") return vec(h->F, P);
  if (k == "Previous Value Vector") return vec(h->Fprev, P);
  if (k == "Current Mean") return vec(h->mean, N);
  if (k == "Previous Mean") return vec(h->prevMean, N);
  if (k == "Best Ever Variables") return vec(h->bestEverVars, N);
  if (k == "Current Best Variables") return vec(h->currBestVars, N);
  if (k == "Max Distances") return vec(h->maxDist, N);
  if (k == "Best Ever Value") return vec(&h->sc->bestEverValue, 1);
  if (k == "Previous Best Ever Value") return vec(&h->sc->previousBestEverValue, 1);
  if (k == "Current Best Value") return vec(&h->sc->currentBestValue, 1);
  if (k == "Previous Best Value") return vec(&h->sc->previousBestValue, 1);
  if (k == "Mutation Rate") return vec(&h->sc->mutationRate, 1);
  if (k == "Crossover Rate") return vec(&h->sc->crossoverRate, 1);
  if (k == "Current Minimum Step Size") return vec(&h->sc->currentMinimumStepSize, 1);
  if (k == "Best Sample Index") return vec(&h->sc->bestSampleIndex, 1);
  if (k == "Infeasible Sample Count") return vec(&h->sc->infeasibleSampleCount, 1);
  if (k == "Model Evaluation Count") return vec(&h->osc->modelEvaluationCount, 1);
  return false;
}

int dea_stats(kg_dea_s *h, int distances) {
  hipLaunchKernelGGL(k_dea_stats, dim3((h->N + 63) / 64), dim3(64), 0, h->stream, h->N, h->P, distances, h->X,
                     h->mean, h->maxDist);
  KG_HIP(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" {

int kg_dea_create(const kg_dea_cfg *cfg, kg_dea_t *out) {
  KG_CHECK(cfg && out, "kg_dea_create: null argument");
  KG_CHECK(cfg->variable_count >= 1, "'Variable Count' must be >= 1");
  KG_CHECK(cfg->variable_count < (1u << 24) && cfg->population_size < (1u << 24), "DEA: shape too large");
  KG_CHECK(cfg->lower_bound && cfg->upper_bound, "DEA needs the variables' 'Lower Bound' and 'Upper Bound'");
  KG_CHECK(cfg->parent_rule == KG_DEA_PARENT_RANDOM || cfg->parent_rule == KG_DEA_PARENT_BEST,
           "unknown DEA 'Parent Selection Rule'");
  KG_CHECK(cfg->mutation_rule == KG_DEA_MUTATION_FIXED || cfg->mutation_rule == KG_DEA_MUTATION_SELF_ADAPTIVE,
           "unknown DEA 'Mutation Rule'");
  KG_CHECK(cfg->accept_rule >= KG_DEA_ACCEPT_BEST && cfg->accept_rule <= KG_DEA_ACCEPT_IMPROVED,
           "unknown DEA 'Accept Rule'");
  // mutateSingle's rejection loops (DEA.cpp.base:121-128, :157-160) draw
  // distinct indices other than the sample's own: with fewer they never end
  const size_t need = cfg->parent_rule == KG_DEA_PARENT_RANDOM ? 4 : 3;
  KG_CHECK(cfg->population_size >= need,
           "DEA 'Population Size' must be at least 4 with Parent Selection Rule 'Random' and 3 with 'Best' "
           "(the mutation draws that many distinct samples).");
  for (size_t d = 0; d < cfg->variable_count; d++) {
    KG_CHECK(std::isfinite(cfg->lower_bound[d]) && std::isfinite(cfg->upper_bound[d]),
             "DEA needs finite 'Lower Bound' and 'Upper Bound' for every variable");
    KG_CHECK(!(cfg->upper_bound[d] < cfg->lower_bound[d]), "Lower Bound exceeds Upper Bound.");  // DEA.cpp.base:19-21
  }
  KG_HIP(hipSetDevice(cfg->device));
  auto *h = new kg_dea_s();
  h->cfg = *cfg;
  h->cfg.lower_bound = h->cfg.upper_bound = nullptr;
  const size_t N = cfg->variable_count, P = cfg->population_size;
  h->N = (int)N;
  h->P = (int)P;
  // an attempt needs at most 2N + 5 words plus its rejected index draws; the
  // default window holds a few attempts per sample
  const size_t minWindow = 16;
  h->window = cfg->window_words ? std::max<size_t>(cfg->window_words, minWindow) : std::max<size_t>(4096, 4 * P * (N + 8));
  h->maxWindows = cfg->max_windows ? cfg->max_windows : 1024;
  h->ucap = std::max(h->window, P * N);
  auto fail = [&]() {
    kg_dea_destroy(h);
    return 1;
  };
  if (stream_acquire(&h->stream) != hipSuccess) {
    set_error("kg_dea_create: no stream");
    return fail();
  }
  if (dalloc(&h->X, P * N) || dalloc(&h->cand, P * N) || dalloc(&h->F, P) || dalloc(&h->Fprev, P) ||
      dalloc(&h->mean, N) || dalloc(&h->prevMean, N) || dalloc(&h->bestEverVars, N) || dalloc(&h->currBestVars, N) ||
      dalloc(&h->maxDist, N) || dalloc(&h->lb, N) || dalloc(&h->ub, N) || dalloc(&h->ubuf, h->ucap) ||
      dalloc(&h->accept, P) || dalloc(&h->sc, 1) || dalloc(&h->chain, 1) || dalloc(&h->osc, 1))
    return fail();
  if (hipMemcpy(h->lb, cfg->lower_bound, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->ub, cfg->upper_bound, N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_dea_create: bounds upload failed");
    return fail();
  }
  DeaScalars sc{};
  sc.bestEverValue = sc.previousBestEverValue = -INFINITY;  // DEA.config Module Defaults
  sc.mutationRate = cfg->mutation_rate;
  sc.crossoverRate = cfg->crossover_rate;
  if (hipMemcpy(h->sc, &sc, sizeof(sc), hipMemcpyHostToDevice) != hipSuccess) {
    set_error("kg_dea_create: scalar upload failed");
    return fail();
  }
  if (N <= 128 && allow_dynamic_lds((const void *)k_objective2, ob2_lds_bytes((int)N)) != hipSuccess) {
    set_error("kg_dea_create: objective kernel LDS");
    return fail();
  }
  // the ring holds the largest window the chain may grow to (4 x the default)
  if (h->uniform.init(8 * h->ucap + 16384)) return fail();
  unsigned char st[5000];
  gsl_seed_state(cfg->uniform_seed, st);
  if (h->uniform.import_gsl(st, h->stream)) return fail();
  gsl_seed_state(cfg->normal_seed, h->normalState);
  *out = h;
  return 0;
}

int kg_dea_destroy(kg_dea_t h) {
  if (!h) return 0;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->uniform.drain();
  for (void *p : {(void *)h->X, (void *)h->cand, (void *)h->F, (void *)h->Fprev, (void *)h->mean, (void *)h->prevMean,
                  (void *)h->bestEverVars, (void *)h->currBestVars, (void *)h->maxDist, (void *)h->lb, (void *)h->ub,
                  (void *)h->ubuf, (void *)h->accept, (void *)h->sc, (void *)h->chain, (void *)h->osc})
    if (p) dev_release(p);
  h->times.release();
  if (h->stream) stream_release(h->stream);
  delete h;
  return 0;
}

int kg_dea_initialize(kg_dea_t h) {
  KG_CHECK(h, "kg_dea_initialize: null handle");
  const size_t N = h->N, P = h->P, tot = P * N;
  {
    Stage st(h->times, h->stream, "words");
    if (h->uniform.uniforms(h->ubuf, tot, h->stream)) return 1;
  }
  Stage st(h->times, h->stream, "propose");
  hipLaunchKernelGGL(k_dea_init, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->N, tot, h->lb, h->ub,
                     h->ubuf, h->X, h->cand);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_fill, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, h->stream, h->F, P, -INFINITY);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_dea_init_scalars, dim3(1), dim3(1), 0, h->stream, h->sc);
  KG_HIP(hipGetLastError());
  for (double *p : {h->prevMean, h->bestEverVars, h->currBestVars, h->maxDist})
    KG_HIP(hipMemsetAsync(p, 0, N * sizeof(double), h->stream));
  KG_HIP(hipMemsetAsync(h->Fprev, 0, P * sizeof(double), h->stream));
  if (dea_stats(h, 0)) return 1;
  h->initialized = true;
  return 0;
}

int kg_dea_prepare(kg_dea_t h, size_t generation) {
  KG_CHECK(h, "kg_dea_prepare: null handle");
  KG_CHECK(generation >= 1, "kg_dea_prepare: generations count from 1");
  KG_CHECK(h->initialized, "kg_dea_prepare: the handle holds no population (kg_dea_initialize, or a restored state, first)");
  const size_t P = h->P;
  h->windowsLast = 0;
  if (generation > 1) {
    KG_HIP(hipMemsetAsync(h->chain, 0, sizeof(DeaChain), h->stream));
    for (size_t w = 0;; w++) {
      if (w >= h->maxWindows) {
        DeaChain c{};
        KG_HIP(hipMemcpyAsync(&c, h->chain, sizeof(c), hipMemcpyDeviceToHost, h->stream));
        KG_HIP(hipStreamSynchronize(h->stream));
        set_error("DEA: sample " + std::to_string(c.sample) + " of generation " + std::to_string(generation) +
                  " has no feasible candidate after " + std::to_string(w) + " windows of " +
                  std::to_string(h->window) +
                  " uniform draws: the configuration cannot become feasible and the reference would redraw forever");
        return 1;
      }
      {
        Stage st(h->times, h->stream, "words");
        if (h->uniform.peek_uniforms(h->ubuf, h->window, h->stream)) return 1;
      }
      {
        Stage st(h->times, h->stream, "propose");
        hipLaunchKernelGGL(k_dea_propose, dim3(1), dim3(DEA_TPB), 0, h->stream, h->N, h->P,
                           h->cfg.parent_rule == KG_DEA_PARENT_BEST ? 1 : 0,
                           h->cfg.mutation_rule == KG_DEA_MUTATION_SELF_ADAPTIVE ? 1 : 0, h->cfg.fix_infeasible ? 1 : 0,
                           (const double *)h->X, h->cand, (const double *)h->lb, (const double *)h->ub,
                           (const double *)h->ubuf, (unsigned long long)h->window, h->sc, h->chain);
        KG_HIP(hipGetLastError());
        if (h->uniform.consume_words_dev(&h->chain->used, h->stream)) return 1;
      }
      h->windowsLast++;
      DeaChain c{};
      KG_HIP(hipMemcpyAsync(&c, h->chain, sizeof(c), hipMemcpyDeviceToHost, h->stream));
      KG_HIP(hipStreamSynchronize(h->stream));
      if (c.done) break;
      if (c.attempts == 0) {
        // the window does not hold one whole attempt: double it
        const size_t cap = 2 * h->window;
        KG_CHECK(2 * cap + 8192 <= h->uniform.capacity_words(),
                 "DEA: one proposal attempt needs more uniform draws than the device window can hold");
        if (cap > h->ucap) {
          double *nb = nullptr;
          if (dalloc(&nb, cap)) return 1;
          dev_release(h->ubuf, h->stream);
          h->ubuf = nb;
          h->ucap = cap;
        }
        h->window = cap;
      }
    }
  }
  // _previousValueVector = _valueVector (:115), at generation 1 as well
  KG_HIP(hipMemcpyAsync(h->Fprev, h->F, P * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  return 0;
}

int kg_dea_eval_builtin(kg_dea_t h, int objective) {
  KG_CHECK(h, "kg_dea_eval_builtin: null handle");
  KG_CHECK(objective >= 0 && objective <= 2, "unknown builtin objective");
  Stage st(h->times, h->stream, "evaluate");
  if (h->N <= 128)
    hipLaunchKernelGGL(k_objective2, dim3((h->P + OB2_R - 1) / OB2_R), dim3(256), ob2_lds_bytes(h->N), h->stream, h->N,
                       h->P, objective, (const double *)h->cand, h->F, h->osc, (double)h->P);
  else
    hipLaunchKernelGGL(k_objective, dim3((h->P + OB_C - 1) / OB_C), dim3(256), 0, h->stream, h->N, h->P, objective,
                       (const double *)h->cand, h->F, h->osc, (double)h->P);
  KG_HIP(hipGetLastError());
  return 0;
}

int kg_dea_get_candidates(kg_dea_t h, double *X, size_t ld) {
  KG_CHECK(h, "kg_dea_get_candidates: null handle");
  KG_CHECK(X, "kg_dea_get_candidates: null output");
  KG_CHECK(ld == 0 || ld >= (size_t)h->N, "kg_dea_get_candidates: ld is smaller than the variable count");
  const size_t N = h->N;
  if (ld == 0) ld = N;
  KG_HIP(hipMemcpy2DAsync(X, ld * sizeof(double), h->cand, N * sizeof(double), N * sizeof(double), h->P,
                          hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_dea_set_fitness(kg_dea_t h, const double *F) {
  KG_CHECK(h, "kg_dea_set_fitness: null handle");
  KG_CHECK(F, "kg_dea_set_fitness: null fitness vector");
  // Optimization::evaluate (optimization.cpp.base:32-33)
  for (int i = 0; i < h->P; i++)
    KG_CHECK(std::isfinite(F[i]), "Non finite value of function evaluation detected for sample " + std::to_string(i));
  Stage st(h->times, h->stream, "evaluate");
  KG_HIP(hipMemcpyAsync(h->F, F, h->P * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // KORALI_START of every sample (DEA.cpp.base:77); kg_cmaes.hip's kernel on the same CmaesScalars
  hipLaunchKernelGGL(k_add_evals, dim3(1), dim3(1), 0, h->stream, h->osc, (double)h->P);
  KG_HIP(hipGetLastError());
  KG_HIP(hipStreamSynchronize(h->stream));  // F is the caller's
  return 0;
}

int kg_dea_update(kg_dea_t h, size_t generation) {
  KG_CHECK(h, "kg_dea_update: null handle");
  KG_CHECK(h->initialized, "kg_dea_update: the handle holds no population");
  (void)generation;
  Stage st(h->times, h->stream, "update");
  const size_t tot = (size_t)h->P * h->N;
  hipLaunchKernelGGL(k_dea_select, dim3(1), dim3(DEA_TPB), 0, h->stream, h->N, h->P, h->cfg.accept_rule,
                     (const double *)h->F, (const double *)h->Fprev, (const double *)h->cand, h->mean, h->prevMean,
                     h->bestEverVars, h->currBestVars, h->accept, h->sc);
  KG_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_dea_apply, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, h->stream, h->N, tot,
                     (const int *)h->accept, (const double *)h->cand, h->X);
  KG_HIP(hipGetLastError());
  return dea_stats(h, 1);
}

int kg_dea_generation(kg_dea_t h, size_t generation, int objective) {
  KG_CHECK(h, "kg_dea_generation: null handle");
  if (generation == 1 && !h->initialized && kg_dea_initialize(h)) return 1;
  if (kg_dea_prepare(h, generation)) return 1;
  if (kg_dea_eval_builtin(h, objective)) return 1;
  return kg_dea_update(h, generation);
}

int kg_dea_synchronize(kg_dea_t h) {
  KG_CHECK(h, "kg_dea_synchronize: null handle");
  KG_HIP(hipStreamSynchronize(h->stream));
  CmaesScalars o;
  StreamState s;
  KG_HIP(hipMemcpy(&o, h->osc, sizeof(o), hipMemcpyDeviceToHost));
  KG_HIP(hipMemcpy(&s, h->uniform.state(), sizeof(s), hipMemcpyDeviceToHost));
  KG_CHECK(!(o.errors & KG_ERR_NONFINITE_F), "Non finite value of function evaluation detected");
  KG_CHECK(!(s.errors & KG_ERR_RNG_UNDERRUN), "DEA: the uniform stream was consumed past its generated words");
  KG_CHECK(s.errors == 0, "DEA: uniform stream error");
  return 0;
}

int kg_dea_field_size(kg_dea_t h, const char *name, size_t *n) {
  KG_CHECK(h, "kg_dea_field_size: null handle");
  KG_CHECK(n, "kg_dea_field_size: null output");
  DeaField f;
  KG_CHECK(dea_field(h, name, f), std::string("unknown DEA field: ") + (name ? name : "(null)"));
  *n = f.n;
  return 0;
}

int kg_dea_get_field(kg_dea_t h, const char *name, double *out, size_t n) {
  KG_CHECK(h, "kg_dea_get_field: null handle");
  KG_CHECK(out, "kg_dea_get_field: null output");
  DeaField f;
  KG_CHECK(dea_field(h, name, f), std::string("unknown DEA field: ") + (name ? name : "(null)"));
  KG_CHECK(n == f.n, std::string("DEA field size mismatch: ") + name);
  KG_HIP(hipMemcpyAsync(out, f.dev, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  return 0;
}

int kg_dea_set_field(kg_dea_t h, const char *name, const double *in, size_t n) {
  KG_CHECK(h, "kg_dea_set_field: null handle");
  KG_CHECK(in, "kg_dea_set_field: null input");
  DeaField f;
  KG_CHECK(dea_field(h, name, f), std::string("unknown DEA field: ") + (name ? name : "(null)"));
  KG_CHECK(n == f.n, std::string("DEA field size mismatch: ") + name);
  KG_HIP(hipMemcpyAsync(f.dev, in, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  KG_HIP(hipStreamSynchronize(h->stream));
  h->initialized = true;  // a restored state replaces setInitialConfiguration
  return 0;
}

int kg_dea_get_rng(kg_dea_t h, int which, void *state5000) {
  KG_CHECK(h, "kg_dea_get_rng: null handle");
  KG_CHECK(state5000, "kg_dea_get_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  if (which == 0) {
    memcpy(state5000, h->normalState, 5000);
    return 0;
  }
  return h->uniform.export_gsl(state5000, h->stream);
}

int kg_dea_set_rng(kg_dea_t h, int which, const void *state5000) {
  KG_CHECK(h, "kg_dea_set_rng: null handle");
  KG_CHECK(state5000, "kg_dea_set_rng: null state");
  KG_CHECK(which == 0 || which == 1, "rng index must be 0 (Normal) or 1 (Uniform)");
  if (which == 0) {
    memcpy(h->normalState, state5000, 5000);
    return 0;
  }
  return h->uniform.import_gsl(state5000, h->stream);
}

int kg_dea_windows(kg_dea_t h, size_t *last_windows, size_t *window_words) {
  KG_CHECK(h, "kg_dea_windows: null handle");
  if (last_windows) *last_windows = h->windowsLast;
  if (window_words) *window_words = h->window;
  return 0;
}

int kg_dea_profile(kg_dea_t h, int enable) {
  KG_CHECK(h, "kg_dea_profile: null handle");
  h->times.on = enable != 0;
  return 0;
}

int kg_dea_profile_read(kg_dea_t h, const char *stage, double *ms_total, size_t *count) {
  KG_CHECK(h, "kg_dea_profile_read: null handle");
  KG_CHECK(ms_total && count, "kg_dea_profile_read: null output");
  return h->times.read(h->stream, stage, ms_total, count);
}

}  // extern "C"
