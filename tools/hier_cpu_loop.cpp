// One-core CPU loop of the Hierarchical/Psi log-likelihood with libm, as the
// reference computes it (Psi::evaluateLogLikelihood + logSumExp: one
// getLogDensity call per term, a vector of K values per group, two passes),
// at the shape tools/time_hier.py times on the device; and of Hierarchical/
// Theta's two sums (Theta::initialize's denominators, one evaluateLogLikelihood
// per candidate without the sub-problem's model).
//   g++ -O2 -o tools/hier_cpu_loop tools/hier_cpu_loop.cpp && tools/hier_cpu_loop [P] [G] [K] [repeats]
//   tools/hier_cpu_loop theta [P] [M] [K] [repeats]
#include <cstring>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

struct Normal {
  double mean, sd, logNorm;
  void update() { logNorm = -0.5 * std::log(2 * M_PI) - std::log(sd); }
  double logDensity(double x) const {
    const double d = (x - mean) / sd;
    return logNorm - 0.5 * d * d;
  }
};
struct LogNormal {
  double mu, sigma, aux;
  void update() { aux = -0.5 * std::log(2 * M_PI) - std::log(sigma); }
  double logDensity(double x) const {
    if (x <= 0) return -INFINITY;
    const double logx = std::log(x), d = (logx - mu) / sigma;
    return aux - logx - 0.5 * d * d;
  }
};

static double logSumExp(const std::vector<double> &v) {
  double m = -std::numeric_limits<double>::infinity();
  for (double x : v)
    if (x > m) m = x;
  if (std::isinf(m)) return m;
  double s = 0.0;
  for (double x : v) s += std::exp(x - m);
  return m + std::log(s);
}

// Theta: M Psi rows (mean, sd, mu, sigma), K sub-samples, P candidates
static int theta(size_t P, size_t M, size_t K, size_t reps) {
  std::mt19937_64 rng(1);
  std::normal_distribution<double> nrm(0.0, 1.0);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> psi(M * 4), s0(K), s1(K), lp(K), cand(P * 2), ll(P), den;
  for (size_t i = 0; i < M; i++) {
    psi[4 * i] = -2 + 4 * uni(rng);
    psi[4 * i + 1] = 0.2 + 2.8 * uni(rng);
    psi[4 * i + 2] = -1 + 2 * uni(rng);
    psi[4 * i + 3] = 0.2 + 1.8 * uni(rng);
  }
  for (size_t j = 0; j < K; j++) {
    s0[j] = 1.5 * nrm(rng);
    s1[j] = std::exp(0.2 + 0.6 * nrm(rng));
    lp[j] = -6.0 + 5.0 * uni(rng);
  }
  for (size_t c = 0; c < P; c++) {
    cand[2 * c] = 1.5 * nrm(rng);
    cand[2 * c + 1] = std::exp(0.2 + 0.6 * nrm(rng));
  }
  std::vector<double> msDen, msRound;
  double sink = 0;
  for (size_t r = 0; r < reps; r++) {
    auto t0 = std::chrono::steady_clock::now();
    den.clear();
    std::vector<double> logValues(K);
    for (size_t i = 0; i < M; i++) {  // theta.cpp.base:64-83
      Normal n{psi[4 * i], psi[4 * i + 1], 0};
      LogNormal l{psi[4 * i + 2], psi[4 * i + 3], 0};
      n.update();
      l.update();
      for (size_t j = 0; j < K; j++) {
        double logConditionalPrior = 0;
        logConditionalPrior += n.logDensity(s0[j]);
        logConditionalPrior += l.logDensity(s1[j]);
        logValues[j] = logConditionalPrior - lp[j];
      }
      den.push_back(-std::log((double)K) + logSumExp(logValues));
    }
    msDen.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < P; c++) {  // :97-124 without the sub-problem's model
      std::vector<double> values(M);
      for (size_t i = 0; i < M; i++) {
        Normal n{psi[4 * i], psi[4 * i + 1], 0};
        LogNormal l{psi[4 * i + 2], psi[4 * i + 3], 0};
        n.update();
        l.update();
        double logConditionalPrior = 0.;
        logConditionalPrior += n.logDensity(cand[2 * c]);
        logConditionalPrior += l.logDensity(cand[2 * c + 1]);
        values[i] = logConditionalPrior - den[i];
      }
      ll[c] = 0.0 - std::log((double)M) + logSumExp(values);
    }
    msRound.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    sink += ll[r % P] + den[r % M];
  }
  std::sort(msDen.begin(), msDen.end());
  std::sort(msRound.begin(), msRound.end());
  printf("{\"theta_cpu_denominators_ms\": %.3f, \"theta_cpu_loop_ms_per_round\": %.3f, \"theta_cpu_repeats\": %zu, "
         "\"theta_cpu_checksum\": %.17g}\n",
         msDen[msDen.size() / 2], msRound[msRound.size() / 2], reps, sink);
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "theta"))
    return theta(argc > 2 ? atol(argv[2]) : 1000, argc > 3 ? atol(argv[3]) : 2000, argc > 4 ? atol(argv[4]) : 1000,
                 argc > 5 ? atol(argv[5]) : 5);
  const size_t P = argc > 1 ? atol(argv[1]) : 2000, G = argc > 2 ? atol(argv[2]) : 5,
               K = argc > 3 ? atol(argv[3]) : 1000, reps = argc > 4 ? atol(argv[4]) : 5;
  std::mt19937_64 rng(1);
  std::normal_distribution<double> nrm(0.0, 1.0);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<std::vector<double>> x0(G), x1(G), lp(G);
  for (size_t g = 0; g < G; g++)
    for (size_t j = 0; j < K; j++) {
      x0[g].push_back(0.3 * g + 1.5 * nrm(rng));
      x1[g].push_back(std::exp(0.2 + 0.6 * nrm(rng)));
      lp[g].push_back(-6.0 + 5.0 * uni(rng));
    }
  std::vector<double> cand(P * 4), ll(P);
  for (size_t c = 0; c < P; c++) {
    cand[4 * c] = -2 + 4 * uni(rng);
    cand[4 * c + 1] = 0.2 + 2.8 * uni(rng);
    cand[4 * c + 2] = -1 + 2 * uni(rng);
    cand[4 * c + 3] = 0.2 + 1.8 * uni(rng);
  }
  std::vector<double> ms;
  double sink = 0;
  for (size_t r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t c = 0; c < P; c++) {
      Normal n{cand[4 * c], cand[4 * c + 1], 0};
      LogNormal l{cand[4 * c + 2], cand[4 * c + 3], 0};
      n.update();
      l.update();
      double logLikelihood = 0.0;
      for (size_t g = 0; g < G; g++) {
        std::vector<double> logValues(K);
        for (size_t j = 0; j < K; j++) {
          logValues[j] = -lp[g][j];
          logValues[j] += n.logDensity(x0[g][j]);
          logValues[j] += l.logDensity(x1[g][j]);
        }
        logLikelihood += logSumExp(logValues);
      }
      ll[c] = logLikelihood;
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    sink += ll[r % P];
  }
  std::sort(ms.begin(), ms.end());
  printf("{\"cpu_loop_ms_per_round\": %.3f, \"P\": %zu, \"G\": %zu, \"K\": %zu, \"repeats\": %zu, \"checksum\": %.17g}\n",
         ms[ms.size() / 2], P, G, K, reps, sink);
  return 0;
}
