// One-core CPU loop of the Hierarchical/Psi log-likelihood with libm, as the
// reference computes it (Psi::evaluateLogLikelihood + logSumExp: one
// getLogDensity call per term, a vector of K values per group, two passes),
// at the shape tools/time_hier.py times on the device.
//   g++ -O2 -o tools/hier_cpu_loop tools/hier_cpu_loop.cpp && tools/hier_cpu_loop [P] [G] [K] [repeats]
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

int main(int argc, char **argv) {
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
