// Phase times of the host tridiagonalisation (kg_host_tridiag.cpp built with
// KG_HT_PHASES) on a Wishart matrix: build and run on the box's core,
//   g++ -O3 -std=c++17 -pthread -ffp-contract=off -fno-math-errno -Wno-psabi -DKG_HT_PHASES \
//       -I korali_amd/csrc -o tools/host_tridiag_phases tools/host_tridiag_phases.cpp \
//       korali_amd/csrc/kg_host_tridiag.cpp
//   tools/host_tridiag_phases 128 400
// One handle, `reps` decompositions: best and median wall time, then the
// single-core pass's phases or, with helper threads (the default from N = 128,
// KORALI_AMD_HOST_TRIDIAG_THREADS), each thread's time in the load of C, the
// replicated O(N) work, the pass over its own blocks and the flag waits.
// (Without -DKG_HT_PHASES the tool links too and reports the wall times only.)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include <x86intrin.h>

#include "kg_host_tridiag.hpp"

unsigned long long kg_ht_phases[8];
unsigned long long kg_ht_mt_phases[64][8];

int main(int argc, char **argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 128, reps = argc > 2 ? atoi(argv[2]) : 200;
  std::mt19937_64 g(N);
  std::normal_distribution<double> nd;
  std::vector<double> Y((size_t)N * 2 * N), C((size_t)N * N);
  for (auto &y : Y) y = nd(g);
  for (int i = 0; i < N; i++)
    for (int j = 0; j < N; j++) {
      double s = 0;
      for (int k = 0; k < 2 * N; k++) s += Y[(size_t)i * 2 * N + k] * Y[(size_t)j * 2 * N + k];
      C[(size_t)i * N + j] = s / (2 * N);
    }
  kg::HostTridiag h;
  h.init(N);
  std::vector<double> H((size_t)N * N), tau(N), d(N), sd(N);
  for (int k = 0; k < 5; k++) h.run(C.data(), N, H.data(), tau.data(), d.data(), sd.data());
  for (auto &p : kg_ht_phases) p = 0;
  for (auto &row : kg_ht_mt_phases)
    for (auto &p : row) p = 0;
  std::vector<double> each(reps);
  const unsigned long long c0 = __rdtsc();
  const auto t0 = std::chrono::steady_clock::now();
  for (int k = 0; k < reps; k++) {
    const auto a = std::chrono::steady_clock::now();
    h.run(C.data(), N, H.data(), tau.data(), d.data(), sd.data());
    each[k] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count();
  }
  const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
  const double tsc = (double)(__rdtsc() - c0) / reps, per_us = tsc / us;
  std::sort(each.begin(), each.end());
  printf("N=%d threads=%d: best %.1f median %.1f mean %.1f us per tridiagonalisation (TSC %.0f MHz)\n", N, h.threads,
         each[0], each[reps / 2], us, per_us);
  if (h.threads == 1) {
    static const char *nm[6] = {"copy C", "column i", "dnrm2", "scalars+v", "row pass", "x.v, w"};
    double acc = 0;
    for (int k = 0; k < 6; k++) {
      const double p = kg_ht_phases[k] / (double)reps / per_us;
      acc += p;
      printf(" | %s %.1f", nm[k], p);
    }
    printf(" | rest %.1f\n", us - acc);
    return 0;
  }
  if (!kg_ht_mt_phases[0][2]) return 0;  // (built without the counters)
  // us per decomposition, per thread; per step = / (N - 2)
  printf("  thread | load C | replicated | pass | flag waits | rest\n");
  for (int t = 0; t < h.threads; t++) {
    const unsigned long long *p = kg_ht_mt_phases[t];
    const double ld = p[0] / (double)reps / per_us, rep = (p[1] + p[4]) / (double)reps / per_us,
                 ps = p[2] / (double)reps / per_us, wt = p[3] / (double)reps / per_us;
    printf("  %6d | %6.1f | %10.1f | %4.1f | %10.1f | %.1f\n", t, ld, rep, ps, wt, us - ld - rep - ps - wt);
  }
  return 0;
}
