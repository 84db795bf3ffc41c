// The multi-threaded host tridiagonalisation's protocol under the thread and
// the address/undefined-behaviour sanitizers: kg_host_tridiag.cpp alone, no
// device code, its own main.  Build twice and run each directly,
//   g++ -O1 -g -std=c++17 -pthread -ffp-contract=off -fno-math-errno -Wno-psabi -fsanitize=thread
//       -I korali_amd/csrc -o tools/host_tridiag_races_tsan tools/host_tridiag_races.cpp
//       korali_amd/csrc/kg_host_tridiag.cpp
//   (the same with -fsanitize=address,undefined -o tools/host_tridiag_races_asan)
//   tools/host_tridiag_races_tsan [decompositions, default 200]
// At N = 25 and 128 with 2, 4 and 8 threads: `decompositions` runs on fresh
// matrices, a new pool every 25th, every output compared bit for bit with the
// single-core pass.  Exit status 0: all equal (the sanitizer reports on its own).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kg_host_tridiag.hpp"

namespace {
struct Out {
  std::vector<double> H, tau, d, sd;
  explicit Out(int N) : H((size_t)N * N), tau(N), d(N), sd(N) {}
  void clear() {
    for (auto *a : {&H, &tau, &d, &sd}) std::fill(a->begin(), a->end(), 0.0);
  }
  bool same(const Out &o, int N) const {
    bool ok = !std::memcmp(d.data(), o.d.data(), sizeof(double) * N) &&
              !std::memcmp(sd.data(), o.sd.data(), sizeof(double) * (N - 1)) &&
              !std::memcmp(tau.data(), o.tau.data(), sizeof(double) * (N - 2));
    for (int i = 0; ok && i + 2 < N; i++)
      ok = !std::memcmp(&H[(size_t)i * N], &o.H[(size_t)i * N], sizeof(double) * (N - 1 - i));
    return ok;
  }
};

void matrix(int N, unsigned seed, std::vector<double> &C) {
  std::mt19937_64 g(seed);
  std::normal_distribution<double> nd;
  const int K = N + 3;
  std::vector<double> Y((size_t)N * K);
  for (auto &y : Y) y = nd(g);
  for (int i = 0; i < N; i++)
    for (int j = 0; j <= i; j++) {
      double s = 0;
      for (int k = 0; k < K; k++) s += Y[(size_t)i * K + k] * Y[(size_t)j * K + k];
      C[(size_t)i * N + j] = C[(size_t)j * N + i] = s / K;
    }
  if (seed % 7 == 3) {  // a zero column in the middle: a tau = 0 step
    const int z = N / 2;
    for (int k = 0; k < N; k++) C[(size_t)z * N + k] = C[(size_t)k * N + z] = 0.0;
    C[(size_t)z * N + z] = 2.0;
  }
}
}  // namespace

int main(int argc, char **argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 200;
  int bad = 0;
  for (int N : {25, 128}) {
    std::vector<double> C((size_t)N * N);
    Out ref(N), got(N);
    setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", "1", 1);
    kg::HostTridiag one;
    if (one.init(N)) return 2;
    for (int P : {2, 4, 8}) {
      setenv("KORALI_AMD_HOST_TRIDIAG_THREADS", std::to_string(P).c_str(), 1);
      kg::HostTridiag *h = nullptr;
      int threads = 0, diff = 0;
      for (int k = 0; k < reps; k++) {
        if (k % 25 == 0) {  // a new pool
          delete h;
          h = new kg::HostTridiag();
          if (h->init(N)) return 2;
          threads = h->threads;
        }
        matrix(N, 1000u * N + 10u * k + P, C);
        ref.clear(), got.clear();
        one.run(C.data(), N, ref.H.data(), ref.tau.data(), ref.d.data(), ref.sd.data());
        if (k % 3 == 0) h->wake();
        h->run(C.data(), N, got.H.data(), got.tau.data(), got.d.data(), got.sd.data());
        diff += !got.same(ref, N);
      }
      delete h;
      std::printf("N=%d asked %d threads, ran %d: %d decompositions, %d differ from the single-core pass\n", N, P,
                  threads, reps, diff);
      bad += diff;
    }
  }
  return bad != 0;
}
