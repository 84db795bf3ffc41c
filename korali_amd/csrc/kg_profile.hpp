// kg_profile.hpp — the per-stage timer of the population solvers' handles
// (CMA-ES, TMCMC, DEA, MOCMAES, Nested, MCMC), host only.
//
// A handle holds one kg::StageTimes by value.  While it is on, a kg::Stage
// guard brackets the launches of a stage with two events on their stream and
// a kg::HostStage guard times host work with the steady clock; nothing waits
// until read(), which synchronises the stream once, folds the finished event
// pairs into per-stage (ms, count) totals, and hands out one stage's total,
// forgetting it.  While it is off a guard costs one branch and no HIP call.
//
// VRACER's VrStage (kg_vracer.hip) and the Supervisor's SvStage
// (kg_supervisor.hip) are separate on purpose: the first draws its events from
// a pool, weights stages and switches itself off inside graph capture, the
// second waits for every profiled stage.  Either would add options here.
#pragma once

#include <chrono>
#include <map>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "kg_common.hpp"

namespace kg {

struct StageTimes {
  bool on = false;
  std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t>> pending;  // recorded, not yet folded
  std::map<std::string, hipEvent_t> open;                                // mark() begun, not ended
  std::map<std::string, std::pair<double, size_t>> totals;

  // host time of one pass through `name`
  void add(const char *name, double ms) {
    auto &p = totals[name];
    p.first += ms;
    p.second += 1;
  }
  // one pass through `name` that has no time of its own
  void count(const char *name) { totals[name].second += 1; }

  // an explicit begin (phase 0) / end (phase 1) on `s`, recorded whether the
  // timer is on or not.  A second begin replaces the first; an end without a
  // begin is an error.
  int mark(hipStream_t s, const char *stage, int phase) {
    hipEvent_t e;
    KG_HIP(hipEventCreate(&e));
    KG_HIP(hipEventRecord(e, s));
    auto it = open.find(stage);
    if (phase == 0) {
      if (it != open.end()) (void)hipEventDestroy(it->second);
      open[stage] = e;
      return 0;
    }
    if (it == open.end()) {
      (void)hipEventDestroy(e);
      set_error(std::string("profile mark: end of stage '") + stage + "', which was not begun");
      return 1;
    }
    pending.emplace_back(stage, it->second, e);
    open.erase(it);
    return 0;
  }

  // waits for `s`, folds every pending pair into the totals, then returns
  // and forgets `stage`'s total ((0, 0) for a stage nobody recorded)
  int read(hipStream_t s, const char *stage, double *ms_total, size_t *n) {
    KG_HIP(hipStreamSynchronize(s));
    for (auto &t : pending) {
      float ms = 0.f;
      KG_HIP(hipEventElapsedTime(&ms, std::get<1>(t), std::get<2>(t)));
      add(std::get<0>(t).c_str(), ms);
      (void)hipEventDestroy(std::get<1>(t));
      (void)hipEventDestroy(std::get<2>(t));
    }
    pending.clear();
    auto it = totals.find(stage ? stage : "");
    if (it == totals.end()) {
      *ms_total = 0;
      *n = 0;
    } else {
      *ms_total = it->second.first;
      *n = it->second.second;
      totals.erase(it);
    }
    return 0;
  }

  // the handle's destroy: the events nobody read
  void release() {
    for (auto &t : pending) {
      (void)hipEventDestroy(std::get<1>(t));
      (void)hipEventDestroy(std::get<2>(t));
    }
    pending.clear();
    for (auto &m : open) (void)hipEventDestroy(m.second);
    open.clear();
  }
};

// the launches between construction and destruction, on stream `s`
struct Stage {
  StageTimes &t;
  const char *name;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  Stage(StageTimes &t_, hipStream_t s_, const char *n) : t(t_), name(n), s(s_) {
    if (t.on) {
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      (void)hipEventRecord(a, s);
    }
  }
  ~Stage() {
    if (t.on) {
      (void)hipEventRecord(b, s);
      t.pending.emplace_back(name, a, b);
    }
  }
  Stage(const Stage &) = delete;
  Stage &operator=(const Stage &) = delete;
};

// host work between construction and destruction, by the steady clock
struct HostStage {
  StageTimes &t;
  const char *name;
  std::chrono::steady_clock::time_point t0;
  HostStage(StageTimes &t_, const char *n) : t(t_), name(n), t0(std::chrono::steady_clock::now()) {}
  ~HostStage() {
    if (t.on) t.add(name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  HostStage(const HostStage &) = delete;
  HostStage &operator=(const HostStage &) = delete;
};

}  // namespace kg
