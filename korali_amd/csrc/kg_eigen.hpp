// kg_eigen.hpp — GSL-faithful symmetric eigensolver (gsl_eigen_symmv +
// gsl_eigen_symmv_sort ABS_ASC) for CMAES::updateEigensystem.
#pragma once

#include <vector>

#include "kg_common.hpp"
#include "kg_host_tridiag.hpp"

namespace kg {

struct EigRec;

// profiling callback: phase 0/1 = begin/end of a device stage (events on the
// stream), 2/3 = begin/end of a host stage (wall clock)
typedef void (*ProfileFn)(void *ctx, const char *stage, int phase);

// Which kernels a handle launches and with what geometry: decided once, by
// EigenSolver::init (from N, the chase's place and the KORALI_AMD_* switches
// as they stand at creation), and only read afterwards.
struct EigenPlan {
  // phase A: k_tridiag (one workgroup, the older LDS kernel), k_tridiag_mw,
  // k_tridiag_sq, k_tridiag_mw2, the host core (kg_host_tridiag.cpp)
  enum class Tridiag { Lds, Mw, Sq, Mw2, Host };
  // phase B: k_unpack (one workgroup), k_unpack_wv (one wave per column),
  // k_unpack_mw with every reflector row in LDS / with the rows streamed
  enum class Unpack { OneWg, Wave, MwAllH, MwStream };
  Tridiag tridiag = Tridiag::Lds;
  Unpack unpack = Unpack::OneWg;
  bool sqDpp = true;  // k_tridiag_sq / _mw2: scalar chains on registers / DPP broadcasts (KORALI_AMD_SQ_DPP=0: LDS-streamed)
  int mwRows = 0, mwGroups = 0;  // Mw / Mw2: rows per workgroup, workgroups
  size_t mwLds = 0;              //           dynamic LDS bytes
  int applyTeam = 64, applyRows = 4;  // k_apply: lanes per row team (KORALI_AMD_APPLY_TEAM=16), rows per workgroup
  int chaseEvery = 1;      // host chase: progress word every so many QR steps (KORALI_AMD_CHASE_PUBLISH_EVERY)
  bool chaseFused = true;  // KORALI_AMD_CHASE_FUSED=0: the separate chop pass and rotation copy
};

class EigenSolver {
 public:
  ~EigenSolver();
  void drain();  // waits for the side stream (device chase)
  // hostChase: run the serial implicit-QR Givens recurrence on the calling
  // host core (overlapped with the device unpack); otherwise on one lane.
  int init(int N, bool hostChase);
  int run(const double *C, int diagonal, double *B, double *D, double *minEig, double *maxEig,
          double *eigenFailures, unsigned int *errors, hipStream_t s, ProfileFn prof, void *profCtx);
  // run = run_begin (tridiagonalisation, unpack: workspace only) + run_finish
  int run_begin(const double *C, int diagonal, double *B, double *D, double *minEig, double *maxEig,
          double *eigenFailures, unsigned int *errors, hipStream_t s, ProfileFn prof, void *profCtx);
  int run_finish(const double *C, int diagonal, double *B, double *D, double *minEig, double *maxEig,
          double *eigenFailures, unsigned int *errors, hipStream_t s, ProfileFn prof, void *profCtx);
  bool begun = false;
  // the caller changed C after run_begin: the next run() starts over
  // (phase A again; a host hand-off is published again under a new sequence)
  void invalidate() { begun = false; }
  // C reaches the host core for the tridiagonalisation: run_begin only
  // publishes C, so a caller may issue it as soon as C is final
  bool host_tridiag() const { return plan.tridiag == EigenPlan::Tridiag::Host; }
  unsigned long long *trace = nullptr;  // optional device counters (k_tridiag sub-phases)
  // QR steps / Givens rotations of the last host chase (diagnostics)
  void last_counts(int &steps, int &rotations) const {
    steps = (hostChase && host.meta) ? host.meta[0] : -1;
    rotations = (hostChase && host.meta) ? host.meta[1] : -1;
  }
  bool hostChase = true;
  EigenPlan::Tridiag tridiag_kind() const { return plan.tridiag; }  // (diagnostics)
  // host-core tridiagonalisation: wall time of the last one (ms)
  double last_host_tridiag_ms = 0.0;

 private:
  int N = 0, maxRot = 0;
  EigenPlan plan;  // filled by init, constant afterwards
  int launch_unpack(hipStream_t s, ProfileFn prof, void *profCtx);
  int launch_apply(bool streamed, unsigned long long seq, double *B, double *D, double *minEig, double *maxEig,
                   double *eigenFailures, unsigned int *errors, hipStream_t s);
  // Tridiag::Host: C's lower triangle reaches the host through host-coherent
  // memory (k_publish_c), the host writes the reflectors + tau back
  // (k_fetch_h copies them to gH / tau ahead of the unpack)
  HostTridiag htri;
  double *h_C = nullptr, *d_C_map = nullptr, *h_H = nullptr, *d_H_map = nullptr;
  int ldc = 0;  // row stride of h_C (even: 16-byte rows)
  unsigned int *pubDone = nullptr;  // k_publish_c's workgroup counter (device memory)
  unsigned long long cSeq = 0, pubSeq = 0;  // sequence of the C hand-off the host waits for; publications so far
  double *gH = nullptr, *gQt = nullptr, *tau = nullptr, *dsd = nullptr, *chaseWork = nullptr;
  unsigned long long *comm = nullptr;  // in-launch hand-off granules (N > 128 tridiagonalisation)
  struct Rec {
    int *hdr = nullptr;
    double *cs = nullptr;
    int *meta = nullptr;
    double *eval = nullptr;
    int *perm = nullptr;
    operator EigRec() const;
  } dev, host, hmap;  // hmap: device aliases of the host-coherent chase buffers
  unsigned long long *hprog = nullptr, *dprog = nullptr;  // streamed-chase progress word (host / device view)
  unsigned long long chaseSeq = 0;
  unsigned long long *dprogDev = nullptr;  // fetcher -> apply progress word (device memory)
  double *h_dsd = nullptr, *d_dsd_map = nullptr;  // host-coherent d/sd and its device alias
  unsigned long long dsdSeq = 0;
  std::vector<double> hgc, hgs;
  hipStream_t side = nullptr;
  hipEvent_t ev_dsd = nullptr, ev_chase = nullptr;
};

}  // namespace kg
