/*
 * korali_amd.h — C-ABI of the MI355X-native population-generation engine.
 *
 * This is the drop-in boundary for Korali's population-based solver
 * generation loop.  The reference calls GSL / gslcblas directly from its C++
 * solver modules; each entry point below replaces one of those solver
 * stages (reference paths relative to the korali root):
 *
 *   kg_cmaes_initialize   CMAES::setInitialConfiguration   CMAES.cpp.base:14-184
 *                         (initMuWeights :233-284, initCovariance :286-313)
 *   kg_cmaes_sample       CMAES::prepareGeneration         CMAES.cpp.base:439-492
 *                         (updateEigensystem/eigen :869-938, sampleSingle
 *                          :494-545, Optimizer::isSampleFeasible
 *                          optimizer.cpp.base:5-14, Normal::getRandomNumber
 *                          univariate/normal/normal.cpp.base:32-35)
 *   kg_cmaes_eval_builtin Optimization::evaluate → user objective
 *                         optimization.cpp.base:26-34, batched over λ
 *   kg_cmaes_sample_eval  the two above in one call (one launch where it applies)
 *   kg_cmaes_get_candidates / kg_cmaes_set_fitness
 *                         KORALI_START/WAITALL/GET of CMAES::runGeneration
 *                         CMAES.cpp.base:204-224 (host-callback objectives)
 *   kg_cmaes_update       CMAES::updateDistribution        CMAES.cpp.base:547-688
 *                         (sort_index :940-950, adaptC :690-718,
 *                          updateSigma :720-761, numericalErrorTreatment :763-772)
 *   kg_cmaes_generation   CMAES::runGeneration             CMAES.cpp.base:186-231
 *   kg_cmaes_{get,set}_field / _{get,set}_rng
 *                         Module::getConfiguration / setConfiguration of the
 *                         solver state incl. RNG "Range" (distribution.cpp.base:10-62)
 *
 *   kg_tmcmc_*            TMCMC::runGeneration             TMCMC.cpp.base:107-157
 *   kg_supervisor_*       DeepSupervisor::runGeneration / getEvaluation
 *                         deepSupervisor.cpp.base:97-187 (float32 networks; the
 *                         section below cites each layer and optimizer)
 *
 * Conventions: every function returns 0 on success and non-zero on error;
 * kg_last_error() returns the message (thread-local).  No C++ exceptions or
 * torch types cross this boundary.  Host arrays are caller-owned and copied;
 * device buffers are owned by the handle.  Matrices are row-major doubles,
 * exactly as the reference stores them (std::vector<double> N*N).
 */
#ifndef KORALI_AMD_H
#define KORALI_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_ABI_VERSION 8

const char *kg_last_error(void);
int kg_abi_version(void);
int kg_device_count(int *count);

/* -------------------------------------------------------------- CMA-ES */
typedef struct kg_cmaes_s *kg_cmaes_t;

enum kg_mu_type { KG_MU_LOGARITHMIC = 0, KG_MU_LINEAR = 1, KG_MU_EQUAL = 2, KG_MU_PROPORTIONAL = 3 };
enum kg_objective { KG_OBJ_NEGATIVE_ROSENBROCK = 0, KG_OBJ_NEGATIVE_ACKLEY = 1, KG_OBJ_NEGATIVE_SPHERE = 2 };
/* Covariance rank-mu update: EXACT replays the reference's sequential
 * per-element summation (bit-faithful); MFMA sums y_k y_k^T on the FP64
 * matrix cores (v_mfma_f64_16x16x4f64), within 1e-12 relative. */
enum kg_cov_mode { KG_COV_EXACT = 0, KG_COV_MFMA = 1 };

typedef struct {
  size_t variable_count;  /* N  (CMAES "Variable Count") */
  size_t population_size; /* λ  ("Population Size") */
  size_t mu_value;        /* μ  ("Mu Value"; 0 → λ/2, CMAES.cpp.base:27) */
  int mu_type;            /* enum kg_mu_type ("Mu Type") */
  double initial_sigma_cumulation_factor; /* ≤0 → formula default */
  double initial_damp_factor;             /* ≤0 → formula default */
  double initial_cumulative_covariance;   /* ≤0 or >1 → formula default */
  int is_sigma_bounded;                   /* "Is Sigma Bounded" */
  int diagonal_covariance;                /* "Diagonal Covariance" */
  int mirrored_sampling;                  /* "Mirrored Sampling" (pairs z, -z; CMAES.cpp.base:461-491) */
  double max_infeasible_resamplings;      /* "Termination Criteria/Max Infeasible Resamplings" */
  const double *lower_bound;              /* N, may be NULL → -inf */
  const double *upper_bound;              /* N, may be NULL → +inf */
  const double *initial_value;            /* N, NaN → midpoint of bounds */
  const double *initial_std;              /* N, NaN → 0.3*(ub-lb) */
  const double *min_std_update;           /* N, may be NULL → 0 */
  uint64_t normal_seed;                   /* seed of the Normal generator (GSL mt19937) */
  uint64_t uniform_seed;                  /* seed of the Uniform generator */
  int cov_mode;                           /* enum kg_cov_mode */
  int device;                             /* HIP device ordinal */
  int store_bdz;                          /* also keep the BDZ matrix (state export) */
  int eigen_device_chase;                 /* 0: implicit-QR Givens recurrence on the calling host
                                             core, overlapped with the device unpack (default);
                                             1: on one device lane.  Identical results. */
  int shard_rank;                         /* population sharding: this rank's index */
  int shard_count;                        /* ranks sharing one population; 0 or 1 = unsharded */
  /* "Use Gradient Information" / "Gradient Step Size" (CMAES.cpp.base:82-87,
   * :611-621): the mean moves by sum_i w_i step / sqrt(N) g_(i) after the
   * weighted recombination; the samples' gradients come through
   * kg_cmaes_set_gradients (host-evaluated objectives only, unsharded) */
  int use_gradients;
  double gradient_step_size;
  /* "Granularity" of each variable (N, may be NULL → all 0 = continuous;
   * CMAES.cpp.base:44-50, :515-544, :834-867): samples are rounded to it,
   * discrete mutations drawn from the Uniform Generator, sigma follows the
   * masked path length; with or without Mirrored Sampling, sharded or not. */
  const double *granularity;
  /* CCMA-ES (Problem "Constraints"; CMAES.cpp.base:54-68, :132-170,
   * :315-437, :551-580, :724-731, :774-832).  constraint_count > 0: the
   * viability regime (viability_population_size samples, viability_mu_value
   * → half of it) until the mean satisfies every constraint; the constraint
   * values come from the callback of kg_cmaes_set_constraints.  The four
   * doubles below are then required (CMAES.config defaults: 1e6, 0.1818,
   * 0.1, 0.2).  Not with Mirrored Sampling, discrete variables or
   * sharding. */
  size_t constraint_count;
  size_t viability_population_size;
  size_t viability_mu_value;
  double max_covariance_matrix_corrections;
  double target_success_rate;
  double covariance_matrix_adaption_strength;
  double global_success_learning_rate;
} kg_cmaes_cfg;

int kg_cmaes_create(const kg_cmaes_cfg *cfg, kg_cmaes_t *out);

/* Constraint values of `rows` samples (row-major rows x N, host memory):
 * out[r * constraint_count + c] = constraint c at X[r] (Optimization::
 * evaluateConstraints, optimization.cpp.base:11-24: the reference runs
 * sample.run(_constraints[c]) for c in order).  ids[r] = the sample's index
 * in the population, or (size_t)-1 for the mean (checkMeanAndSetRegime).
 * Return 0, or nonzero to abort the generation (kg_last_error() then names
 * the callback). */
typedef int (*kg_constraint_fn)(const double *X, size_t rows, size_t N, const size_t *ids, double *out, void *ctx);
int kg_cmaes_set_constraints(kg_cmaes_t h, kg_constraint_fn fn, void *ctx);
/* CMAES::runGeneration up to the objective with constraints
 * (CMAES.cpp.base:190-196): checkMeanAndSetRegime, prepareGeneration,
 * updateConstraints and handleConstraints (covariance shrunk along the
 * constraint normals on the device, re-decomposed, the violating samples
 * redrawn from the Normal stream and re-evaluated).  Then evaluate the
 * current population (kg_cmaes_population_size rows) and kg_cmaes_update. */
int kg_cmaes_prepare_constrained(kg_cmaes_t h, size_t generation);
/* the current population / mu (CCMA-ES viability regime: the viability sizes) */
int kg_cmaes_population_size(kg_cmaes_t h, size_t *lambda, size_t *mu);
int kg_cmaes_destroy(kg_cmaes_t h);
int kg_cmaes_initialize(kg_cmaes_t h);
int kg_cmaes_sample(kg_cmaes_t h);
int kg_cmaes_eval_builtin(kg_cmaes_t h, int objective);
/* kg_cmaes_sample + kg_cmaes_eval_builtin in one call, with the same results.
 * For N <= 128, a full covariance, one shard, infinite bounds and no discrete
 * variables the draw and the objective are one launch; every other
 * configuration, and a draw whose overflow guard sends it through the redraw
 * rounds, runs the two steps.  KORALI_AMD_FUSED_DRAW=0 (read by
 * kg_cmaes_create) always runs the two steps. */
int kg_cmaes_sample_eval(kg_cmaes_t h, int objective);
int kg_cmaes_get_candidates(kg_cmaes_t h, double *X, size_t ld);
int kg_cmaes_set_fitness(kg_cmaes_t h, const double *F);
/* Bayesian problems (F(x) = logPosterior, bayesian.cpp.base:79-84): like
 * kg_cmaes_set_fitness, but -inf (a candidate outside the prior's support)
 * is a valid value; NaN and +inf are still rejected.  Ties sort by index. */
int kg_cmaes_set_log_posterior(kg_cmaes_t h, const double *F);
/* the samples' "Gradient" (lambda x N, row i = sample i), with
 * use_gradients, after kg_cmaes_set_fitness and before kg_cmaes_update */
int kg_cmaes_set_gradients(kg_cmaes_t h, const double *G);
int kg_cmaes_update(kg_cmaes_t h, size_t generation);
/* One whole generation (CMAES::runGeneration).  The device work is enqueued
 * on the handle's stream, but the call itself BLOCKS the calling thread for
 * part of it: with the default host-side Givens chase (cfg eigen_device_chase = 0)
 * the thread waits for the generation's tridiagonal form and then runs the
 * implicit-QR chase itself (kg_eigen.hip EigenSolver::run), streaming the
 * rotations to the device; the call returns once the chase is done and the
 * rest of the generation is queued.  With the device chase (eigen_device_chase =
 * 1, bit-identical, slower) the call only enqueues. */
int kg_cmaes_generation(kg_cmaes_t h, size_t generation, int objective);
/* The next generation's first half ahead of time: the generator prefetch /
 * polar pass and the eigendecomposition's tridiagonalisation and unpack,
 * which touch only workspace (no state a result file holds), so a caller
 * can enqueue them before deciding whether that generation will run (the
 * engine does, before its termination check).  kg_cmaes_sample completes
 * it; without this call kg_cmaes_sample does both halves. */
int kg_cmaes_begin_sample(kg_cmaes_t h);
/* The termination scalars of the last kg_cmaes_update without a stream
 * synchronisation: the device publishes them (and the error flags) into
 * host-coherent memory at the end of the update; this spins until they
 * arrive.  out[] = Model Evaluation Count, Infeasible Sample Count, Maximum
 * Covariance Eigenvalue, Minimum Covariance Eigenvalue, Current Min Standard
 * Deviation, Current Max Standard Deviation, Best Ever Value, Current Best
 * Value, Previous Best Value.  Device-side errors are reported as by
 * kg_cmaes_synchronize.  (Experiment::run's check, experiment.cpp.base:56-99
 * + the generated CMAES/optimizer/solver checkTermination.) */
#define KG_TERMINATION_FIELDS 9
int kg_cmaes_wait_termination_fields(kg_cmaes_t h, double *out);
/* Population sharding over shard_count ranks (one handle per rank, state
 * replicated, λ % shard_count == 0).  kg_cmaes_sample and
 * kg_cmaes_eval_builtin then cover only rows [rank λ/S, (rank+1) λ/S) (with
 * finite bounds, discrete variables, Mirrored Sampling or a diagonal
 * covariance kg_cmaes_sample draws the whole population on every rank: the
 * redraw walk and the ±z pairs are sequential over it);
 * the caller all-gathers "Value Vector" (λ doubles, shards in rank order)
 * — with use_gradients also "Gradients" (λ x N doubles, each rank's rows set
 * by kg_cmaes_set_gradients, shards in rank order) — and then runs the
 * update protocol of the handle's covariance mode.
 *
 * cov_mode KG_COV_EXACT — the reference's summation order, every rank's state
 * bit-identical to the unsharded run (CMAES.cpp.base:603-609, :690-718 sum
 * mean and rank-μ over the selected rows in selection order):
 *   kg_cmaes_update_partial    replicated sort, best bookkeeping; this rank's
 *                              selected rows (ascending selection rank) packed
 *                              into block `rank` of "Shard Rows";
 *   kg_cmaes_shard_row_count   waits for the packing; *count = doubles per
 *                              rank block (0: nothing to exchange);
 *   caller                     in-place all-gather of "Shard Rows", *count
 *                              doubles per rank (skip when 0);
 *   kg_cmaes_update_rows       the μ selected rows in selection order on every
 *                              rank; mean and paths (replicated); the rank-μ
 *                              chains of this rank's share of the covariance's
 *                              lower triangle into "Shard Covariance" (packed,
 *                              entry d (d+1)/2 + e, INT64_MIN bits elsewhere);
 *   caller                     MAX all-reduce of "Shard Covariance" viewed as
 *                              int64 (every entry's owner's exact bits);
 *   kg_cmaes_update_finalize   covariance, σ.
 *
 * cov_mode KG_COV_MFMA — per-shard partial sums (within 1e-12 of the
 * sequential order): kg_cmaes_update_partial, sum all-reduce of "Shard
 * Partials", kg_cmaes_update_finalize.
 *
 * The sort and selection are replicated bit-exactly in both modes. */
int kg_cmaes_update_partial(kg_cmaes_t h, size_t generation);
int kg_cmaes_shard_row_count(kg_cmaes_t h, size_t *count);
int kg_cmaes_update_rows(kg_cmaes_t h, size_t generation);
int kg_cmaes_update_finalize(kg_cmaes_t h, size_t generation);
int kg_cmaes_synchronize(kg_cmaes_t h); /* waits and reports device-side errors */
/* named state fields, keys as in the reference's solver JSON
 * ("Sigma", "Covariance Matrix", "Current Mean", ...); sizes in doubles */
int kg_cmaes_field_size(kg_cmaes_t h, const char *name, size_t *n);
int kg_cmaes_get_field(kg_cmaes_t h, const char *name, double *out, size_t n);
int kg_cmaes_set_field(kg_cmaes_t h, const char *name, const double *in, size_t n);
/* several scalar fields with one device read (termination checks, logging) */
int kg_cmaes_get_fields(kg_cmaes_t h, const char *const *names, size_t count, double *out);
int kg_cmaes_get_sorting_index(kg_cmaes_t h, uint64_t *out);
/* GSL mt19937 state as Korali serialises it: 624 x uint64 words + int32 mti
 * + 4 pad bytes = 5000 bytes.  which: 0 Normal, 1 Uniform generator. */
int kg_cmaes_get_rng(kg_cmaes_t h, int which, void *state5000);
int kg_cmaes_set_rng(kg_cmaes_t h, int which, const void *state5000);
/* device pointer of a named buffer (zero-copy interop) and the HIP stream */
int kg_cmaes_device_ptr(kg_cmaes_t h, const char *name, void **ptr);
int kg_cmaes_stream(kg_cmaes_t h, void **stream);
/* kernel timing probe: average device time (ms) of the named kernel family
 * over the last generation(s) since the previous call, measured with HIP
 * events on the handle's stream; enable with kg_cmaes_profile(h, 1).
 * "adaptC_row" / "adaptC_lane" carry no time: their count is how often that
 * exact covariance kernel was launched. */
int kg_cmaes_profile(kg_cmaes_t h, int enable);
int kg_cmaes_profile_read(kg_cmaes_t h, const char *stage, double *ms_total, size_t *count);
/* A stage bracketed by the caller (phase 0 = begin, 1 = end): an event pair
 * on the handle's stream, read back with kg_cmaes_profile_read -- the C++
 * engine's exchange steps (collectives enqueued on this stream) under
 * KORALI_AMD_EXCHANGE_PROFILE=1.  Returns 1 for an end without a begin. */
int kg_cmaes_profile_mark(kg_cmaes_t h, const char *stage, int phase);

/* ----------------------------------------------------------------- DEA */
/* Optimizer/DEA (differential evolution), bit-exact to DEA.cpp.base:
 *
 *   kg_dea_initialize     DEA::setInitialConfiguration     DEA.cpp.base:15-61
 *                         (initSamples :87-97)
 *   kg_dea_prepare        DEA::prepareGeneration           DEA.cpp.base:99-116
 *                         (mutateSingle :118-176, fixInfeasible :178-190,
 *                          Optimizer::isSampleFeasible optimizer.cpp.base:5-14,
 *                          Uniform::getRandomNumber → gsl_rng_uniform)
 *   kg_dea_eval_builtin   Optimization::evaluate → user objective
 *                         optimization.cpp.base:26-34, batched over P
 *   kg_dea_get_candidates / kg_dea_set_fitness
 *                         KORALI_START/WAITALL/GET of DEA::runGeneration
 *                         DEA.cpp.base:69-82, :195-196 (host-callback objectives)
 *   kg_dea_update         DEA::updateSolver                DEA.cpp.base:192-278
 *   kg_dea_generation     DEA::runGeneration               DEA.cpp.base:63-85
 *   kg_dea_{get,set}_field / _{get,set}_rng
 *                         Module::getConfiguration / setConfiguration of the
 *                         solver state incl. RNG "Range" (distribution.cpp.base:10-62)
 *
 * The proposal is a chain over the samples on one workgroup: every draw
 * comes from one sequential uniform stream and a sample consumes a
 * data-dependent number of words (the DEA proposal chain).  The
 * kernel reads a window of `window_words` peeked draws and stops before an
 * attempt that would run past it; kg_dea_prepare relaunches from there. */
typedef struct kg_dea_s *kg_dea_t;

enum kg_dea_mutation_rule { KG_DEA_MUTATION_FIXED = 0, KG_DEA_MUTATION_SELF_ADAPTIVE = 1 };
enum kg_dea_parent_rule { KG_DEA_PARENT_RANDOM = 0, KG_DEA_PARENT_BEST = 1 };
enum kg_dea_accept_rule {
  KG_DEA_ACCEPT_BEST = 0,
  KG_DEA_ACCEPT_GREEDY = 1,
  KG_DEA_ACCEPT_ITERATIVE = 2,
  KG_DEA_ACCEPT_IMPROVED = 3
};

typedef struct {
  size_t variable_count;     /* N */
  size_t population_size;    /* P ("Population Size"; >= 4 with parent rule Random, >= 3 with Best) */
  const double *lower_bound; /* N, finite */
  const double *upper_bound; /* N, finite, >= lower_bound (DEA.cpp.base:19-21) */
  double crossover_rate;     /* "Crossover Rate" */
  double mutation_rate;      /* "Mutation Rate" */
  int mutation_rule;         /* enum kg_dea_mutation_rule ("Mutation Rule") */
  int parent_rule;           /* enum kg_dea_parent_rule ("Parent Selection Rule") */
  int accept_rule;           /* enum kg_dea_accept_rule ("Accept Rule") */
  int fix_infeasible;        /* "Fix Infeasible" */
  uint64_t normal_seed;      /* seed of the Normal generator (kept and exported, never drawn from) */
  uint64_t uniform_seed;     /* seed of the Uniform generator (GSL mt19937) */
  size_t window_words;       /* uniform draws the proposal kernel sees per launch; 0 → max(4096, 4 P (N + 8)).
                                A window smaller than one attempt is doubled on demand. */
  size_t max_windows;        /* windows one kg_dea_prepare may use before it reports a configuration
                                that cannot become feasible; 0 → 1024.  Not a reference setting: the
                                reference redraws forever there, and this bound is what turns that into
                                an error (kg_last_error) instead of a hang. */
  int device;                /* HIP device ordinal */
} kg_dea_cfg;

/* Every entry checks its arguments: a null handle or pointer, a stage called
 * on a handle without a population, or ld < N is an error, not a crash. */
int kg_dea_create(const kg_dea_cfg *cfg, kg_dea_t *out);
int kg_dea_destroy(kg_dea_t h);
int kg_dea_initialize(kg_dea_t h);
/* candidates of `generation` (generation 1: the initial samples) and
 * "Previous Value Vector" = "Value Vector" (DEA.cpp.base:115).  Blocks until
 * the chain is through (one small device read per window). */
int kg_dea_prepare(kg_dea_t h, size_t generation);
int kg_dea_eval_builtin(kg_dea_t h, int objective); /* enum kg_objective; "Model Evaluation Count" += P */
int kg_dea_get_candidates(kg_dea_t h, double *X, size_t ld);
int kg_dea_set_fitness(kg_dea_t h, const double *F); /* finite values only; "Model Evaluation Count" += P */
int kg_dea_update(kg_dea_t h, size_t generation);
/* prepare + eval_builtin + update (generation 1 initializes a fresh handle first) */
int kg_dea_generation(kg_dea_t h, size_t generation, int objective);
int kg_dea_synchronize(kg_dea_t h); /* waits and reports device-side errors */
/* named state fields, keys as in the reference's solver JSON ("Sample
 * Population", "Candidate Population", "Value Vector", "Previous Value
 * Vector", "Current Mean", "Previous Mean", "Best Ever Variables", "Current
 * Best Variables", "Max Distances"; scalars "Best Ever Value", "Previous Best
 * Ever Value", "Current Best Value", "Previous Best Value", "Best Sample
 * Index", "Infeasible Sample Count", "Model Evaluation Count", "Mutation
 * Rate", "Crossover Rate", "Current Minimum Step Size"); sizes in doubles */
int kg_dea_field_size(kg_dea_t h, const char *name, size_t *n);
int kg_dea_get_field(kg_dea_t h, const char *name, double *out, size_t n);
int kg_dea_set_field(kg_dea_t h, const char *name, const double *in, size_t n);
/* 5000-byte GSL states as for CMA-ES.  which: 0 Normal, 1 Uniform generator. */
int kg_dea_get_rng(kg_dea_t h, int which, void *state5000);
int kg_dea_set_rng(kg_dea_t h, int which, const void *state5000);
/* Diagnostics only (replaces nothing in the reference, holds no solver state):
 * windows the last kg_dea_prepare used, and the current window size in words.
 * The tests read it to see that the relaunch and window-growth paths ran. */
int kg_dea_windows(kg_dea_t h, size_t *last_windows, size_t *window_words);
/* stage timing as kg_cmaes_profile; stages "words" (stream production and
 * the uniform conversion), "propose", "evaluate", "update" */
int kg_dea_profile(kg_dea_t h, int enable);
int kg_dea_profile_read(kg_dea_t h, const char *stage, double *ms_total, size_t *count);

/* ------------------------------------------------------------- MOCMAES */
/* Optimizer/MOCMAES (multi-objective CMA-ES), bit-exact to MOCMAES.cpp.base:
 *
 *   kg_mocmaes_initialize     MOCMAES::setInitialConfiguration  MOCMAES.cpp.base:10-140
 *   kg_mocmaes_prepare        MOCMAES::prepareGeneration        MOCMAES.cpp.base:172-184
 *                             (sampleSingle :186-228: parent pick :188-195,
 *                              gsl_linalg_cholesky_decomp1 + gsl_matrix_scale :198-207,
 *                              Multivariate Normal::getRandomVector
 *                              multivariate/normal/normal.cpp.base:30-35 until
 *                              Optimizer::isSampleFeasible optimizer.cpp.base:5-14 holds :209-217)
 *   kg_mocmaes_eval_builtin   Optimization::evaluateMultiple → user objective
 *                             optimization.cpp.base:36-45, batched over P
 *   kg_mocmaes_get_candidates / kg_mocmaes_set_values
 *                             KORALI_START/WAITALL/GET of MOCMAES::runGeneration
 *                             MOCMAES.cpp.base:148-166 (host-callback objectives)
 *   kg_mocmaes_update         MOCMAES::updateDistribution       MOCMAES.cpp.base:334-408
 *                             (sortSampleIndices :230-332) and
 *                             MOCMAES::updateStatistics         MOCMAES.cpp.base:410-520
 *   kg_mocmaes_generation     MOCMAES::runGeneration            MOCMAES.cpp.base:142-170
 *   kg_mocmaes_{get,set}_field / _{get,set}_rng
 *                             Module::getConfiguration / setConfiguration of the
 *                             solver state incl. RNG "Range" (distribution.cpp.base:10-62)
 *
 * Limits (MOCMAES): N <= 128 (a parent's factor is kept in LDS),
 * N <= P (updateStatistics reads _currentSigma[d] for d < N, :455: out of
 * bounds in the reference otherwise), 2 <= K <= 8.
 * A parent covariance with a non-positive Cholesky pivot is an error here
 * (kg_last_error); the reference ignores gsl_linalg_cholesky_decomp1's status
 * (:203-206) and draws from the partially factored matrix.
 * "Infeasible Sample Count" stays 0: the reference's increment is commented
 * out (:215). */
typedef struct kg_mocmaes_s *kg_mocmaes_t;

enum kg_mocmaes_parent_order {
  KG_MOCMAES_PARENTS_DESCENDING = 0, /* slot values.size() - sortedIndices[i] - 1 (MOCMAES.cpp.base:385) */
  KG_MOCMAES_PARENTS_RECORDED = 1    /* the slot order of the reference's committed 2021 result files
                                        (tests/python/plot/mocmaes): ascending index of the merged
                                        population; not a Korali setting */
};

/* builtin objective kernels (examples/optimization/multiobjective/_model/model.py) */
enum kg_mocmaes_objective {
  KG_MOCMAES_OBJ_ROSENBROCK_SPHERE = 0,     /* negative_rosenbrock_and_sphere, K = 2 */
  KG_MOCMAES_OBJ_ROSENBROCK_TWO_SPHERES = 1 /* negative_rosenbrock_and_two_spheres, K = 3 */
};

typedef struct {
  size_t variable_count;     /* N, 1..128 and <= population size */
  size_t population_size;    /* P ("Population Size"; 0 → ceil(4 + floor(3 log N)), :24) */
  size_t mu_value;           /* "Mu Value" (0 → P / 2, :25), <= P */
  size_t num_objectives;     /* K ("Num Objectives"), 2..8 */
  const double *lower_bound; /* N (may be infinite where value and deviation are given) */
  const double *upper_bound; /* N */
  const double *initial_value; /* N or NULL; non-finite → inferred from finite bounds (:73-78).  The
                                  reference never reads it again: the parents start at 0 (:119) */
  const double *initial_sdev;  /* N or NULL; non-finite → 0.3 (upper - lower) (:80-85) */
  double evolution_path_adaption_strength; /* < 0 → 2 / (N + 2) (:127) */
  double covariance_learning_rate;         /* < 0 → 2 / (N^2 + 6) (:128) */
  double target_success_rate;              /* "Target Success Rate", (0, 1] */
  double success_learning_rate;            /* "Success Learning Rate", (0, 1] */
  int parent_order;          /* enum kg_mocmaes_parent_order */
  uint64_t multinormal_seed; /* seed of the Multinormal generator (GSL mt19937) */
  uint64_t uniform_seed;     /* seed of the Uniform generator */
  size_t window_blocks;      /* blocks of N normals the draw sees per launch; at least P + 64 */
  size_t max_windows;        /* windows one kg_mocmaes_prepare may use before it reports a sample that
                                never becomes feasible; 0 → 1024.  Not a reference setting: the
                                reference redraws forever there. */
  size_t archive_rows;       /* first capacity of the "Sample Collection" buffers (grown on demand);
                                0 → max(4 P, 1024) */
  int device;                /* HIP device ordinal */
} kg_mocmaes_cfg;

/* Every entry checks its arguments, and create its configuration, before the
 * device is touched. */
int kg_mocmaes_create(const kg_mocmaes_cfg *cfg, kg_mocmaes_t *out);
int kg_mocmaes_destroy(kg_mocmaes_t h);
int kg_mocmaes_initialize(kg_mocmaes_t h);
/* Previous* = Current* (a buffer swap) and the P draws of `generation`
 * (generation 1 initializes a fresh handle first).  Blocks until the draw
 * chain is through (one small device read per window).  The offspring's
 * covariance, sigma, path and success rate are written by kg_mocmaes_update. */
int kg_mocmaes_prepare(kg_mocmaes_t h, size_t generation);
int kg_mocmaes_eval_builtin(kg_mocmaes_t h, int objective); /* enum kg_mocmaes_objective; "Model Evaluation Count" += P */
int kg_mocmaes_get_candidates(kg_mocmaes_t h, double *X, size_t ld);
int kg_mocmaes_set_values(kg_mocmaes_t h, const double *V); /* P x K row-major, finite; "Model Evaluation Count" += P */
int kg_mocmaes_update(kg_mocmaes_t h, size_t generation);
int kg_mocmaes_generation(kg_mocmaes_t h, size_t generation, int objective);
int kg_mocmaes_synchronize(kg_mocmaes_t h); /* waits and reports device-side errors */
/* named state fields, keys as in MOCMAES.config's Internal Settings: {Current,
 * Previous, Parent} x {"Sample Population", "Sigma", "Covariance Matrix",
 * "Evolution Paths", "Success Probabilities"}, "Current Values", "Previous
 * Values", "Parent Index", {"Best Ever", "Previous Best", "Current Best"} x
 * {"Values", "Variables Vector"}, "Current Best Value Differences", "Current
 * Best Variable Differences", "Current Min Standard Deviations", "Current Max
 * Standard Deviations", "Sample Collection", "Sample Value Collection";
 * scalars "Current Non Dominated Sample Count", "Infeasible Sample Count",
 * "Finished Sample Count", "Model Evaluation Count"; sizes in doubles.
 * Setting "Sample Collection" sets the archive's row count; "Sample Value
 * Collection" follows with the same rows. */
int kg_mocmaes_field_size(kg_mocmaes_t h, const char *name, size_t *n);
int kg_mocmaes_get_field(kg_mocmaes_t h, const char *name, double *out, size_t n);
int kg_mocmaes_set_field(kg_mocmaes_t h, const char *name, const double *in, size_t n);
/* 5000-byte GSL states as for CMA-ES.  which: 0 Multinormal, 1 Uniform generator. */
int kg_mocmaes_get_rng(kg_mocmaes_t h, int which, void *state5000);
int kg_mocmaes_set_rng(kg_mocmaes_t h, int which, const void *state5000);
/* Diagnostics only (holds no solver state; any pointer may be NULL): windows
 * the last prepare used and the window size in blocks, the archive buffers'
 * capacity in rows, and the rank-peeling rounds the last multi-workgroup sort
 * counted (0 after a one-workgroup sort).  The tests read them to see that
 * the relaunch, growth and multi-workgroup paths ran. */
int kg_mocmaes_diagnostics(kg_mocmaes_t h, size_t *last_windows, size_t *window_blocks, size_t *archive_capacity,
                           size_t *last_rounds);
/* stage timing as kg_cmaes_profile; stages "draw", "evaluate", "sort",
 * "update", "parents", "statistics" */
int kg_mocmaes_profile(kg_mocmaes_t h, int enable);
int kg_mocmaes_profile_read(kg_mocmaes_t h, const char *stage, double *ms_total, size_t *count);

/* ------------------------------------------------------------ testing */
/* Host reference of the mt19937 jump-ahead the chunked device producer
 * uses: out = the 624 untempered words `distance` positions after window624
 * (window624 = 624 consecutive untempered words of a GSL mt19937 stream,
 * not starting at the seeding word 0).  Runs on the host, no device needed. */
int kg_debug_mt_jump(const uint32_t *window624, uint64_t distance, uint32_t *out624);
/* One device mt19937 stream (csrc/kg_rng.hpp MtStream: the generator every
 * solver draws its normals and uniforms from) with no solver around it.  Each
 * entry is the MtStream call of its name on the handle's stream, waited for;
 * host arrays travel through device buffers the handle owns.
 * open: a ring for capacity_words beyond the current block on `device`, then
 * the import of a 5000-byte GSL state (nonzero return for an mti outside
 * [0, 624]).  KORALI_AMD_MT_PARALLEL_MIN / _CHUNK_LOG2 / _CHUNK_PARTS choose
 * the producer as they do for the solvers.  import: the same import again on
 * the used handle. */
typedef struct kg_debug_mt_s *kg_debug_mt_t;
int kg_debug_mt_open(int device, size_t capacity_words, const void *state5000, kg_debug_mt_t *out);
int kg_debug_mt_close(kg_debug_mt_t h);
int kg_debug_mt_import(kg_debug_mt_t h, const void *state5000);
/* the polar count and scatter passes' workgroups for a draw of M normals */
int kg_debug_mt_count_blocks(kg_debug_mt_t h, size_t M, size_t *count_blocks);
/* M gsl_ran_gaussian(1) normals, not consumed: normal k of [k_lo, min(k_hi, M))
 * into z[k - k_lo]; z (z_len doubles, at least the window) is uploaded first
 * and read back whole, so entries the pass does not write keep the caller's
 * values.  block_end (NULL, or M / block_len entries, uploaded and read back
 * the same way): the attempt index of normal (b+1) block_len - 1; it stays
 * on the device for the consume entries.  *count_blocks (may be NULL) as
 * kg_debug_mt_count_blocks, the grid this draw launched. */
int kg_debug_mt_polar_normals(kg_debug_mt_t h, size_t M, size_t block_len, size_t k_lo, size_t k_hi, double *z,
                              size_t z_len, unsigned long long *block_end, size_t *count_blocks);
/* Advance past `used` normals of the last draw: through its block_end
 * (use_block_end, `used` a multiple of that draw's block_len) or through the
 * draw's own record of normal M - 1 (used == M).  _dev: used_blocks blocks of
 * block_len normals, the count read from device memory. */
int kg_debug_mt_consume_normals(kg_debug_mt_t h, size_t used, size_t block_len, int use_block_end);
int kg_debug_mt_consume_normals_dev(kg_debug_mt_t h, unsigned long long used_blocks, size_t block_len);
/* M gsl_rng_uniform draws, consumed (uniforms) or not (peek_uniforms), and the
 * consumption of `words` words, the count read from device memory. */
int kg_debug_mt_uniforms(kg_debug_mt_t h, size_t M, double *u);
int kg_debug_mt_peek_uniforms(kg_debug_mt_t h, size_t M, double *u);
int kg_debug_mt_consume_words_dev(kg_debug_mt_t h, unsigned long long words);
/* The side stream: the producer for M normals (prefetch); the polar pass on
 * it into the handle's buffer, uploaded from z (z_len >= M) first, *launched
 * = 0 when no side stream exists yet (polar_normals_ahead); join, then the
 * buffer's first z_len doubles into z (NULL: the join alone). */
int kg_debug_mt_prefetch(kg_debug_mt_t h, size_t M);
int kg_debug_mt_polar_normals_ahead(kg_debug_mt_t h, size_t M, size_t block_len, const double *z, size_t z_len,
                                    int *launched);
int kg_debug_mt_join(kg_debug_mt_t h, double *z, size_t z_len);
int kg_debug_mt_export_gsl(kg_debug_mt_t h, void *state5000);
/* The device's StreamState: out7 = lo, pos, hi, nzero, errors (KG_ERR_* bits:
 * 2 generator underrun, 8 zero-word list full), last_attempt, total_normals;
 * *ring_words (may be NULL) the ring's size in words. */
int kg_debug_mt_state(kg_debug_mt_t h, unsigned long long *out7, unsigned long long *ring_words);
/* The host core's tridiagonalisation (phase A of CMAES::eigen,
 * CMAES.cpp.base:896-938 → gsl_linalg_symmtd_decomp, run every generation
 * from prepareGeneration :441) on a given matrix: C row-major N x N (lower
 * triangle read); H (N x N): row i < N-2 = column i below the diagonal
 * (H[i][0] = sd[i], the reflector's entries after it), tau (N), d (N),
 * sd (N).  Runs on the host, no device needed. */
int kg_debug_host_tridiag(size_t N, const double *C, double *H, double *tau, double *d, double *sd);
/* The same, `count` matrices in a row on one workspace and one pool of helper
 * threads, as the solver decomposes generation after generation: matrix k at
 * C + k N N, its outputs at H + k N N, tau + k N, d + k N, sd + k N. */
int kg_debug_host_tridiag_seq(size_t N, size_t count, const double *C, double *H, double *tau, double *d, double *sd);
/* The host core's Givens chase (phase C of the eigendecomposition, GSL
 * eigen/symmv.c + qrstep.c as kg_eigen.hip's qr_chase) on the tridiagonal
 * (d[N], sd[N-1]) reps times: sorted eigenvalues (ABS_ASC) and their
 * permutation, counts[3] = {QR steps, rotations, overflow}, the first cs_cap
 * rotation values (c, s pairs) and the mean wall time per chase.  fused
 * selects the sweep with the chop test folded in.  CPU only (no device code). */
int kg_debug_host_chase(size_t N, const double *d, const double *sd, int fused, size_t reps, double *eval, int *perm,
                        double *cs, size_t cs_cap, int *counts, double *ns_per_chase);
/* The workgroup Cholesky every solver shares (gsl_linalg_cholesky_decomp1 in
 * gslcblas order, csrc/kg_gsl.hpp) on `device`: in, out row-major N x N
 * (1 <= N <= 1024).  out's lower triangle and diagonal hold the factor, or
 * GSL's partial factor when a pivot was not positive (*failed = 1); its
 * strict upper triangle is in's. */
int kg_debug_cholesky(int device, size_t N, const double *in, double *out, int *failed);
/* The univariate priors' log-density (csrc/kg_gsl.hpp) on `device`: the
 * constant of distribution `kind` (enum kg_prior_kind) with parameters a, b
 * in *out_const and its getLogDensity at x[0..n) in out. */
int kg_debug_prior_logdens(int device, int kind, double a, double b, const double *x, size_t n, double *out_const,
                           double *out);
/* Host-only check of the TMCMC resampling (no device call): `reps`
 * consecutive gsl_ran_multinomial draws (K categories, N trials) from one
 * mt19937 seeded with `seed`, by the exact conditional-binomial walk
 * (n_exact) and by the interval-decided walk the handle uses (n_interval);
 * each array holds reps * K counts.  Replaces nothing in the reference
 * (TMCMC.cpp.base:303-309 draws through Multinomial::getSelections). */
int kg_debug_multinomial(uint64_t seed, size_t K, unsigned N, const double *p, size_t reps, unsigned *n_exact,
                         unsigned *n_interval);
/* The device CartPole (examples/learning/reinforcement/cartpole/_model/
 * cartpole.py: scipy dopri5 advance, restated in kg_vracer.hip) on given
 * forces: n trajectories from u0 (n x 4) at t = 0, `steps` advances each with
 * force[j * steps + k]; u_out (n x steps x 4) the state after every advance,
 * over (n x steps) 1 where the pole fell or the cart left the track, -1 where
 * the integration failed.  Runs on `device`. */
int kg_debug_cartpole(int device, const double *u0, const double *force, size_t n, size_t steps, double *u_out,
                      int *over);
/* kg_debug_cartpole from time t0[j] (NULL: 0) instead of 0, the time after
 * the last advance in t_out (n, may be NULL): one environment step at a time
 * on the device's dynamics (a host 'Environment Function' equal to the
 * CartPole kernel, tests/test_gpu_vracer_host_env.py). */
int kg_debug_cartpole_at(int device, const double *u0, const double *t0, const double *force, size_t n, size_t steps,
                         double *u_out, double *t_out, int *over);

/* --------------------------------------------------------------- TMCMC */
typedef struct kg_tmcmc_s *kg_tmcmc_t;

enum kg_likelihood { KG_LIK_GAUSSIAN = 0 }; /* -0.5*sum(x^2), model.py:32-37 */

typedef struct {
  size_t variable_count;  /* N */
  size_t population_size; /* P ("Population Size") */
  double max_chain_length;               /* "Max Chain Length" (>= 1) */
  double default_burn_in;                /* "Burn In" (TMCMC.config "Default Burn In", >= 0) */
  double target_cov;                     /* "Target Coefficient Of Variation" */
  double covariance_scaling;             /* "Covariance Scaling" */
  double min_annealing_exponent_update;  /* "Min Annealing Exponent Update" */
  double max_annealing_exponent_update;  /* "Max Annealing Exponent Update" */
  const double *prior_min;               /* N: Univariate/Uniform prior of each variable */
  const double *prior_max;               /* N */
  /* Korali draws variable d's generation-1 candidate from the distribution
   * object _k->_distributions[_variables[d]->_distributionIndex]
   * (TMCMC.cpp.base:218-220); variables that share a distribution share its
   * RNG.  prior_distribution[d] is that index (NULL: variable d uses
   * distribution d); prior_seeds[k] seeds distribution k. */
  const int *prior_distribution;         /* N or NULL */
  size_t distribution_count;             /* entries of prior_seeds (0: N) */
  const uint64_t *prior_seeds;
  uint64_t multinomial_seed, multivariate_seed, uniform_seed;
  int likelihood;                        /* enum kg_likelihood */
  int device;
  /* "Per Generation Burn In": entry k is the burn-in of generation k+2
   * (setBurnIn, TMCMC.cpp.base:781-789); NULL / 0 entries: Burn In only */
  const double *per_generation_burn_in;
  size_t per_generation_burn_in_count;
  /* chain sharding: shard_count ranks, one handle each,
   * state replicated; 0 = unsharded (kg_tmcmc_process), >= 1 = sharded
   * (the partial / exchange / finalize protocol below, also for one rank) */
  int shard_rank;
  int shard_count;
  /* "Version" (TMCMC.config): 0 TMCMC, 1 mTMCMC — gradient / Fisher
   * information proposals per chain (TMCMC.cpp.base:383-681), with the
   * reference's constraints (:48-83: Max Chain Length 1, Step Size >= 0,
   * Domain Extension Factor >= 0, Uniform priors) and this implementation's
   * (burn-in 0, unsharded, N <= 128, likelihoods set by the caller) */
  int version;
  double step_size;               /* "Step Size" (default 0.1) */
  double domain_extension_factor; /* "Domain Extension Factor" (default 0.2) */
  /* per variable, enum kg_prior_kind (prior_min / prior_max = the
   * distribution's two parameters as listed there).  Variables sharing a
   * distribution share its kind.  NULL: every prior Uniform.  mTMCMC:
   * Uniform only. */
  const int *prior_kind;
} kg_tmcmc_cfg;

enum kg_prior_kind {
  KG_PRIOR_UNIFORM = 0,     /* Minimum, Maximum (uniform.cpp.base) */
  KG_PRIOR_NORMAL = 1,      /* Mean, Standard Deviation (normal.cpp.base) */
  KG_PRIOR_EXPONENTIAL = 2, /* Location, Mean (exponential.cpp.base) */
  KG_PRIOR_LAPLACE = 3,     /* Mean, Width (laplace.cpp.base) */
  KG_PRIOR_CAUCHY = 4,      /* Location, Scale (cauchy.cpp.base) */
  KG_PRIOR_LOGNORMAL = 5    /* Mu, Sigma (logNormal.cpp.base) */
};

int kg_tmcmc_create(const kg_tmcmc_cfg *cfg, kg_tmcmc_t *out);
int kg_tmcmc_destroy(kg_tmcmc_t h);
/* one whole generation (TMCMC::runGeneration) with the builtin likelihood */
int kg_tmcmc_generation(kg_tmcmc_t h, size_t generation);
int kg_tmcmc_synchronize(kg_tmcmc_t h);
int kg_tmcmc_field_size(kg_tmcmc_t h, const char *name, size_t *n);
int kg_tmcmc_get_field(kg_tmcmc_t h, const char *name, double *out, size_t n);
int kg_tmcmc_set_field(kg_tmcmc_t h, const char *name, const double *in, size_t n);
/* which: 0 Multinomial, 1 Multivariate, 2 Uniform, 3+k prior distribution k */
int kg_tmcmc_get_rng(kg_tmcmc_t h, int which, void *state5000);
int kg_tmcmc_set_rng(kg_tmcmc_t h, int which, const void *state5000);
/* the stages of one generation:
 *   prepare  = (gen 1: setInitialConfiguration :21-105) + prepareGeneration :159-227;
 *              the first candidate of every started chain is pending evaluation
 *   evaluate = Bayesian::evaluate with the builtin likelihood (bayesian.cpp.base:24-84)
 *              of the pending candidates
 *   advance  = one step of every unfinished chain (runGeneration's WAITANY loop
 *              :112-144 + processCandidate :229-252): accept / reject, database
 *              entry past the burn-in, and the next candidate of chains with
 *              steps left, which become pending; *pending = their number.
 *              Chains run Chain Lengths[c] + Current Burn In steps, in the
 *              Sequential conduit's chain-major RNG order.
 *   process  = the remaining steps (builtin likelihood) + processGeneration :254-381 */
int kg_tmcmc_prepare(kg_tmcmc_t h, size_t generation);
int kg_tmcmc_evaluate(kg_tmcmc_t h);
int kg_tmcmc_advance(kg_tmcmc_t h, size_t generation, size_t *pending);
/* P flags: 1 where the chain's candidate awaits evaluation */
int kg_tmcmc_get_pending(kg_tmcmc_t h, unsigned char *mask);
int kg_tmcmc_process(kg_tmcmc_t h, size_t generation);
/* Chain sharding over shard_count ranks: each rank draws, evaluates and steps
 * only its contiguous share of the started chains (it counts the whole
 * Multivariate / Uniform streams, so positions stay global).  Then
 *   kg_tmcmc_process_partial  - remaining steps + packs the rank's database,
 *                               leader and candidate rows and its accepted
 *                               count into "Shard Exchange" (int64 words,
 *                               INT64_MIN where the rank owns nothing),
 *   caller                    - MAX all-reduce of "Shard Exchange" viewed as
 *                               int64 (exact bits of every owner), on the
 *                               handle's stream (kg_tmcmc_stream),
 *   kg_tmcmc_process_finalize - unpacks, then processGeneration :254-381
 *                               replicated: every rank's state stays
 *                               bit-identical to the unsharded run. */
int kg_tmcmc_process_partial(kg_tmcmc_t h, size_t generation);
int kg_tmcmc_process_finalize(kg_tmcmc_t h, size_t generation);
int kg_tmcmc_device_ptr(kg_tmcmc_t h, const char *name, void **ptr);
int kg_tmcmc_stream(kg_tmcmc_t h, void **stream);
/* host-callback likelihoods (KORALI_START/WAITANY of TMCMC::runGeneration
 * :114-144): kg_tmcmc_evaluate_prior forms the uniform log-priors of the
 * pending candidates on the device ("Chain Candidates LogPriors"; -inf prior
 * -> logLikelihood -inf, bayesian.cpp.base:56-77), then the host reads the
 * P x N candidates, runs the model for pending chains whose prior is finite
 * and hands both back with kg_tmcmc_set_evaluations (entries of chains that
 * are not pending are ignored), then calls kg_tmcmc_advance; repeat while
 * chains are pending, then kg_tmcmc_process. */
int kg_tmcmc_evaluate_prior(kg_tmcmc_t h);
int kg_tmcmc_get_candidates(kg_tmcmc_t h, double *X, size_t ld);
int kg_tmcmc_set_evaluations(kg_tmcmc_t h, const double *log_prior, const double *log_likelihood);
/* mTMCMC, generations > 1, after kg_tmcmc_set_evaluations:
 * calculateGradients + calculateProposals (TMCMC.cpp.base:383-558) from
 * every candidate's "logLikelihood Gradient" (P x N) and "Fisher
 * Information" (P x N x N, row-major), as Bayesian/Reference computes them
 * (reference.cpp.base:231-621); rows of chains whose candidate log-prior or
 * log-likelihood is not finite are not read.  Also forms the proposal
 * log-density ratios of the acceptance step (:634-677). */
int kg_tmcmc_set_gradients(kg_tmcmc_t h, const double *grad, const double *fisher);
/* The Hierarchical/Psi and Hierarchical/ThetaNew log-likelihoods as the
 * handle's builtin likelihood.  Both are sums over sample
 * databases that earlier runs left behind, no user model:
 *
 *   KG_HIER_PSI       Psi::evaluateLogLikelihood      psi.cpp.base:120-141
 *                     (+ updateConditionalPriors :110-118): group g is
 *                     sub-experiment g's "Sample Database" (rows, D columns)
 *                     and "Sample LogPrior Database" (log_prior); conditional
 *                     prior k's two parameters are variable param_index[2k],
 *                     param_index[2k+1] of the evaluated point, or
 *                     param_const[...] where the index is -1;
 *   KG_HIER_THETANEW  ThetaNew::evaluateLogLikelihood thetaNew.cpp.base:35-54:
 *                     one group, the Psi experiment's "Sample Database" (rows,
 *                     row_width columns); param_index selects database
 *                     columns; the handle has N = prior_count variables.
 *
 * logSumExp is auxiliar/math.hpp:205-225 operation for operation; log and exp
 * are the correctly rounded ones of the other likelihoods. */
enum kg_hier_mode { KG_HIER_PSI = 0, KG_HIER_THETANEW = 1, KG_HIER_THETA = 2 /* kg_tmcmc_set_hierarchical_theta */ };

typedef struct {
  int mode;                  /* enum kg_hier_mode */
  size_t prior_count;        /* D conditional priors (1..128) */
  const int *kind;           /* D, enum kg_prior_kind */
  const int *param_index;    /* 2 D: supplier of each prior's first / second parameter, or -1 */
  const double *param_const; /* 2 D: the parameter where its index is -1 */
  size_t group_count;        /* G (ThetaNew: 1) */
  const size_t *group_size;  /* G, each >= 1 */
  size_t row_width;          /* doubles per row (Psi: D) */
  const double *rows;        /* sum(group_size) x row_width, row-major, group after group */
  const double *log_prior;   /* Psi: sum(group_size); ThetaNew: not read */
} kg_tmcmc_hierarchical;

/* Copies everything to the device; after kg_tmcmc_create and before the first
 * kg_tmcmc_prepare.  From then on kg_tmcmc_evaluate, the remaining steps of
 * kg_tmcmc_process / _partial and kg_tmcmc_generation evaluate this likelihood
 * (replaces the per-sample host call of Hierarchical::evaluateLogPosterior,
 * hierarchical.cpp.base:34-55; chains with a -inf log-prior are not
 * evaluated, :39-43).  A conditional prior whose scale parameter is <= 0
 * (the distributions' updateDistribution checks) or a NaN log-posterior
 * (:51) is recorded on the device; the next call that waits for the device
 * (kg_tmcmc_prepare, _process_finalize / _process / _generation,
 * _synchronize, _get_field, _set_field, _get_rng, _hierarchical_loglik)
 * returns non-zero with the reference's message and the chain index.
 * mTMCMC handles are refused. */
int kg_tmcmc_set_hierarchical(kg_tmcmc_t h, const kg_tmcmc_hierarchical *d);
/* The same kernel on `rows` arbitrary points X (rows x N, row-major), the
 * prior not consulted and NaN results returned as they are; waits. */
int kg_tmcmc_hierarchical_loglik(kg_tmcmc_t h, const double *X, size_t rows, double *out);

/* Hierarchical/Theta (phase 3b; theta.cpp.base:59-124): the
 * posterior of one sub-experiment's parameters, informed by the Psi
 * experiment's samples.  With S (sub_rows x D) / lpS the sub-experiment's
 * "Sample Database" / "Sample LogPrior Database", Psi row i's conditional
 * priors (a_i, b_i, cn_i) as KG_HIER_THETANEW forms them, K = sub_rows and
 * M = psi_rows:
 *
 *   den_i = -log(K) + LSE_j( (0.0 + sum_k logdens_k(S[j][k]; i)) - lpS[j] )    once (:64-83)
 *   LL(x) = (subLL(x) - log(M)) + LSE_i( (0.0 + sum_k logdens_k(x[k]; i)) - den_i )   (:97-124)
 *
 * subLL is the sub-problem's own log-likelihood: the handle's builtin kernel
 * (kg_tmcmc_evaluate / _generation), or what kg_tmcmc_set_evaluations is
 * given.  Everything is computed as written, infinities and NaN included. */
typedef struct {
  size_t prior_count;         /* D conditional priors (1..128) = the handle's variable_count */
  const int *kind;            /* D, enum kg_prior_kind */
  const int *param_index;     /* 2 D: Psi database column of each prior's first / second parameter, or -1 */
  const double *param_const;  /* 2 D: the parameter where param_index is -1 */
  size_t psi_rows, psi_width; /* the Psi experiment's "Sample Database" (M x psi_width, row-major) */
  const double *psi_db;
  size_t sub_rows;            /* the sub-experiment's "Sample Database" (K x D, row-major) ... */
  const double *sub_db;
  const double *sub_log_prior; /* ... and "Sample LogPrior Database" (K) */
} kg_tmcmc_hier_theta;

/* As kg_tmcmc_set_hierarchical (same place in a handle's life, same refusals,
 * one hierarchical likelihood per handle); forms the denominators on the
 * handle's stream and waits.  A Psi row with an invalid scale parameter is
 * refused with the reference's message and the row.  From then on
 * kg_tmcmc_evaluate_prior queues the LSE term of the pending chains beside
 * the handle's stream (it depends on the candidates only, so it runs while
 * the host evaluates the models), kg_tmcmc_set_evaluations completes the
 * log-likelihoods it is given to LL(x), and kg_tmcmc_evaluate / _generation
 * do both after the builtin kernel.  A NaN log-posterior is reported as
 * kg_tmcmc_set_hierarchical describes, also by the two calls below. */
int kg_tmcmc_set_hierarchical_theta(kg_tmcmc_t h, const kg_tmcmc_hier_theta *d);
/* den (M = psi_rows doubles); waits. */
int kg_tmcmc_theta_denominators(kg_tmcmc_t h, double *out, size_t M);
/* LL of `rows` arbitrary points X (rows x D, row-major) with the sub-problem's
 * log-likelihoods sub_loglik (rows; null: 0.0), the prior not consulted and
 * NaN results returned as they are; waits. */
int kg_tmcmc_theta_loglik(kg_tmcmc_t h, const double *X, size_t rows, const double *sub_loglik, double *out);
int kg_tmcmc_profile(kg_tmcmc_t h, int enable);
int kg_tmcmc_profile_read(kg_tmcmc_t h, const char *stage, double *ms_total, size_t *count);

/* ---------------------------------------------------------------- VRACER
 * The VRACER agent with the continuous Normal
 * policy, its critic/policy network and the CartPole environment of
 * examples/learning/reinforcement/cartpole, all on the device:
 *
 *   kg_vracer_create              Agent::initialize + VRACER::initializeAgent
 *                                 agent.cpp.base:9-154, VRACER.cpp.base:10-63,
 *                                 continuous.cpp.base:9-93 (Normal transforms)
 *   kg_vracer_run_policy          VRACER::runPolicy              VRACER.cpp.base:183-205
 *   kg_vracer_environment_step    one action of every concurrent environment
 *                                 (continuous.cpp.base:95-150) + Agent::processEpisode
 *                                 of the episodes that ended (agent.cpp.base:376-572)
 *   kg_vracer_train_policy        VRACER::trainPolicy x updates  VRACER.cpp.base:65-181
 *                                 (generateMiniBatch :574-597, updateExperienceMetadata
 *                                 :599-735, DeepSupervisor::runGeneration, fAdam)
 *   kg_vracer_training_step       the body of Agent::trainingGeneration's loop
 *                                 (agent.cpp.base:176-235): environment step, then
 *                                 as many policy updates as Experiences Between
 *                                 Policy Updates allows
 *   kg_vracer_{get,set}_field / _scalar   replay memory, hyperparameters and agent
 *                                 state (the reference's serialized agent fields)
 * Float32 throughout, as the reference.  Hyperparameters are Korali's vector:
 * per layer [W (out x in, row-major), b]. */
typedef struct kg_vracer_s *kg_vracer_t;
typedef struct {
  size_t state_size, action_size;          /* Variables of Type State / Action */
  size_t hidden_size, hidden_layers;       /* Linear + Elementwise/Tanh hidden layers */
  size_t environments;                     /* Concurrent Environments */
  size_t environment_count;                /* Problem / Environment Count */
  size_t mini_batch_size;                  /* Mini Batch / Size */
  size_t replay_maximum_size, replay_start_size;   /* Experience Replay sizes */
  size_t max_episode_steps;                /* the environment's truncation length */
  double experiences_between_policy_updates;
  double discount_factor, learning_rate, importance_weight_truncation_level;
  double off_policy_cutoff_scale, off_policy_target, off_policy_annealing_rate, off_policy_refer_beta;
  int l2_regularization_enabled;
  double l2_regularization_importance;
  const double *initial_exploration_noise; /* action_size values */
  uint64_t seed;                           /* action-noise / mini-batch stream key */
  int device;
  int policy_distribution;                 /* Policy / Distribution: 0 Normal, 1 Clipped Normal */
  const double *action_lower_bounds, *action_upper_bounds;  /* action_size values (may be NULL for Normal) */
  int reward_rescaling;                    /* Reward / Rescaling / Enabled (environment_count <= 8) */
  int state_rescaling;                     /* State Rescaling / Enabled (state_size <= 8) */
  int host_environment;                    /* 1: a host 'Environment Function' feeds the steps
                                              (kg_vracer_host_*); any state_size, action_size <= 4;
                                              0: the device CartPole (4 states, 1 action) */
} kg_vracer_config;

int kg_vracer_create(const kg_vracer_config *cfg, kg_vracer_t *out);
/* A discrete agent, Agent / Discrete / dVRACER on Reinforcement Learning /
 * Discrete (replaces Discrete::initializeAgent, solver/agent/discrete/
 * discrete.cpp.base:7-13; dVRACER::initializeAgent, dVRACER.cpp.base:8-57; the
 * problem's 'Possible Actions', problem/reinforcementLearning/discrete/
 * discrete.cpp.base:7-21): `possible_actions` = K action vectors of
 * action_size components each (1 <= K <= 7, row-major in `actions`).  The
 * network's output is V, K Q-values and the inverse temperature (Identity x
 * (1 + K), Sigmoid; scale 1, shift 0); the policy is the softmax of
 * dVRACER::runPolicy (:156-222), actions are categorical draws
 * (Discrete::getAction, discrete.cpp.base:15-78), importance weights and
 * gradients those of discrete.cpp.base:80-163 and dVRACER.cpp.base:83-154.
 * cfg's policy_distribution, action bounds and initial_exploration_noise are
 * ignored.  Every other kg_vracer_* call works on either kind of handle:
 *   kg_vracer_run_policy       returns the 2 + K transformed outputs per row;
 *   kg_vracer_set_action_noise forces the next step's uniforms in [0, 1), one
 *                              per environment (n = environments);
 *   kg_vracer_test_episodes    takes the first most probable action;
 *   fields                     exp_policy / cur_policy are R x (K + 1) (q,
 *                              invT); action_index (int, R),
 *                              exp_action_probabilities and
 *                              cur_action_probabilities (R x K),
 *                              possible_actions (K x action_size); the running
 *                              episodes' episode_action_index (int) and
 *                              episode_action_probabilities (x K), environments x
 *                              max_episode_steps slots. */
int kg_vracer_create_discrete(const kg_vracer_config *cfg, size_t possible_actions,
                              const double *actions /* K x action_size */, kg_vracer_t *out);
int kg_vracer_destroy(kg_vracer_t h);
int kg_vracer_hyperparameter_count(kg_vracer_t h, size_t *n);
int kg_vracer_field_size(kg_vracer_t h, const char *name, size_t *elem_bytes, size_t *count);
int kg_vracer_get_field(kg_vracer_t h, const char *name, void *dst, size_t bytes);
int kg_vracer_set_field(kg_vracer_t h, const char *name, const void *src, size_t bytes);
int kg_vracer_get_scalar(kg_vracer_t h, const char *name, double *v);
int kg_vracer_set_scalar(kg_vracer_t h, const char *name, double v);
int kg_vracer_run_policy(kg_vracer_t h, const float *states, size_t n, float *out);
/* Use the given standard normals (environments x action_size) for the next
 * environment step's actions instead of the device stream (testing). */
int kg_vracer_set_action_noise(kg_vracer_t h, const float *noise, size_t n);
int kg_vracer_environment_step(kg_vracer_t h, size_t *new_experiences);
/* Agent::rescaleStates (agent.cpp.base:291-322): the replay memory's state
 * moments, every stored state rescaled; episodes launched from then on
 * scale their states with them.  kg_vracer_training_step calls it where the
 * reference does (agent.cpp.base:204-207). */
int kg_vracer_rescale_states(kg_vracer_t h);
int kg_vracer_train_policy(kg_vracer_t h, size_t updates);
/* the policy updates the experiences collected so far call for
 * (Agent::trainingGeneration, agent.cpp.base:201-231: State Rescaling at the
 * first update, then as many updates as Experiences Between Policy Updates
 * allows); kg_vracer_training_step = kg_vracer_environment_step + this */
int kg_vracer_train_pending(kg_vracer_t h, size_t *updates);
/* Host environments (a user 'Environment Function', run by the engine as a
 * coroutine per environment: reinforcementLearning.cpp.base:58-83,
 * :130-200, :276-340).  The device keeps the policy, the episode buffers and
 * the replay memory exactly as for the CartPole kernel; the transitions come
 * from the host:
 *   kg_vracer_host_launch   the first launch of every environment: its
 *                           initial state (E x S, raw: rescaled on the
 *                           device) and Environment Id (E);
 *   kg_vracer_host_act      the policy's action of every environment
 *                           (E x A, continuous.cpp.base:95-150), the
 *                           experience kept in the episode buffer;
 *   kg_vracer_host_feed     each environment's reward, state after the
 *                           action (E x S raw; an ended episode's last
 *                           state), termination (0 non terminal, 1 Terminal,
 *                           2 Truncated) and, for the ended ones, the next
 *                           launch's initial state (E x S) and Environment Id
 *                           (E); then Agent::processEpisode of the ended
 *                           episodes in environment order (agent.cpp.base:376-572).
 *                           Launches take sample ids in launch order. */
int kg_vracer_host_launch(kg_vracer_t h, const float *states, const int *env_ids);
int kg_vracer_host_act(kg_vracer_t h, float *actions);
int kg_vracer_host_feed(kg_vracer_t h, const float *rewards, const float *states, const int *terminations,
                        const float *next_states, const int *next_env_ids, size_t *new_experiences);
int kg_vracer_train_policy_minibatch(kg_vracer_t h, const uint32_t *sorted_ids, size_t count);
int kg_vracer_training_step(kg_vracer_t h, size_t *new_experiences, size_t *updates);
/* Agent::testingGeneration (agent.cpp.base:267-289) on the device CartPole:
 * one episode per entry, reset with seed sample_ids[j] * 1024 +
 * launch_ids[j] (env.py), actions = the policy's mode
 * (generateTestingAction, continuous.cpp.base:219-260: Normal mean, Clipped
 * Normal mean clipped), environment 0's reward, up to max_episode_steps;
 * rewards[j] = the episode's cumulative reward ("Testing Reward",
 * reinforcementLearning.cpp.base:207-255).  Uses the current
 * hyperparameters; replay memory and agent state are untouched. */
int kg_vracer_test_episodes(kg_vracer_t h, const uint64_t *sample_ids, const uint64_t *launch_ids, size_t n,
                            float *rewards);
/* The agent's whole training state in one binary file (replaces
 * Agent::serializeExperienceReplay / deserializeExperienceReplay,
 * agent.cpp.base:849-976, which write the replay memory to
 * <result path>/state.json): the replay memory, the concurrent environments'
 * episodes in flight, the policy, its Adam moments, the agent's scalars and
 * counters, plus user_bytes of the caller's own (the engine's session
 * counters).  kg_vracer_load_state needs a handle created with the same
 * configuration (the seed may differ: the saved one is restored) and
 * continues the saved run bit for bit. */
int kg_vracer_save_state(kg_vracer_t h, const char *path, const void *user, size_t user_bytes);
int kg_vracer_load_state(kg_vracer_t h, const char *path, void *user, size_t user_capacity, size_t *user_bytes);
int kg_vracer_synchronize(kg_vracer_t h);
int kg_vracer_stream(kg_vracer_t h, void **stream);
/* Stage timers (HIP events on the handle's stream): "environment_step",
 * "update", "gemm_rollout" (hidden-layer MFMA products of the rollout
 * forward), "gemm_update".  profile_read returns and resets a stage's total. */
int kg_vracer_profile(kg_vracer_t h, int enable);
int kg_vracer_profile_read(kg_vracer_t h, const char *stage, double *ms_total, size_t *count);

/* -------------------------------------------------------------- Nested */
/* Sampler/Nested (nested sampling, resampling methods Box and Ellipse),
 * Nested.cpp.base; restated in tests/nested_ref.py:
 *   kg_nested_create            Nested::setInitialConfiguration   Nested.cpp.base:59-149
 *   kg_nested_first_generation  Nested::runFirstGeneration        Nested.cpp.base:206-251
 *   kg_nested_generation        Nested::runGeneration             Nested.cpp.base:151-204
 *                               (the `while (accepted == false)` loop of :167-201) and the
 *                               Termination Criteria of Nested.config:63-83
 *   kg_nested_prepare           updateBounds :253-273 (updateBox :493-504, updateEllipse
 *                               :623-632, :685-878, mahalanobisDistance :880-897),
 *                               generateCandidates :402-443, priorTransform :275-279,
 *                               Bayesian::evaluateLogPrior bayesian.cpp.base:24-32,
 *                               logPriorWeight :366-376; generation 1: the draws of :208-210
 *   kg_nested_get_candidates / kg_nested_set_evaluations
 *                               KORALI_START / WAITANY / GET of :172-197 and :216-241
 *   kg_nested_eval_builtin      Bayesian::evaluateLogPosterior    bayesian.cpp.base:56-77
 *   kg_nested_process           Nested::processGeneration         Nested.cpp.base:297-364
 *                               (sortLiveSamplesAscending :506-516, updateDeadSamples :518-530,
 *                               updateEffectiveSamples :981-987, setBoundsVolume :378-392,
 *                               safeLogPlus auxiliar/math.hpp:165-171); generation 1: :243-250
 *   kg_nested_finalize          Nested::finalize :1017-1027 (consumeLiveSamples :532-578,
 *                               generatePosterior :580-612, safeLogMinus math.hpp:180-196)
 *   kg_nested_permutation       the std::shuffle of :584-586
 * The live set, the bounds, the candidates and both generators live on the
 * device; the evidence recurrences, the dead database and the posterior are
 * host code of this library (libm exp / log / log1p, as the reference).
 * Ties of logPriorWeight + logLikelihood rank the lower live index first.
 * Limits: 1 <= N <= 64, Ellipse N >= 3, L >= 2, B >= 1; "Multi Ellipse" is
 * not built. */
typedef struct kg_nested_s *kg_nested_t;

enum kg_nested_method { KG_NESTED_BOX = 0, KG_NESTED_ELLIPSE = 1, KG_NESTED_MULTI_ELLIPSE = 2 /* rejected */ };
/* bits of kg_nested_generation's terminated_by (Nested.config:63-83) */
enum kg_nested_termination {
  KG_NESTED_MIN_LOG_EVIDENCE_DELTA = 1,
  KG_NESTED_MAX_EFFECTIVE_SAMPLE_SIZE = 2,
  KG_NESTED_MAX_LOG_LIKELIHOOD = 4
};

typedef struct {
  size_t variable_count;            /* N */
  size_t number_live_points;        /* "Number Live Points" (L) */
  size_t batch_size;                /* "Batch Size" (B) */
  int add_live_points;              /* "Add Live Points" */
  int resampling_method;            /* enum kg_nested_method */
  size_t proposal_update_frequency; /* "Proposal Update Frequency" */
  double ellipsoidal_scaling;       /* "Ellipsoidal Scaling" */
  double min_log_evidence_delta;    /* Termination Criteria */
  double max_effective_sample_size;
  double max_log_likelihood;
  /* priors as in kg_tmcmc_cfg: the two parameters of each variable's
   * distribution and its enum kg_prior_kind (NULL: every prior Uniform) */
  const double *prior_min;
  const double *prior_max;
  const int *prior_kind;
  /* the variables' "Lower Bound" / "Upper Bound": the unit cube's image for
   * a non-Uniform prior (Nested.cpp.base:77-90); not read for Uniform ones,
   * may be NULL when every prior is Uniform */
  const double *lower_bound;
  const double *upper_bound;
  uint64_t uniform_seed, normal_seed;
  uint64_t shuffle_seed;            /* _shuffleSeed (:61) */
  int likelihood;                   /* enum kg_likelihood, or -1: set by the caller */
  size_t window_tries;              /* tries the first window of a draw holds (0: default) */
  size_t max_windows;               /* windows one draw may use before it fails (0: 4096) */
  int device;
} kg_nested_cfg;

int kg_nested_create(const kg_nested_cfg *cfg, kg_nested_t *out);
int kg_nested_destroy(kg_nested_t h);
int kg_nested_first_generation(kg_nested_t h);
/* one generation > 1 with the builtin likelihood; *terminated_by (may be
 * NULL) receives the criteria that hold afterwards */
int kg_nested_generation(kg_nested_t h, size_t generation, int *terminated_by);
/* the same in stages, for likelihoods evaluated by the caller: prepare, read
 * the transformed candidates (L rows at generation 1, B after), set their
 * log-likelihoods (-inf allowed, NaN an error), process; repeat the three
 * at the same generation until *accepted is non-zero (generation 1 always
 * accepts) */
int kg_nested_prepare(kg_nested_t h, size_t generation);
int kg_nested_get_candidates(kg_nested_t h, double *X, size_t ld);
int kg_nested_set_evaluations(kg_nested_t h, const double *loglik);
int kg_nested_eval_builtin(kg_nested_t h);
int kg_nested_process(kg_nested_t h, size_t generation, int *accepted, int *terminated_by);
int kg_nested_finalize(kg_nested_t h);
/* named state, keys as in Nested.config's Internal Settings ("Live Samples",
 * "Live LogLikelihoods", "Live LogPriors", "Live LogPrior Weights", "Live
 * Samples Rank", "Candidates", "Candidate LogLikelihoods", "Candidate
 * LogPriors", "Candidate LogPrior Weights", "Box Lower Bound", "Box Upper
 * Bound", "Ellipse Axes", "Dead Samples", "Dead LogLikelihoods", "Dead
 * LogPriors", "Dead LogPrior Weights", "Dead LogWeights", "Prior Lower
 * Bound", "Prior Width" and every scalar: "LStar", "LogEvidence", ...), the
 * rest of ellipse_t as "Ellipse Mean", "Covariance Matrix", "Ellipse Inverse
 * Covariance", "Ellipse Determinant", "Ellipse Volume", the results
 * "Posterior Samples Database", "Posterior Samples LogPrior Database" and
 * "Posterior Samples LogLikelihood Database", and "Model Evaluation Count";
 * counts and ranks travel as doubles.  Setting "Dead Samples" sets the
 * database's row count; the other dead fields follow with the same rows. */
int kg_nested_field_size(kg_nested_t h, const char *name, size_t *n);
int kg_nested_get_field(kg_nested_t h, const char *name, double *out, size_t n);
int kg_nested_set_field(kg_nested_t h, const char *name, const double *in, size_t n);
/* 5000-byte GSL states.  which: 0 Normal, 1 Uniform generator. */
int kg_nested_get_rng(kg_nested_t h, int which, void *state5000);
int kg_nested_set_rng(kg_nested_t h, int which, const void *state5000);
/* Diagnostics only (any pointer may be NULL): windows and tries the last
 * candidate draw used, and the current window size in tries. */
int kg_nested_diagnostics(kg_nested_t h, size_t *last_windows, size_t *last_tries, size_t *window_tries);
/* stage timing as kg_cmaes_profile; stages "bounds", "draw", "evaluate", "select" */
int kg_nested_profile(kg_nested_t h, int enable);
int kg_nested_profile_read(kg_nested_t h, const char *stage, double *ms_total, size_t *count);
int kg_nested_synchronize(kg_nested_t h); /* waits and reports device-side errors */
/* out[0..n) = iota(n) after std::shuffle(..., std::default_random_engine(seed))
 * (Nested.cpp.base:584-586).  Host only. */
int kg_nested_permutation(uint64_t seed, size_t n, size_t *out);

/* ---------------------------------------------------------------- MCMC */
/* Sampler/MCMC (Metropolis-Hastings with delayed rejection and adaptive
 * sampling, one chain), MCMC.cpp.base; restated in tests/mcmc_ref.py:
 *   kg_mcmc_create          MCMC::setInitialConfiguration            MCMC.cpp.base:19-54
 *   kg_mcmc_run             MCMC::runGeneration :56-101, `count` times in one or a few
 *                           launches (generateCandidate :170-185, recursiveAlpha :134-168,
 *                           updateState :187-219, choleskyDecomp :103-132), and the
 *                           Termination Criteria "Max Samples" (MCMC.config:44-52) and
 *                           "Max Model Evaluations"
 *   kg_mcmc_propose         generateCandidate(level)                 :64, :170-185
 *   kg_mcmc_get_candidate   the sample's "Parameters"                :69
 *   kg_mcmc_decide          KORALI_GET of logP(x), recursiveAlpha, the accept test :76-90
 *   kg_mcmc_end_generation  the database push, updateState, _chainLength++ :93-100
 *   kg_mcmc_database        _sampleDatabase / _sampleEvaluationDatabase
 * The whole state and both generators live on the device.  exp is the
 * correctly rounded exp_cr.  recursiveAlpha is a table over the contiguous
 * sub-paths of (leader, candidate 0, ..., candidate level) instead of a
 * recursion; a call that returns early on a zero numerator still reports the
 * denominator the rest of the function would have formed (the reference
 * leaves it uninitialised and reads it one level later).
 * Limits: 1 <= N <= 64, 1 <= Rejection Levels <= 8, Max Samples * N <= 2^27. */
typedef struct kg_mcmc_s *kg_mcmc_t;

enum kg_mcmc_probability {
  KG_MCMC_HOST = 0,    /* the caller supplies logP(x) (with priors: the log-likelihood) */
  KG_MCMC_GAUSSIAN = 1 /* -0.5 * sum_d x_d^2, squares as x * x, d ascending */
};
/* why kg_mcmc_run returned (bits) */
enum kg_mcmc_stop {
  KG_MCMC_MAX_SAMPLES = 1,          /* the database holds max_samples rows */
  KG_MCMC_MAX_MODEL_EVALUATIONS = 2 /* "Model Evaluation Count" reached the given maximum */
};

typedef struct {
  size_t variable_count;           /* N */
  long long burn_in;               /* "Burn In" */
  long long leap;                  /* "Leap" */
  long long rejection_levels;      /* "Rejection Levels" (R) */
  int use_adaptive_sampling;       /* "Use Adaptive Sampling" */
  long long non_adaption_period;   /* "Non Adaption Period" */
  double chain_covariance_scaling; /* "Chain Covariance Scaling" */
  size_t max_samples;              /* Termination Criteria / "Max Samples": the database's capacity */
  const double *initial_mean;      /* the variables' "Initial Mean" (N) */
  const double *initial_sdev;      /* the variables' "Initial Standard Deviation" (N) */
  int probability_kernel;          /* enum kg_mcmc_probability */
  /* priors as in kg_tmcmc_cfg; prior_kind NULL: no priors, logP(x) is the kernel's value alone */
  const double *prior_min;
  const double *prior_max;
  const int *prior_kind;
  uint64_t normal_seed, uniform_seed;
  size_t window_candidates; /* candidates (N^2 normals and one uniform each) one launch's stream
                               windows hold (0: default); grown to R if smaller */
  int device;
} kg_mcmc_cfg;

int kg_mcmc_create(const kg_mcmc_cfg *cfg, kg_mcmc_t *out);
int kg_mcmc_destroy(kg_mcmc_t h);
/* Builtin kernel: up to `count` whole generations first_generation,
 * first_generation + 1, ... with no host round trip inside a stream window.
 * Stops before a generation when the database is full and after the one in
 * which "Model Evaluation Count" reaches max_model_evaluations (0: no limit).
 * *done (may be NULL) receives the generations completed, *stopped_by (may be
 * NULL) the enum kg_mcmc_stop bits that hold afterwards. */
int kg_mcmc_run(kg_mcmc_t h, size_t first_generation, size_t count, size_t max_model_evaluations, size_t *done,
                int *stopped_by);
/* The same one level at a time, for probabilities evaluated by the caller:
 * for level = 0, 1, ... until *accepted or level == R - 1: propose, read the
 * candidate, decide with its logP(x) (NaN is an error; ignored with a builtin
 * kernel, may then be passed as 0); then end_generation. */
int kg_mcmc_propose(kg_mcmc_t h, size_t level);
int kg_mcmc_get_candidate(kg_mcmc_t h, double *x);
int kg_mcmc_decide(kg_mcmc_t h, size_t level, double logp, int *accepted);
int kg_mcmc_end_generation(kg_mcmc_t h, size_t generation);
/* the database: X (rows x N, may be NULL), logp (rows, may be NULL); *rows
 * holds the capacity of X / logp in rows on entry and the row count on return */
int kg_mcmc_database(kg_mcmc_t h, double *X, double *logp, size_t *rows);
/* named state, keys as in MCMC.config's Internal Settings ("Chain Leader",
 * "Chain Leader Evaluation", "Chain Candidate", "Chain Candidates
 * Evaluations", "Cholesky Decomposition Covariance", "Cholesky Decomposition
 * Chain Covariance", "Chain Mean", "Chain Covariance", "Chain Covariance
 * Placeholder", "Acceptance Rate", "Acceptance Count", "Proposed Sample
 * Count", "Chain Length", "Sample Database", "Sample Evaluation Database"),
 * "Model Evaluation Count" and "Cholesky Failures" (how often the reference
 * would have warned and kept the old factor); counts travel as doubles.
 * Setting "Sample Database" sets the row count; "Sample Evaluation Database"
 * follows with the same rows. */
int kg_mcmc_field_size(kg_mcmc_t h, const char *name, size_t *n);
int kg_mcmc_get_field(kg_mcmc_t h, const char *name, double *out, size_t n);
int kg_mcmc_set_field(kg_mcmc_t h, const char *name, const double *in, size_t n);
/* 5000-byte GSL states.  which: 0 Normal, 1 Uniform generator. */
int kg_mcmc_get_rng(kg_mcmc_t h, int which, void *state5000);
int kg_mcmc_set_rng(kg_mcmc_t h, int which, const void *state5000);
/* Diagnostics only (any pointer may be NULL): the launches the last
 * kg_mcmc_run used, how many of them followed an exhausted stream window,
 * and the window size in candidates. */
int kg_mcmc_diagnostics(kg_mcmc_t h, size_t *last_windows, size_t *last_relaunches, size_t *window_candidates);
/* stage timing as kg_cmaes_profile; stages "window", "chain", "consume" */
int kg_mcmc_profile(kg_mcmc_t h, int enable);
int kg_mcmc_profile_read(kg_mcmc_t h, const char *stage, double *ms_total, size_t *count);
int kg_mcmc_synchronize(kg_mcmc_t h); /* waits and reports device-side errors */

/* ------------------------------------------------------- DeepSupervisor
 * Learner/DeepSupervisor on a Supervised Learning problem (feed-forward,
 * float32, one timestep), the whole training step on the device:
 *
 *   kg_supervisor_create            DeepSupervisor::initialize  deepSupervisor.cpp.base:9-95
 *                                   (NeuralNetwork::initialize neuralNetwork.cpp.base:14-160:
 *                                    the layer pipelines of both batch sizes)
 *   kg_supervisor_set_training_data the problem's _inputData / _solutionData
 *                                   (supervisedLearning.cpp.base:18-48 checks them)
 *   kg_supervisor_train             DeepSupervisor::runGeneration's step loop :106-160
 *                                   (Linear forward / backward linear.cpp.base:219-232,
 *                                    :284-292, :337-350; Activation activation.cpp.base:147-209,
 *                                    :270-314; Output output.cpp.base:115-232; the L2 term
 *                                    :147-153; fAdam.cpp:64-91, fAdaBelief.cpp:25-53,
 *                                    fMadGrad.cpp:54-74, fRMSProp.cpp:52-69, fAdagrad.cpp:38-54)
 *   kg_supervisor_forward           DeepSupervisor::getEvaluation :177-187
 *   kg_supervisor_backward_direct   NeuralNetwork::backward on given output gradients
 *                                   (the "Direct Gradient" loss, :140-141)
 *   kg_supervisor_{get,set}_field   getHyperparameters / setHyperparameters :163-175,
 *                                   the optimizer's vectors, each layer's values
 *
 * Layers are numbered as the reference numbers them: 0 is the input, then the
 * given layers, the Output layer last.  Hyperparameters and their gradient are
 * one float vector each in the reference's layout, [W (OC x IC), b] per Linear
 * layer.  The dense products run on the FP32 matrix cores; every reduction has
 * a fixed order (no floating-point atomics): equal states give equal bits. */
typedef struct kg_supervisor_s *kg_supervisor_t;
enum kg_supervisor_layer_type { KG_SV_LINEAR = 0, KG_SV_ACTIVATION = 1 };
enum kg_supervisor_function {
  KG_SV_TANH = 0,     /* Elementwise/Tanh */
  KG_SV_RELU = 1,     /* Elementwise/ReLU (alpha: the negative slope) */
  KG_SV_LOGISTIC = 2, /* Elementwise/Logistic */
  KG_SV_SOFTRELU = 3, /* Elementwise/SoftReLU */
  KG_SV_SOFTSIGN = 4, /* Elementwise/SoftSign */
  KG_SV_ELINEAR = 5,  /* Elementwise/Linear (alpha x + beta) */
  KG_SV_LOG = 6,      /* Elementwise/Log */
  KG_SV_SOFTMAX = 7   /* Softmax (backward: the diagonal term, activation.cpp.base:311-313) */
};
enum kg_supervisor_mask { KG_SV_IDENTITY = 0, KG_SV_ABSOLUTE = 1, KG_SV_SOFTPLUS = 2, KG_SV_MASK_TANH = 3, KG_SV_SIGMOID = 4 };
enum kg_supervisor_optimizer { KG_SV_ADAM = 0, KG_SV_ADABELIEF = 1, KG_SV_MADGRAD = 2, KG_SV_RMSPROP = 3, KG_SV_ADAGRAD = 4 };
enum kg_supervisor_loss { KG_SV_MEAN_SQUARED_ERROR = 0, KG_SV_DIRECT_GRADIENT = 1 };
typedef struct {
  int type;               /* enum kg_supervisor_layer_type */
  size_t output_channels; /* Linear: >= 1 */
  int function;           /* Activation: enum kg_supervisor_function */
  float alpha, beta;      /* Activation */
} kg_supervisor_layer;
typedef struct {
  size_t input_size, solution_size;                 /* Problem: Input / Size, Solution / Size */
  size_t training_batch_size, inference_batch_size; /* Problem: the two batch sizes (>= 1) */
  size_t layer_count;                               /* the hidden layers, the last Linear (solution_size
                                                       channels) and the output activation, if any */
  const kg_supervisor_layer *layers;
  const float *output_scale, *output_shift; /* Output Layer: Scale, Shift (solution_size values, or NULL) */
  const int *output_mask;                   /* Output Layer: Transformation Mask (enum kg_supervisor_mask, or NULL) */
  int optimizer;                            /* enum kg_supervisor_optimizer */
  int loss;                                 /* enum kg_supervisor_loss */
  float learning_rate;
  int l2_enabled;
  float l2_importance; /* as the solver holds it (the generated parser truncates it to an integer) */
  int device;
} kg_supervisor_config;

/* Limits, checked here with messages: every size >= 1, every layer width and
 * batch size below 2^31, an Activation's width is its predecessor's, the last
 * layer's width is solution_size. */
int kg_supervisor_create(const kg_supervisor_config *cfg, kg_supervisor_t *out);
int kg_supervisor_destroy(kg_supervisor_t h);
int kg_supervisor_hyperparameter_count(kg_supervisor_t h, size_t *n);
/* X: training_batch_size x input_size, S: training_batch_size x solution_size (host, row-major) */
int kg_supervisor_set_training_data(kg_supervisor_t h, const float *X, const float *S);
/* `steps` optimisation steps enqueued back to back; the loss (sum g^2 / (2 N),
 * float, :132-136) of the last step is read once, after it.  Direct Gradient:
 * the solution data are the output gradients of the last forward pass of
 * training_batch_size rows (an error if there was none); *loss is left alone. */
int kg_supervisor_train(kg_supervisor_t h, size_t steps, float *loss);
/* rows must be one of the two batch sizes (neuralNetwork.cpp.base:344-360);
 * out: rows x solution_size */
int kg_supervisor_forward(kg_supervisor_t h, const float *X, size_t rows, float *out);
/* backward of G (training_batch_size x solution_size) through the last forward
 * pass of that size; fills the hyperparameter gradient, no optimizer step */
int kg_supervisor_backward_direct(kg_supervisor_t h, const float *G);
/* Fields (float): "hyperparameters", "gradient"; the optimizer's vectors
 * ("first_moment", "second_moment" | "first_moment", "second_central_moment" |
 * "s", "v", "z" | "r", "v" | "s"); "training_input", "training_solution";
 * "output:<layer>" / "inference_output:<layer>" (a layer's values, batch x
 * width; layer 0: the input of the last pass) and "output_gradient:<layer>"
 * (the gradient with respect to a Linear layer's values).
 * Scalars: "learning_rate", "current_loss", "beta1_pow", "beta2_pow",
 * "model_evaluation_count" (settable); "layer_count", "tile", "k_step",
 * "weight_gradient_splits:<layer>", "weight_gradient_chunk:<layer>". */
int kg_supervisor_field_size(kg_supervisor_t h, const char *name, size_t *elem_bytes, size_t *count);
int kg_supervisor_get_field(kg_supervisor_t h, const char *name, void *dst, size_t bytes);
int kg_supervisor_set_field(kg_supervisor_t h, const char *name, const void *src, size_t bytes);
int kg_supervisor_get_scalar(kg_supervisor_t h, const char *name, double *value);
int kg_supervisor_set_scalar(kg_supervisor_t h, const char *name, double value);
int kg_supervisor_synchronize(kg_supervisor_t h);
/* Stage timers (HIP events; a profiled step waits for each stage): "forward",
 * "data_gradient", "weight_gradient", "optimizer", "other".  profile_read
 * returns and resets a stage's total. */
int kg_supervisor_profile(kg_supervisor_t h, int enable);
int kg_supervisor_profile_read(kg_supervisor_t h, const char *stage, double *ms_total, size_t *count);

#ifdef __cplusplus
}
#endif
#endif /* KORALI_AMD_H */
