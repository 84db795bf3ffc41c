"""Plain Python restatement of the reference's Metropolis sampler
(source/modules/solver/sampler/MCMC/MCMC.cpp.base, with delayed rejection and
adaptive sampling): the oracle of the MCMC tests.  IEEE double arithmetic in
the reference's order, one rounding per operation.

The generators are the oracle's GSL mt19937 (kr_rng_get, kr_ran_gaussian_n),
the Cholesky factor its kr_cholesky (gsl_linalg_cholesky_decomp1's Level-2
form), the priors' logarithms its kr_log_cr.  `exp` selects what recursiveAlpha
takes its exponentials from: "cr" is the oracle's correctly rounded kr_exp_cr
(what the device computes), "libm" is math.exp (what the reference computes).

logp: "gaussian" (-0.5 * sum x_d^2, squares as x * x, d ascending) or a Python
callable of the parameter list.  With priors (prior_kinds given) it is the
log-likelihood: logP = logPrior + logLikelihood, and a -inf prior skips it.
"""
import gzip
import json
import math
import os

import numpy as np

from oracle import refcpu
from nested_ref import KINDS, _lib, exp_cr, log_cr

INF = float("inf")
NAN = float("nan")

COUNTS = ["Acceptance Count", "Proposed Sample Count", "Chain Length", "Model Evaluation Count", "Cholesky Failures"]
SCALARS = COUNTS + ["Acceptance Rate", "Chain Leader Evaluation"]
VECTORS = ["Chain Leader", "Chain Candidate", "Chain Candidates Evaluations", "Chain Mean", "Chain Covariance",
           "Chain Covariance Placeholder", "Cholesky Decomposition Covariance",
           "Cholesky Decomposition Chain Covariance"]
DATABASE = ["Sample Database", "Sample Evaluation Database"]
FIELDS = SCALARS + VECTORS + DATABASE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcmc_golden.json.gz")


def load_golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def exp_libm(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def div(a, b):
    """IEEE a / b (Python raises where C gives inf or NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def min1(x):
    """std::min(1.0, x): (x < 1.0) ? x : 1.0, so NaN gives 1.0"""
    return x if x < 1.0 else 1.0


def recursive_alpha(exp, leader, ll, n):
    """recursiveAlpha (:134-168) -> (alpha, denominator); ll[0..n] are read.
    The reference's early `numerator == 0.0` return leaves its caller's
    denominatorStar uninitialised, and the next level reads it (:163-164).
    Pinned here: such a call still reports the denominator the rest of the
    function would have formed."""
    if n == 0:
        return min1(exp(ll[0] - leader)), exp(leader)
    rev = [ll[n - 1 - i] for i in range(n)]
    numerator = exp(ll[n])
    for i in range(n):
        a, _ = recursive_alpha(exp, ll[n], rev, i)
        numerator *= (1.0 - a)
    a, den_star = recursive_alpha(exp, leader, ll, n - 1)
    denominator = den_star * (1.0 - a)
    if numerator == 0.0:
        return 0.0, denominator
    return min1(div(numerator, denominator)), denominator


def table_alpha(exp, y, level):
    """The same value without recursion, as the device forms it: y[0] is the
    leader's evaluation, y[j + 1] candidate j's.  Every call of the recursion
    is the alpha of a contiguous sub-path of y walked up (a -> b, a < b: fa,
    fd) or down from the newest entry (top -> a: ra, rd)."""
    E = [exp(v) for v in y]
    fa, fd = {}, {}
    for n in range(level + 1):
        top = n + 1
        ra, rd = {}, {}
        for a in range(n, 0, -1):
            if a == n:
                rd[a], ra[a] = E[top], min1(exp(y[a] - y[top]))
            else:
                num = E[a]
                for b in range(a + 1, n + 1):
                    num *= (1.0 - fa[a, b])
                rd[a] = rd[a + 1] * (1.0 - ra[a + 1])
                ra[a] = 0.0 if num == 0.0 else min1(div(num, rd[a]))
        for a in range(n, -1, -1):
            if a == n:
                fd[a, top], fa[a, top] = E[a], min1(exp(y[top] - y[a]))
            else:
                num = E[top]
                for b in range(n, a, -1):
                    num *= (1.0 - ra[b])
                fd[a, top] = fd[a, top - 1] * (1.0 - fa[a, top - 1])
                fa[a, top] = 0.0 if num == 0.0 else min1(div(num, fd[a, top]))
    return fa[0, level + 1]


class McmcRef:
    def __init__(self, N, initial_mean, initial_sd, burn_in=0, leap=1, rejection_levels=1, adaptive=False,
                 non_adaption_period=0, scaling=1.0, max_samples=5000, normal_seed=0, uniform_seed=0,
                 logp="gaussian", prior_kinds=None, prior_min=None, prior_max=None, exp="cr"):
        _lib()
        self.N, self.R = int(N), int(rejection_levels)
        # :23-27
        if scaling <= 0.0:
            raise ValueError("Chain Covariance Scaling must be larger 0.0 (is %f).\n" % scaling)
        if leap < 1:
            raise ValueError("Leap must be larger 0 (is %d).\n" % leap)
        if rejection_levels < 1:
            raise ValueError("Rejection Levels must be larger 0 (is %d).\n" % rejection_levels)
        self.burn_in, self.leap, self.adaptive = int(burn_in), int(leap), bool(adaptive)
        self.nap, self.scaling, self.max_samples = int(non_adaption_period), float(scaling), int(max_samples)
        self.exp = {"cr": exp_cr, "libm": exp_libm}[exp]
        self.logp = logp
        N, R = self.N, self.R
        bc = lambda v: [float(x) for x in np.broadcast_to(np.asarray(v, dtype=np.float64), (N,))]
        self.kinds = None
        if prior_kinds is not None:
            self.kinds = [KINDS[k.lower()] if isinstance(k, str) else int(k) for k in prior_kinds]
            self.pmin, self.pmax = bc(prior_min), bc(prior_max)
            pi = 3.14159265358979323846
            self.cst = []
            for d in range(N):
                k, a, b = self.kinds[d], self.pmin[d], self.pmax[d]
                self.cst.append(-0.5 * log_cr(2 * pi) - log_cr(b) if k in (1, 5) else -log_cr(b) if k == 2 else
                                -log_cr(2. * b) if k == 3 else -log_cr(b * pi) if k == 4 else -log_cr(b - a))
        self.normal = refcpu.Rng(seed=int(normal_seed))
        self.uniform = refcpu.Rng(seed=int(uniform_seed))
        # setInitialConfiguration (:29-53)
        self.cand = np.zeros((R, N))
        self.cand_eval = np.zeros(R)
        self.chol = np.zeros((N, N))
        self.chol_chain = np.zeros((N, N))
        self.leader = np.array(bc(initial_mean))
        self.chol[np.diag_indices(N)] = bc(initial_sd)
        self.mean = np.zeros(N)
        self.cov = np.zeros((N, N))
        self.placeholder = np.zeros((N, N))
        self.accept = self.proposed = self.length = self.evals = self.chol_failures = 0
        self.leader_eval = -INF
        self.rate = 1.0
        self.db, self.db_eval = [], []
        self.generation = 0

    # ------------------------------------------------------------ generators
    def _normals(self, n):
        import ctypes as C
        out = np.empty(n)
        _lib().kr_ran_gaussian_n(self.normal.ptr, n, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out

    def _uniform(self):
        return _lib().kr_rng_get(self.uniform.ptr) / 4294967296.0

    # ------------------------------------------------------------ evaluation
    def _logdens(self, d, x):
        k, a, b, c = self.kinds[d], self.pmin[d], self.pmax[d], self.cst[d]
        if k == 1:
            z = (x - a) / b
            return c - 0.5 * z * z
        if k == 2:
            y = x - a
            return -INF if y < 0 else c - y / b
        if k == 3:
            return c - abs(x - a) / b
        if k == 4:
            y = x - a
            return c - log_cr(1. + y * y / (b * b))
        if k == 5:
            if x <= 0:
                return -INF
            lx = log_cr(x)
            z = (lx - a) / b
            return c - lx - 0.5 * z * z
        return c if a <= x <= b else -INF

    def _model(self, x):
        if self.logp == "gaussian":
            ss = 0.0
            for v in x:
                ss += v * v
            return -0.5 * ss
        return float(self.logp(list(x)))

    def evaluate(self, x):
        x = [float(v) for v in x]
        if self.kinds is None:
            return self._model(x)
        lp = 0.0
        for d in range(self.N):
            lp += self._logdens(d, x[d])
        if lp == -INF:
            return -INF
        return lp + self._model(x)

    # ------------------------------------------------------------ the chain
    def generate_candidate(self, i):
        """:170-185"""
        N = self.N
        self.proposed += 1
        self.cand[i] = self.leader if i == 0 else self.cand[i - 1]
        L = self.chol if (not self.adaptive or len(self.db) <= self.nap + self.burn_in) else self.chol_chain
        z = self._normals(N * N).reshape(N, N)  # d-major, e-minor, the factor's zeros included
        c = self.cand[i].copy()
        for e in range(N):  # every row's add chain in e order, one rounding per product and per sum
            c = c + L[:, e] * z[:, e]
        self.cand[i] = c

    def step(self):
        """runGeneration (:56-101)"""
        self.generation += 1
        accepted = False
        i = 0
        while i < self.R and not accepted:
            self.generate_candidate(i)
            self.evals += 1
            self.cand_eval[i] = self.evaluate(self.cand[i])
            alpha, _ = recursive_alpha(self.exp, self.leader_eval, [float(v) for v in self.cand_eval], i)
            if alpha == 1.0 or alpha > self._uniform():
                self.accept += 1
                accepted = True
                self.leader_eval = float(self.cand_eval[i])
                self.leader = self.cand[i].copy()
            i += 1
        if self.length >= self.burn_in and self.generation % self.leap == 0:
            self.db.append(self.leader.copy())
            self.db_eval.append(self.leader_eval)
        self.update_state()
        self.length += 1

    def update_state(self):
        """:187-219"""
        N = self.N
        self.rate = div(float(self.accept), float(self.length))
        n = len(self.db)
        if n == 0:
            return
        if n == 1:
            self.mean = self.leader.copy()
            return
        # (elementwise over the entries the reference's loops visit one by one)
        D = self.mean - self.leader  # the placeholder is formed from the old mean (:198-204)
        self.placeholder[:] = np.outer(D, D)
        self.mean = (self.mean * float(n - 1) + self.leader) / float(n)  # :207
        f, s = (n - 2.0) / (n - 1.0), self.scaling / float(n)
        P, Cv = self.placeholder, self.cov
        low = f * Cv + s * P       # :212 and :216 on the lower triangle and the diagonal
        up = f * low + s * P       # :213 reads the element :212 just wrote
        il, iu = np.tril_indices(N), np.triu_indices(N, 1)
        Cv[il] = low[il]
        Cv[iu] = up.T[iu]
        if self.adaptive and n > self.nap:
            st, F = refcpu.cholesky(Cv)
            if st:
                self.chol_failures += 1  # (the reference warns and keeps the old factor)
            else:
                il = np.tril_indices(N)
                self.chol_chain[il] = F[il]

    def run(self, generations):
        for _ in range(generations):
            self.step()

    def finished(self):
        return len(self.db) >= self.max_samples

    # ------------------------------------------------------------ fields
    def __getitem__(self, name):
        v = {"Acceptance Count": self.accept, "Proposed Sample Count": self.proposed, "Chain Length": self.length,
             "Model Evaluation Count": self.evals, "Cholesky Failures": self.chol_failures,
             "Acceptance Rate": self.rate, "Chain Leader Evaluation": self.leader_eval, "Chain Leader": self.leader,
             "Chain Candidate": self.cand, "Chain Candidates Evaluations": self.cand_eval, "Chain Mean": self.mean,
             "Chain Covariance": self.cov, "Chain Covariance Placeholder": self.placeholder,
             "Cholesky Decomposition Covariance": self.chol,
             "Cholesky Decomposition Chain Covariance": self.chol_chain,
             "Sample Database": np.array(self.db).reshape(-1), "Sample Evaluation Database": self.db_eval}[name]
        return np.asarray(v, dtype=np.float64).reshape(-1).copy()
