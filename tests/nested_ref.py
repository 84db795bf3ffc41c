"""Plain Python/NumPy restatement of the reference's nested sampler
(source/modules/solver/sampler/Nested/Nested.cpp.base), resampling methods Box
and Ellipse: the oracle of the Nested tests.  IEEE double arithmetic in the
reference's order, one rounding per operation.

What the device computes (the live set, the bounds, the candidates, the prior
terms, the builtin likelihood) takes log / exp / pow from the oracle's
correctly rounded kr_log_cr / kr_exp_cr / kr_pow_cr, the generators from its
GSL mt19937 (kr_rng_*, kr_ran_gaussian and its batched form
kr_ran_gaussian_n) and the Cholesky factor from kr_cholesky.  What the
library's host code computes (the evidence recurrences, the dead database, the
posterior) takes exp / log / log1p from math, i.e. libm, as the reference.

Pinned here, not by the reference (GSL 2.6's LU is recursive and its inverse
goes through triangular inverses; neither that source nor a recorded Nested
run is available): the LU is unblocked, right-looking, with partial pivoting
on the first maximal pivot; the inverse is formed column by column by forward
and back substitution; Gamma(N / 2) in K is the closed product, factors
ascending; ties of logPriorWeight + logLikelihood rank the lower live index
first (std::sort leaves their order unspecified).

The candidate draw evaluates tries in blocks, which changes nothing: a try
consumes a fixed amount of stream, candidate i is the i-th try inside the
unit cube, and the generators are left exactly behind the last try used.
"""
import ctypes as C
import math

import numpy as np

from oracle import refcpu

INF = float("inf")
LOWEST = -1.7976931348623157e308
MAX = 1.7976931348623157e308

KINDS = {"uniform": 0, "normal": 1, "exponential": 2, "laplace": 3, "cauchy": 4, "lognormal": 5}

SCALARS = ["Accepted Samples", "Generated Samples", "LogEvidence", "LogEvidence Var", "LogVolume", "Bound LogVolume",
           "Last Accepted", "Next Update", "Information", "LStar", "LStarOld", "LogWeight", "Expected LogShrinkage",
           "Max Evaluation", "Remaining Log Evidence", "Log Evidence Difference", "Effective Sample Size",
           "Sum Log Weights", "Sum Square Log Weights", "Number Dead Samples", "Model Evaluation Count"]
LIVE = ["Live Samples", "Live LogLikelihoods", "Live LogPriors", "Live LogPrior Weights", "Live Samples Rank"]
CANDIDATES = ["Candidates", "Candidate LogLikelihoods", "Candidate LogPriors", "Candidate LogPrior Weights"]
DEAD = ["Dead Samples", "Dead LogLikelihoods", "Dead LogPriors", "Dead LogPrior Weights", "Dead LogWeights"]
BOX = ["Box Lower Bound", "Box Upper Bound"]
ELLIPSE = ["Ellipse Mean", "Covariance Matrix", "Ellipse Inverse Covariance", "Ellipse Axes", "Ellipse Determinant",
           "Ellipse Volume"]
POSTERIOR = ["Posterior Samples Database", "Posterior Samples LogPrior Database",
             "Posterior Samples LogLikelihood Database"]


def _lib():
    L = refcpu.lib()
    if not getattr(L, "_nested_bound", False):
        for f in ("kr_log_cr", "kr_exp_cr"):
            getattr(L, f).argtypes = [C.c_double]
            getattr(L, f).restype = C.c_double
        L.kr_pow_cr.argtypes = [C.c_double, C.c_double]
        L.kr_pow_cr.restype = C.c_double
        L.kr_ran_gaussian_n.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_double)]
        L.kr_ran_gaussian_n.restype = None
        L._nested_bound = True
    return L


def log_cr(x):
    return _lib().kr_log_cr(x)


def exp_cr(x):
    return _lib().kr_exp_cr(x)


def pow_cr(x, y):
    return _lib().kr_pow_cr(x, y)


# libm, with C's results where Python raises
def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def _log(x):
    if x == 0:
        return -INF
    if x < 0 or x != x:
        return float("nan")
    return math.log(x)


def safe_log_plus(x, y):
    """auxiliar/math.hpp:165-171"""
    if x > y:
        return x + math.log1p(_exp(y - x))
    return y + math.log1p(_exp(x - y))


def safe_log_minus(x, y):
    """auxiliar/math.hpp:180-196"""
    if x - y > 12.0:
        return x
    if x > y:
        return y + _log(_exp(x - y) - 1.)
    raise ValueError("Invalid input to mathematical function 'safeLogMinus")


def gamma_half(n):
    """Gamma(n / 2), the closed product, factors ascending"""
    if n % 2 == 0:
        g = 1.0
        for k in range(1, n // 2):
            g *= float(k)
    else:
        g = math.sqrt(math.pi)
        for k in range(n // 2):
            g *= k + 0.5
    return g


def ellipse_constant(N):
    """K of :863"""
    return math.sqrt(math.pow(math.pi, float(N))) * 2. / (float(N) * gamma_half(N))


def lu_decomp(A):
    """Unblocked right-looking LU with partial pivoting, first maximal pivot.
    -> (LU, perm, signum)"""
    lu = np.array(A, dtype=np.float64)
    n = lu.shape[0]
    perm = list(range(n))
    signum = 1.0
    for j in range(n):
        col = np.abs(lu[j:, j])
        ip = j + int(np.argmax(col))  # argmax: the first maximum
        if ip != j:
            lu[[j, ip], :] = lu[[ip, j], :]
            perm[j], perm[ip] = perm[ip], perm[j]
            signum = -signum
        ajj = lu[j, j]
        if ajj != 0.0:
            lu[j + 1:, j] = lu[j + 1:, j] / ajj
            lu[j + 1:, j + 1:] = lu[j + 1:, j + 1:] - np.outer(lu[j + 1:, j], lu[j, j + 1:])
    return lu, perm, signum


def lu_det(lu, signum):
    det = signum
    for i in range(lu.shape[0]):
        det *= lu[i, i]
    return float(det)


def lu_invert(lu, perm):
    """column c = back(forward(P e_c)); all columns at once, each in its own order"""
    n = lu.shape[0]
    X = np.zeros((n, n))
    for i in range(n):
        X[i, perm[i]] = 1.0
    for i in range(1, n):
        tmp = X[i, :].copy()
        for k in range(i):
            tmp = tmp - lu[i, k] * X[k, :]
        X[i, :] = tmp
    X[n - 1, :] = X[n - 1, :] / lu[n - 1, n - 1]
    for i in range(n - 2, -1, -1):
        tmp = X[i, :].copy()
        for k in range(i + 1, n):
            tmp = tmp - lu[i, k] * X[k, :]
        X[i, :] = tmp / lu[i, i]
    return X


def cholesky_decomp1(A):
    """gsl_linalg_cholesky_decomp1: L in the lower triangle and the diagonal,
    the upper triangle keeps A"""
    st, F = refcpu.cholesky(A)
    if st:
        raise ArithmeticError("covariance of the live samples is not positive definite")
    out = np.array(A, dtype=np.float64)
    il = np.tril_indices(out.shape[0])
    out[il] = F[il]
    return out


class NestedRef:
    def __init__(self, N, L, prior_min, prior_max, batch_size=1, method="Ellipse", add_live_points=True,
                 proposal_update_frequency=1500, ellipsoidal_scaling=1.0, min_log_evidence_delta=0.01,
                 max_effective_sample_size=10e6, max_log_likelihood=10e6, prior_kinds=None, lower_bound=None,
                 upper_bound=None, uniform_seed=0, normal_seed=0, shuffle_seed=0, likelihood="gaussian",
                 block_tries=0):
        _lib()
        self.N, self.L, self.B = int(N), int(L), int(batch_size)
        self.ellipse = method.lower() == "ellipse"
        if method.lower() not in ("box", "ellipse"):
            raise ValueError("Resampling Method 'Multi Ellipse' is not restated")
        if self.ellipse and self.N < 3:
            raise ValueError("Resampling Method 'Ellipse' and 'Multi Ellipse' only suitable for problems of dim larger 2 "
                             "(use Resampling Method 'Box').")
        self.add_live_points = bool(add_live_points)
        self.frequency = int(proposal_update_frequency)
        self.scaling = float(ellipsoidal_scaling)
        self.min_delta, self.max_ess, self.max_ll = (float(min_log_evidence_delta), float(max_effective_sample_size),
                                                      float(max_log_likelihood))
        bc = lambda v: [float(x) for x in np.broadcast_to(np.asarray(v, dtype=np.float64), (self.N,))]
        self.pmin, self.pmax = bc(prior_min), bc(prior_max)
        self.kinds = [0] * self.N if prior_kinds is None else [KINDS[k.lower()] if isinstance(k, str) else int(k)
                                                               for k in prior_kinds]
        self.lower, self.width = [], []
        for d in range(self.N):  # :73-91
            if self.kinds[d] == 0:
                self.width.append(self.pmax[d] - self.pmin[d])
                self.lower.append(self.pmin[d])
            else:
                lb, ub = bc(lower_bound)[d], bc(upper_bound)[d]
                assert math.isfinite(lb) and math.isfinite(ub)
                self.width.append(ub - lb)
                self.lower.append(lb)
        pi = 3.14159265358979323846
        self.cst = []
        for d in range(self.N):
            k, a, b = self.kinds[d], self.pmin[d], self.pmax[d]
            if k in (1, 5):
                c = -0.5 * log_cr(2 * pi) - log_cr(b)
            elif k == 2:
                c = -log_cr(b)
            elif k == 3:
                c = -log_cr(2. * b)
            elif k == 4:
                c = -log_cr(b * pi)
            else:
                c = -log_cr(b - a)
            self.cst.append(c)
        self.log_width = [log_cr(w) for w in self.width]
        self.likelihood = likelihood
        self.uniform = refcpu.Rng(seed=int(uniform_seed))
        self.normal = refcpu.Rng(seed=int(normal_seed))
        self.shuffle_seed = int(shuffle_seed)
        self.block = int(block_tries) or max(2 * self.B, 16)
        self.K = ellipse_constant(self.N)
        N, L, B = self.N, self.L, self.B
        self.live = np.zeros((L, N))
        self.live_ll, self.live_lp, self.live_lpw = np.zeros(L), np.zeros(L), np.zeros(L)
        self.rank = list(range(L))
        self.cand = np.zeros((B, N))
        self.cand_ll, self.cand_lp, self.cand_lpw = np.zeros(B), np.zeros(B), np.zeros(B)
        self.box_lo, self.box_up = np.zeros(N), np.zeros(N)
        self.mean, self.cov, self.inv_cov, self.axes = np.zeros(N), np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
        self.det = self.volume = 0.0
        self.dead, self.dead_ll, self.dead_lp, self.dead_lpw, self.dead_lw = [], [], [], [], []
        self.post, self.post_lp, self.post_ll = [], [], []
        # :116-131
        self.s = {k: 0.0 for k in SCALARS}
        self.s["LogEvidence"] = LOWEST
        self.s["Sum Log Weights"] = LOWEST
        self.s["Sum Square Log Weights"] = LOWEST
        self.s["Log Evidence Difference"] = MAX
        self.s["Expected LogShrinkage"] = math.log((L + 1.) / L)
        self.s["LStar"] = self.s["LStarOld"] = LOWEST
        self.last_tries = 0
        self.last_blocks = 0

    # ------------------------------------------------------------ generators
    def _uniforms(self, n):
        g, p = _lib().kr_rng_get, self.uniform.ptr
        return np.array([g(p) for _ in range(n)], dtype=np.float64) / 4294967296.0

    def _normals(self, n):
        out = np.empty(max(n, 1))
        _lib().kr_ran_gaussian_n(self.normal.ptr, n, out.ctypes.data_as(C.POINTER(C.c_double)))
        return out[:n]

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

    def transform(self, X):
        """priorTransform (:275-279)"""
        return np.asarray(self.lower) + np.asarray(X) * np.asarray(self.width)

    def _evaluate(self, X):
        """-> theta, ll (None with a host likelihood), lp, lpw"""
        theta = self.transform(X)
        n = theta.shape[0]
        lp, lpw, ll = np.zeros(n), np.zeros(n), np.zeros(n)
        for c in range(n):
            p = w = ss = 0.0
            for d in range(self.N):
                v = float(theta[c, d])
                ld = self._logdens(d, v)
                p += ld
                w += ld
                w += self.log_width[d]
                ss += v * v
            lp[c], lpw[c] = p, w
            ll[c] = -INF if p == -INF else -0.5 * ss
        if self.likelihood != "gaussian":
            host = np.asarray(self.likelihood(theta), dtype=np.float64)
            ll = np.where(lp == -INF, -INF, host)
        return theta, ll, lp, lpw

    def _key(self, i):
        return self.live_lpw[i] + self.live_ll[i]

    def _sort(self):
        """sortLiveSamplesAscending (:506-516); a stable sort: ties keep the lower index first"""
        keys = self.live_lpw + self.live_ll
        self.rank = sorted(range(self.L), key=lambda i: keys[i])

    # ------------------------------------------------------ first generation
    def first_generation(self):
        """:206-251"""
        L, N = self.L, self.N
        self.live = self._uniforms(L * N).reshape(L, N)
        _, self.live_ll, self.live_lp, self.live_lpw = self._evaluate(self.live)
        self.s["Model Evaluation Count"] += L
        self.s["Generated Samples"] += L
        self._sort()
        k = self._key(self.rank[0])
        if math.isfinite(k):
            self.s["LStar"] = float(k)
        self.s["Max Evaluation"] = float(self._key(self.rank[-1]))

    # ---------------------------------------------------------------- bounds
    def update_bounds(self):
        """:253-273 (the Box method holds no ellipse: it updates on every call)"""
        if self.ellipse and self.s["Generated Samples"] < self.s["Next Update"]:
            return
        self.s["Next Update"] += self.frequency
        if not self.ellipse:
            self.box_lo = self.live.min(axis=0)
            self.box_up = self.live.max(axis=0)
            return
        N, L = self.N, self.L
        m = np.zeros(N)
        for i in range(L):
            m = m + self.live[i]
        self.mean = m / float(L)
        dif = self.live - self.mean
        weight = 1. / (L - 1.)
        if L <= N:
            c = np.zeros(N)
            for k in range(L):
                c = c + dif[k] * dif[k]
            self.cov = np.diag(weight * c)
            self.inv_cov = np.diag(1. / (weight * c))
        else:
            c = np.zeros((N, N))
            for k in range(L):
                c = c + np.outer(dif[k], dif[k])
            c = weight * c
            self.cov = np.triu(c) + np.triu(c, 1).T
        lu, perm, signum = lu_decomp(self.cov)
        if L > N:
            self.inv_cov = lu_invert(lu, perm)
        det = lu_det(lu, signum)
        axes = cholesky_decomp1(self.cov)
        # :852-859, mahalanobisDistance :880-897 reads invCov[i + N j]
        dist = np.zeros(L)
        for i in range(N):
            tmp = np.zeros(L)
            for j in range(N):
                tmp = tmp + dif[:, j] * self.inv_cov[j, i]
            tmp = tmp * dif[:, i]
            dist = dist + tmp
        mx = LOWEST
        for v in dist:
            if v > mx:
                mx = float(v)
        point_volume = exp_cr(self.s["LogVolume"]) * float(L) / float(L)
        vol = math.sqrt(pow_cr(self.scaling * mx, float(N)) * det) * self.K
        if vol > point_volume:
            ef = self.scaling * mx
        else:
            ef = pow_cr((point_volume * point_volume) / (self.K * self.K * det), 1. / float(N))
        self.volume = pow_cr(ef, N / 2.) * math.sqrt(det) * self.K
        self.det = det
        self.cov = self.cov * ef
        self.inv_cov = self.inv_cov * (1. / ef)
        self.axes = axes * math.sqrt(ef)

    # ------------------------------------------------------------ candidates
    def _tries(self, T):
        """T tries from the generators' current position -> (X, inside flags)"""
        N = self.N
        if not self.ellipse:
            u = self._uniforms(T * N).reshape(T, N)
            X = self.box_lo + u * (self.box_up - self.box_lo)
            return X, np.all((X >= 0.) & (X <= 1.), axis=1)
        Z = self._normals(T * N).reshape(T, N)
        U = self._uniforms(T)
        ln = np.zeros(T)
        for d in range(N):
            ln = ln + Z[:, d] * Z[:, d]
        inv_n = 1. / float(N)
        s = np.array([pow_cr(float(u), inv_n) for u in U]) / np.sqrt(ln)
        V = Z * s[:, None]
        X = np.zeros((T, N))
        idx = np.arange(T)  # tries still inside after the coordinates so far
        for k in range(N):
            x = np.full(idx.size, self.mean[k])
            for l in range(k + 1):
                x = x + self.axes[k, l] * V[idx, l]
            X[idx, k] = x
            idx = idx[(x >= 0.) & (x <= 1.)]
            if idx.size == 0:
                break
        ok = np.zeros(T, dtype=bool)
        ok[idx] = True
        return X, ok

    def generate_candidates(self):
        """:402-443"""
        B, kept = self.B, 0
        self.last_tries = self.last_blocks = 0
        T = self.block
        while kept < B:
            su, sn = self.uniform.get_bytes(), self.normal.get_bytes()
            X, ok = self._tries(T)
            self.last_blocks += 1
            hit = np.flatnonzero(ok)[:B - kept]
            self.cand[kept:kept + hit.size] = X[hit]
            kept += hit.size
            if kept < B:
                self.last_tries += T
                if hit.size == 0 and T < 16384:
                    T *= 2
                continue
            used = int(hit[-1]) + 1
            self.last_tries += used
            if used < T:  # leave the generators behind try `used`
                self.uniform.set_bytes(su)
                self.normal.set_bytes(sn)
                if self.ellipse:
                    self._normals(used * self.N)
                    self._uniforms(used)
                else:
                    self._uniforms(used * self.N)

    # ------------------------------------------------------------ generation
    def prepare(self):
        """updateBounds, generateCandidates and the evaluation of :169-197"""
        self.update_bounds()
        self.generate_candidates()
        _, self.cand_ll, self.cand_lp, self.cand_lpw = self._evaluate(self.cand)
        self.s["Model Evaluation Count"] += self.B
        self.s["Generated Samples"] += self.B

    def _dead(self, x, lp, lpw, ll):
        """updateDeadSamples (:518-530), updateEffectiveSamples (:981-987)"""
        s = self.s
        s["Number Dead Samples"] += 1
        self.dead.append([self.lower[d] + float(x[d]) * self.width[d] for d in range(self.N)])
        self.dead_lp.append(float(lp))
        self.dead_lpw.append(float(lpw))
        self.dead_ll.append(float(ll))
        self.dead_lw.append(s["LogWeight"])
        w = s["LogWeight"]
        s["Sum Log Weights"] = safe_log_plus(s["Sum Log Weights"], w)
        s["Sum Square Log Weights"] = safe_log_plus(s["Sum Square Log Weights"], 2. * w)
        s["Effective Sample Size"] = _exp(2. * s["Sum Log Weights"] - s["Sum Square Log Weights"])

    def process(self):
        """processGeneration (:297-364) -> accepted"""
        s = self.s
        idx = self.rank[0]
        before = s["Accepted Samples"]
        for c in range(self.B):
            if self.cand_ll[c] < s["LStar"]:
                continue
            s["Accepted Samples"] += 1
            lv_old, info_old, le_old = s["LogVolume"], s["Information"], s["LogEvidence"]
            s["LogVolume"] -= s["Expected LogShrinkage"]
            d_log_vol = _log(0.5 * _exp(lv_old) - 0.5 * _exp(s["LogVolume"]))
            s["LogWeight"] = safe_log_plus(s["LStar"], s["LStarOld"]) + d_log_vol
            s["LogEvidence"] = safe_log_plus(s["LogEvidence"], s["LogWeight"])
            with np.errstate(all="ignore"):
                term = float(np.float64(_exp(s["LStarOld"] - s["LogEvidence"])) * np.float64(s["LStarOld"])
                             + np.float64(_exp(s["LStar"] - s["LogEvidence"])) * np.float64(s["LStar"]))
            if math.isfinite(term):
                s["Information"] = (_exp(d_log_vol) * term + _exp(le_old - s["LogEvidence"]) * (info_old + le_old)
                                    - s["LogEvidence"])
                s["LogEvidence Var"] += 2. * (s["Information"] - info_old) * s["Expected LogShrinkage"]
            if math.isfinite(self._key(idx)):
                self._dead(self.live[idx], self.live_lp[idx], self.live_lpw[idx], self.live_ll[idx])
            self.live[idx] = self.cand[c]
            self.live_lp[idx] = self.cand_lp[c]
            self.live_lpw[idx] = self.cand_lpw[c]
            self.live_ll[idx] = self.cand_ll[c]
            self._sort()
            idx = self.rank[0]
            k = self._key(idx)
            if math.isfinite(k):
                s["LStarOld"] = s["LStar"]
                s["LStar"] = float(k)
        s["Max Evaluation"] = float(self._key(self.rank[-1]))
        s["Remaining Log Evidence"] = s["Max Evaluation"] + s["LogVolume"]
        s["Log Evidence Difference"] = safe_log_plus(s["LogEvidence"], s["Remaining Log Evidence"]) - s["LogEvidence"]
        self._bounds_volume()
        s["Last Accepted"] += 1
        return before != s["Accepted Samples"]

    def _bounds_volume(self):
        """setBoundsVolume (:378-392)"""
        if not self.ellipse:
            v = LOWEST
            for d in range(self.N):
                v = safe_log_plus(v, _log(float(self.box_up[d] - self.box_lo[d])))
            self.s["Bound LogVolume"] = v
        else:
            self.s["Bound LogVolume"] = _log(self.volume)

    def generation(self):
        """runGeneration for generations > 1 (:160-203) -> the criteria that hold after it"""
        self.s["Last Accepted"] = 0
        accepted = False
        while not accepted:
            self.prepare()
            self.s["Last Accepted"] += 1
            accepted = self.process()

    def terminated(self, generation):
        """Nested.config:63-83"""
        out = []
        if generation > 1 and self.s["Log Evidence Difference"] <= self.min_delta:
            out.append("Min Log Evidence Delta")
        if self.max_ess <= self.s["Effective Sample Size"]:
            out.append("Max Effective Sample Size")
        if self.max_ll <= self.s["LStar"]:
            out.append("Max Log Likelihood")
        return out

    def run(self, max_generations=10**9):
        self.first_generation()
        g = 1
        while g < max_generations and not self.terminated(g):
            g += 1
            self.generation()
        return g

    # -------------------------------------------------------------- finalize
    def consume_live_samples(self):
        """:532-578 (:547 runs one entry past logdvols; the entries that exist get the term)"""
        s, L = self.s, self.L
        logvols = [s["LogVolume"]] * (L + 1)
        logdvols, dlvs = [0.0] * L, [0.0] * L
        for i in range(L):
            logvols[i + 1] += _log(1. - (i + 1.) / (L + 1.))
            logdvols[i] = safe_log_minus(logvols[i], logvols[i + 1])
            dlvs[i] = logvols[i] - logvols[i + 1]
        for i in range(L):
            logdvols[i] += math.log(0.5)
        for i in range(L):
            idx = self.rank[i]
            le_old, info_old = s["LogEvidence"], s["Information"]
            k = self._key(idx)
            if math.isfinite(k):
                s["LStarOld"] = s["LStar"]
                s["LStar"] = float(k)
                self._dead(self.live[idx], self.live_lp[idx], self.live_lpw[idx], self.live_ll[idx])
            d_log_vol = logdvols[i]
            s["LogVolume"] = safe_log_minus(s["LogVolume"], d_log_vol)
            s["LogWeight"] = safe_log_plus(s["LStar"], s["LStarOld"]) + d_log_vol
            s["LogEvidence"] = safe_log_plus(s["LogEvidence"], s["LogWeight"])
            with np.errstate(all="ignore"):
                term = float(np.float64(_exp(s["LStarOld"] - s["LogEvidence"])) * np.float64(s["LStarOld"])
                             + np.float64(_exp(s["LStar"] - s["LogEvidence"])) * np.float64(s["LStar"]))
                s["Information"] = float(np.float64(_exp(d_log_vol)) * term
                                         + _exp(le_old - s["LogEvidence"]) * (info_old + le_old) - s["LogEvidence"])
            s["LogEvidence Var"] += 2. * (s["Information"] - info_old) * dlvs[i]

    def finalize(self, permutation):
        """:1017-1027; permutation(seed, n) -> the shuffled iota of :584-586"""
        if self.add_live_points:
            self.consume_live_samples()
        nd = len(self.dead_lw)
        mx = max(self.dead_lw)
        perm = permutation(self.shuffle_seed, nd)
        k = 1.
        total = float(self._uniforms(1)[0])
        self.post, self.post_lp, self.post_ll = [], [], []
        for i in range(nd):
            r = int(perm[i])
            total += _exp(self.dead_lw[r] - mx)
            if total > k:
                self.post.append(self.dead[r])
                self.post_lp.append(self.dead_lp[r])
                self.post_ll.append(self.dead_ll[r])
                k += 1

    # ----------------------------------------------------------------- state
    def field_names(self, posterior=False):
        return SCALARS + LIVE + CANDIDATES + DEAD + (ELLIPSE if self.ellipse else BOX) + (POSTERIOR if posterior else [])

    def __getitem__(self, name):
        f = {"Live Samples": self.live, "Live LogLikelihoods": self.live_ll, "Live LogPriors": self.live_lp,
             "Live LogPrior Weights": self.live_lpw, "Live Samples Rank": self.rank, "Candidates": self.cand,
             "Candidate LogLikelihoods": self.cand_ll, "Candidate LogPriors": self.cand_lp,
             "Candidate LogPrior Weights": self.cand_lpw, "Dead Samples": self.dead, "Dead LogLikelihoods": self.dead_ll,
             "Dead LogPriors": self.dead_lp, "Dead LogPrior Weights": self.dead_lpw, "Dead LogWeights": self.dead_lw,
             "Box Lower Bound": self.box_lo, "Box Upper Bound": self.box_up, "Ellipse Mean": self.mean,
             "Covariance Matrix": self.cov, "Ellipse Inverse Covariance": self.inv_cov, "Ellipse Axes": self.axes,
             "Ellipse Determinant": [self.det], "Ellipse Volume": [self.volume],
             "Posterior Samples Database": self.post, "Posterior Samples LogPrior Database": self.post_lp,
             "Posterior Samples LogLikelihood Database": self.post_ll}
        if name in self.s:
            return np.array([self.s[name]], dtype=np.float64)
        return np.asarray(f[name], dtype=np.float64).reshape(-1)
