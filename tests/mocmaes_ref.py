"""Plain Python/NumPy restatement of the reference's multi-objective CMA-ES
(source/modules/solver/optimizer/MOCMAES/MOCMAES.cpp.base), the oracle of the
MOCMAES tests: setInitialConfiguration, one generation (prepareGeneration,
sampleSingle, sortSampleIndices, updateDistribution) and updateStatistics, in
IEEE double arithmetic in the reference's order, one rounding per operation.

Normals and uniforms come from the oracle's GSL mt19937 (oracle.refcpu.Rng),
the factor from kr_cholesky, the transform from kr_dtrmv_lower, and the step
size's exponential from kr_exp_cr (the correctly rounded exp the device
evaluates as well; with math.exp two of the recorded windows differ).

parent_order: "descending" is the snapshot's slot order
(pidx = values.size() - sortedIndices[i] - 1, :385); "recorded" fills the
slots in ascending index of the merged population, which is what the
reference's committed result files (tests/python/plot/mocmaes) were written
with.
"""
import ctypes as C
import gzip
import json
import math
import os

import numpy as np

from oracle import refcpu

INF = float("inf")

PER_SAMPLE = ["Sample Population", "Sigma", "Covariance Matrix", "Evolution Paths", "Success Probabilities"]
FIELDS = (["Current Values", "Previous Values", "Parent Index"]
          + [p + " " + s for s in PER_SAMPLE for p in ("Current", "Previous", "Parent")]
          + ["Best Ever Values", "Best Ever Variables Vector", "Previous Best Values", "Previous Best Variables Vector",
             "Current Best Values", "Current Best Variables Vector", "Current Best Value Differences",
             "Current Best Variable Differences", "Current Min Standard Deviations", "Current Max Standard Deviations",
             "Sample Collection", "Sample Value Collection"])
SCALARS = ["Current Non Dominated Sample Count", "Infeasible Sample Count", "Model Evaluation Count"]
# the names the older recorder used
RECORDED_NAMES = {"Previous Best Variables Vector": "Previous Best Variables"}


def load_golden():
    """The reference's 36 recorded states (tests/golden/make_mocmaes_golden.py),
    with 'Sample Collection' and 'Sample Value Collection' put back."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mocmaes_golden.json.gz")
    with gzip.open(path, "rt") as f:
        j = json.load(f)
    rows = j["archive rows"]
    for s in j["states"]:
        idx = s["Solver"].pop("Archive")
        s["Solver"]["Sample Collection"] = [rows[i][0] for i in idx]
        s["Solver"]["Sample Value Collection"] = [rows[i][1] for i in idx]
    return j["states"]


def _exp_cr(x):
    L = refcpu.lib()
    if not getattr(L, "_mocmaes_exp", False):
        L.kr_exp_cr.argtypes = [C.c_double]
        L.kr_exp_cr.restype = C.c_double
        L._mocmaes_exp = True
    return L.kr_exp_cr(x)


# ---------------------------------------------------------------- objectives
# examples/optimization/multiobjective/_model/model.py, with x*x for **2
def negative_rosenbrock_and_sphere(x):
    one = 0.0
    for i in range(len(x) - 1):
        t = x[i + 1] - x[i] * x[i]
        u = 1 - x[i]
        one += 100 * (t * t) + u * u
    two = 0.0
    for v in x:
        two += v * v
    return [-one, -two]


def negative_rosenbrock_and_two_spheres(x):
    one, two = negative_rosenbrock_and_sphere(x)
    three = 0.0
    for v in x:
        three += (v - 2) * (v - 2)
    return [one, two, -three]


OBJECTIVES = {2: negative_rosenbrock_and_sphere, 3: negative_rosenbrock_and_two_spheres}


# ---------------------------------------------------------------------- sort
def sort_literal(values):
    """sortSampleIndices (:230-332) as written.  (A peeling round that finds
    nothing unranked assigns nothing: those rounds are skipped.)"""
    n, K = len(values), len(values[0])
    rank = [0] * n
    min_rank = n
    for r in range(n, 0, -1):
        if all(rank):
            break
        min_max = K
        max_nb = [0] * n
        for i in range(n):
            if rank[i] == 0:
                for j in range(n):
                    if i != j and rank[j] == 0:
                        nb = 0
                        for k in range(K):
                            if values[i][k] < values[j][k]:
                                nb += 1
                        if nb > max_nb[i]:
                            max_nb[i] = nb
                if max_nb[i] < min_max:
                    min_max = max_nb[i]
        for i in range(n):
            if rank[i] == 0 and max_nb[i] == min_max:
                rank[i] = r
                if r < min_rank:
                    min_rank = r
    max_rank = n - min_rank
    rank = [r - min_rank for r in rank]
    reference = [INF] * K
    for i in range(n):
        for k in range(K):
            if values[i][k] < reference[k]:
                reference[k] = values[i][k]
    order_of = [-1] * n
    order = 0
    with np.errstate(invalid="ignore"):
        for r in range(max_rank + 1):
            unsorted = [i for i in range(n) if rank[i] == r and order_of[i] == -1]
            while unsorted:
                m = len(unsorted)
                ub = [[-INF] * K for _ in range(m)]
                for i in range(m):
                    for j in range(m):
                        if i != j:
                            for k in range(K):
                                if values[unsorted[j]][k] > ub[i][k]:
                                    ub[i][k] = values[unsorted[j]][k]
                contrib = [0.0] * m
                for i in range(m):
                    for k in range(K):
                        contrib[i] = float(np.float64(contrib[i]) + (np.float64(ub[i][k]) - np.float64(reference[k])))
                nxt, cur = unsorted[0], contrib[0]
                for i in range(1, m):
                    if contrib[i] > cur:
                        cur, nxt = contrib[i], unsorted[i]
                order_of[nxt] = order
                unsorted = [i for i in range(n) if rank[i] == r and order_of[i] == -1]
                order += 1
    return order_of


def sort_vectorised(values):
    """The same order: peeling rounds as array passes; per rank group the
    exclusive upper bound max_{j != i} from the group's two largest values and
    the multiplicity of the largest, per objective.  maxNBetter[i] is read off
    cnt[i, c], the number of unranked j with nBetter(i, j) = c, which a round
    updates by the columns of the samples it ranked (n^2 K work in all)."""
    v = np.asarray(values, dtype=np.float64)
    n, K = v.shape
    nb = (v[:, None, :] < v[None, :, :]).sum(axis=2)  # nb[i, j]: objectives in which i is worse than j
    cnt = np.stack([(nb == c).sum(axis=1) for c in range(K + 1)], axis=1)  # (j == i counts in c = 0: harmless)
    levels = np.arange(K + 1)
    rnd = np.full(n, -1)
    t = 0
    while (rnd < 0).any():
        un = rnd < 0
        max_nb = np.where(cnt > 0, levels[None, :], 0).max(axis=1)
        min_max = min(K, max_nb[un].min())
        ranked = np.flatnonzero(un & (max_nb == min_max))
        rnd[ranked] = t
        sub = nb[:, ranked]
        for c in range(K + 1):
            cnt[:, c] -= (sub == c).sum(axis=1)
        t += 1
    rounds = t
    reference = np.minimum(v.min(axis=0), INF)
    order_of = np.full(n, -1)
    order = 0
    with np.errstate(invalid="ignore"):
        for g in range(rounds - 1, -1, -1):  # rank r = rounds - 1 - round, ascending r
            members = np.flatnonzero(rnd == g)
            while members.size:
                w = v[members]
                if members.size == 1:
                    ub = np.full((1, K), -INF)
                else:
                    top = w.max(axis=0)
                    cnt = (w == top).sum(axis=0)
                    second = np.where(w == top, -INF, w).max(axis=0)
                    ub = np.where((w == top) & (cnt == 1), second, top)
                contrib = np.zeros(members.size)
                for k in range(K):
                    contrib = contrib + (ub[:, k] - reference[k])
                if math.isnan(contrib[0]):
                    pick = 0
                else:
                    pick = int(np.argmax(np.where(np.isnan(contrib), -INF, contrib)))
                order_of[members[pick]] = order
                order += 1
                members = np.delete(members, pick)
    return [int(o) for o in order_of]


# -------------------------------------------------------------------- solver
class Mocmaes:
    def __init__(self, lower, upper, population, mu=0, num_objectives=2, initial_value=None, initial_sdev=None,
                 cc=-1.0, ccov=-1.0, target_success_rate=0.175, success_learning_rate=0.08, normal_seed=1,
                 uniform_seed=2, parent_order="descending", objective=None):
        assert parent_order in ("descending", "recorded")
        self.lb = [float(x) for x in lower]
        self.ub = [float(x) for x in upper]
        self.N = len(self.lb)
        self.K = int(num_objectives)
        self.parent_order = parent_order
        self.objective = objective or OBJECTIVES[self.K]
        N = self.N
        # setInitialConfiguration (:10-140)
        P = int(population) or int(math.ceil(4. + math.floor(3. * math.log(float(N)))))
        mu = int(mu) or int(P / 2.)
        assert mu <= P
        self.P, self.mu = P, mu
        x0 = [None] * N if initial_value is None else list(initial_value)
        sd = [None] * N if initial_sdev is None else list(initial_sdev)
        trace = 0.
        for d in range(N):
            if x0[d] is None or not math.isfinite(x0[d]):
                x0[d] = (self.ub[d] + self.lb[d]) * 0.5
            if sd[d] is None or not math.isfinite(sd[d]):
                sd[d] = (self.ub[d] - self.lb[d]) * 0.3
            trace += sd[d] * sd[d]
        self.cc = cc if cc >= 0. else 2. / (N + 2.)
        self.ccov = ccov if ccov >= 0. else 2. / (N * N + 6.)
        self.cp = success_learning_rate
        self.target = target_success_rate
        K = self.K
        f = {}
        for p in ("Current", "Previous"):
            f[p + " Sample Population"] = np.zeros((P, N))
            f[p + " Values"] = np.full((P, K), -INF)
            f[p + " Sigma"] = np.zeros(P)
            f[p + " Success Probabilities"] = np.zeros(P)
            f[p + " Evolution Paths"] = np.zeros((P, N))
            f[p + " Covariance Matrix"] = np.zeros((P, N * N))
        f["Parent Index"] = np.zeros(P)
        f["Parent Success Probabilities"] = np.full(mu, self.target)
        psig = math.sqrt(trace / N)
        f["Parent Sigma"] = np.full(mu, psig)
        # :119: the parents start at 0; the inferred 'Initial Value' is never read again
        f["Parent Sample Population"] = np.zeros((mu, N))
        f["Parent Evolution Paths"] = np.zeros((mu, N))
        C0 = np.zeros((mu, N * N))
        for d in range(N):
            C0[:, d * N + d] = sd[d] * sd[d] / (psig * psig)
        f["Parent Covariance Matrix"] = C0
        for nm in ("Best Ever", "Previous Best", "Current Best"):
            f[nm + " Values"] = np.full(K, -INF)
            f[nm + " Variables Vector"] = np.zeros((K, N))
        f["Current Best Value Differences"] = np.full(K, INF)
        f["Current Best Variable Differences"] = np.full(K, INF)
        f["Current Min Standard Deviations"] = np.full(P, min(sd))
        f["Current Max Standard Deviations"] = np.full(P, max(sd))
        f["Sample Collection"] = np.zeros((0, N))
        f["Sample Value Collection"] = np.zeros((0, K))
        f["Current Non Dominated Sample Count"] = 1
        f["Infeasible Sample Count"] = 0
        f["Model Evaluation Count"] = 0
        self.f = f
        self.normal = refcpu.Rng(seed=normal_seed)
        self.uniform = refcpu.Rng(seed=uniform_seed)
        self.blocks_last = 0  # blocks of N normals the last generation drew

    # ---- state exchange with a recorded 'Solver' object
    def load(self, sv):
        for name in FIELDS:
            if RECORDED_NAMES.get(name, name) not in sv:
                continue  # ('Best Ever Variables Vector': the older recorder did not write it)
            rec = sv[RECORDED_NAMES.get(name, name)]
            cur = self.f[name]
            arr = np.asarray(rec, dtype=np.float64)
            if name in ("Sample Collection", "Sample Value Collection"):
                arr = arr.reshape(len(rec), cur.shape[1])
            self.f[name] = arr.reshape((-1,) + cur.shape[1:]).copy()
        for name in SCALARS:
            self.f[name] = int(sv[name])
        self.normal.from_hex(sv["Multinormal Generator"]["Range"])
        self.uniform.from_hex(sv["Uniform Generator"]["Range"])

    def feasible(self, x):
        for d in range(self.N):
            if not math.isfinite(x[d]) or x[d] < self.lb[d] or x[d] > self.ub[d]:
                return False
        return True

    def prepare(self):
        """prepareGeneration + sampleSingle (:172-228)."""
        f, N, P = self.f, self.N, self.P
        for nm in ["Values"] + PER_SAMPLE:
            f["Previous " + nm] = f["Current " + nm]
            f["Current " + nm] = f["Current " + nm].copy()
        lib = refcpu.lib()
        dp = C.POINTER(C.c_double)
        factors = {}
        self.blocks_last = 0
        for i in range(P):
            if self.mu == P:
                p = i
            else:
                p = int(math.floor(min(self.mu, f["Current Non Dominated Sample Count"]) * self.uniform.flat(0., 1.)))
            f["Parent Index"][i] = p
            if p not in factors:
                L = f["Parent Covariance Matrix"][p].copy()
                lib.kr_cholesky(N, L.ctypes.data_as(dp))  # (status ignored, :203)
                factors[p] = L * f["Parent Sigma"][p]      # gsl_matrix_scale (:204)
            L = factors[p]
            while True:
                x = np.array([self.normal.gaussian(1.0) for _ in range(N)])
                lib.kr_dtrmv_lower(N, L.ctypes.data_as(dp), x.ctypes.data_as(dp))
                x = x + f["Parent Sample Population"][p]
                self.blocks_last += 1
                if self.feasible(x):
                    break
            f["Current Sample Population"][i] = x
            for nm in PER_SAMPLE[1:]:
                f["Current " + nm][i] = f["Parent " + nm][p]

    def evaluate(self, values=None):
        f = self.f
        if values is None:
            values = [self.objective([float(v) for v in x]) for x in f["Current Sample Population"]]
        f["Current Values"] = np.asarray(values, dtype=np.float64).reshape(self.P, self.K).copy()
        f["Model Evaluation Count"] += self.P

    def update(self, sorter=sort_vectorised):
        """updateDistribution (:334-408)."""
        f, N, P, mu = self.f, self.N, self.P, self.mu
        values = np.concatenate([f["Current Values"], f["Previous Values"]])
        order = sorter(values.tolist())
        n = len(order)
        cc, ccov, cp = self.cc, self.ccov, self.cp
        factor = math.sqrt(cc * (2. - cc))
        damp = 1.0 + 2.0 * max(0.0, math.sqrt((mu - 1.) / (N + 1.)) - 1.0) + cc
        chiN = math.sqrt(N) * (1. - 1. / (4. * N) + 1. / (21. * N * N))
        X, S, Cm, Pa, Sr = (f["Current " + nm] for nm in PER_SAMPLE)
        for i in range(P):
            s = Sr[i] * (1. - cp)
            if order[i] >= n - mu:
                s += cp
            Sr[i] = min(s, 1.0)
            parent = f["Parent Sample Population"][int(f["Parent Index"][i])]
            path = (1. - cc) * Pa[i]
            diag = Cm[i][::N + 1]
            path = path + factor / np.sqrt(diag) * (X[i] - parent) / S[i]
            Pa[i] = path
            length = 0.
            for d in range(N):
                length += path[d] * path[d]
            length = math.sqrt(length)
            Cn = (1. - ccov) * Cm[i].reshape(N, N) + (ccov * path)[:, None] * path[None, :]
            if Sr[i] >= self.target:
                Cn = Cn + ccov * factor * factor * Cn
            Cm[i] = Cn.reshape(-1)
            S[i] = S[i] * _exp_cr(cc / damp * (length / chiN - 1.0))
        # parents (:381-407)
        new = {nm: f["Parent " + nm].copy() for nm in PER_SAMPLE}
        ordinal = 0
        for i in range(n):
            if order[i] >= n - mu:
                pidx = n - order[i] - 1 if self.parent_order == "descending" else ordinal
                ordinal += 1
                src, j = ("Current ", i) if i < P else ("Previous ", i - P)
                for nm in PER_SAMPLE:
                    new[nm][pidx] = f[src + nm][j]
        for nm in PER_SAMPLE:
            f["Parent " + nm] = new[nm]

    def statistics(self):
        """updateStatistics (:410-520)."""
        f, N, P, K = self.f, self.N, self.P, self.K
        f["Previous Best Values"] = f["Current Best Values"].copy()
        f["Previous Best Variables Vector"] = f["Current Best Variables Vector"].copy()
        V, X = f["Current Values"], f["Current Sample Population"]
        best = np.full(K, -INF)
        for i in range(P):
            for k in range(K):
                if V[i][k] > best[k]:
                    best[k] = V[i][k]
                    f["Current Best Variables Vector"][k] = X[i]
                    f["Current Best Value Differences"][k] = best[k] - f["Previous Best Values"][k]
                    l2 = 0.
                    for d in range(N):
                        t = f["Previous Best Variables Vector"][k][d] - X[i][d]
                        l2 += t * t
                    f["Current Best Variable Differences"][k] = math.sqrt(l2)
        f["Current Best Values"] = best
        for k in range(K):
            if best[k] > f["Best Ever Values"][k]:
                f["Best Ever Values"][k] = best[k]
                f["Best Ever Variables Vector"][k] = f["Current Best Variables Vector"][k]
        # :451-459, with _currentSigma[d] as written
        assert N <= P, "the reference reads _currentSigma[d] for d < N: out of bounds when N > P"
        diag = f["Current Covariance Matrix"][:, ::N + 1]
        sdev = f["Current Sigma"][None, :N] * np.sqrt(diag)
        f["Current Max Standard Deviations"] = sdev.max(axis=1)
        f["Current Min Standard Deviations"] = sdev.min(axis=1)
        dominated = ((V[None, :, :] > V[:, None, :]).sum(axis=2) == K).any(axis=1)  # (j == i never counts K)
        cand = np.flatnonzero(~dominated)
        f["Current Non Dominated Sample Count"] = int(cand.size)
        A, AV = f["Sample Collection"], f["Sample Value Collection"]
        cv = V[cand]
        if len(AV):
            cdom = (cv[:, None, :] > AV[None, :, :]).sum(axis=2) == K
            sdom = (cv[:, None, :] < AV[None, :, :]).sum(axis=2) == K
            keep_s, keep_c = ~cdom.any(axis=0), ~sdom.any(axis=1)
        else:
            keep_s, keep_c = np.zeros(0, dtype=bool), np.ones(cand.size, dtype=bool)
        f["Sample Collection"] = np.concatenate([A[keep_s], X[cand][keep_c]])
        f["Sample Value Collection"] = np.concatenate([AV[keep_s], cv[keep_c]])

    def generation(self, values=None, sorter=sort_vectorised):
        self.prepare()
        self.evaluate(values(self.f["Current Sample Population"]) if callable(values) else values)
        self.update(sorter)
        self.statistics()


# ------------------------------------------------- comparison with a recording
# The recorder evaluated model.py's `**2` through its own libm: in these four
# ten-generation windows (named by their first generation) an objective value
# differs from x*x by a few ulps.  Parameters, selections and both generator
# states still match there.
VALUE_EXCEPTIONS = {(200, "Sample Value Collection"), (260, "Sample Value Collection"),
                    (300, "Sample Value Collection"), (340, "Current Values")}


def mismatches(get, ranges, sv, window, names=RECORDED_NAMES):
    """Names of the recorded fields of state `sv` that `get(name)` (an array or
    a number) does not reproduce exactly; `ranges` = (multinormal, uniform)
    GSL states as upper-case hex.  The window's listed value exceptions are
    exempt from equality, not from their length.  `names`: how `sv` spells
    the fields whose name changed since the recording."""
    bad = []
    for name in FIELDS + SCALARS:
        rname = names.get(name, name)
        if rname not in sv:
            continue
        rec = np.asarray(sv[rname], dtype=np.float64).reshape(-1)
        got = np.asarray(get(name), dtype=np.float64).reshape(-1)
        if rec.shape != got.shape:
            bad.append(name + " (length)")
        elif (window, name) not in VALUE_EXCEPTIONS and not np.array_equal(rec, got):
            bad.append(name)
    if ranges[0] != sv["Multinormal Generator"]["Range"]:
        bad.append("Multinormal Generator/Range")
    if ranges[1] != sv["Uniform Generator"]["Range"]:
        bad.append("Uniform Generator/Range")
    return bad


def recorded_setup(states, parent_order="recorded"):
    """The recorded run's configuration as a Mocmaes (seeds from state 0)."""
    sv, var = states[0]["Solver"], states[0]["Variables"]
    return Mocmaes([v["Lower Bound"] for v in var], [v["Upper Bound"] for v in var], sv["Population Size"],
                   mu=sv["Mu Value"], num_objectives=2, initial_value=[v["Initial Value"] for v in var],
                   initial_sdev=[v["Initial Standard Deviation"] for v in var],
                   normal_seed=sv["Multinormal Generator"]["Random Seed"],
                   uniform_seed=sv["Uniform Generator"]["Random Seed"], parent_order=parent_order)


def as_recorded(m, names=RECORDED_NAMES):
    """A copy of a Mocmaes's state in the shape of a recorded 'Solver' object (what mismatches() compares with)."""
    sv = {names.get(name, name): np.array(m.f[name], dtype=np.float64) for name in FIELDS + SCALARS}
    sv["Multinormal Generator"] = {"Range": m.normal.to_hex()}
    sv["Uniform Generator"] = {"Range": m.uniform.to_hex()}
    return sv
