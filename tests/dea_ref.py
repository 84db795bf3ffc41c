"""Plain NumPy restatement of the reference's differential evolution solver
(source/modules/solver/optimizer/DEA/DEA.cpp.base), the oracle of the DEA
tests.  Every rule and both 'Fix Infeasible' settings; IEEE double arithmetic
in the reference's order, one rounding per operation.

The uniform stream is GSL's mt19937: np.random.MT19937 carries the same
recurrence and tempering, gsl_rng_uniform is random_raw() / 2**32 (no zero
skip), and GSL's seeding equals the legacy RandomState(seed & 0xffffffff)
one.  A GSL state as Korali serialises it ('Range': 624 uint64 words + int32
mti + 4 pad bytes, as upper-case hex) loads and exports losslessly.
"""
import gzip
import json
import os
import struct

import numpy as np

INF = float("inf")

VECTORS = ["Sample Population", "Candidate Population", "Value Vector", "Previous Value Vector", "Current Mean",
           "Previous Mean", "Best Ever Variables", "Current Best Variables", "Max Distances"]
SCALARS = ["Best Ever Value", "Previous Best Ever Value", "Current Best Value", "Previous Best Value",
           "Best Sample Index", "Infeasible Sample Count", "Model Evaluation Count", "Mutation Rate", "Crossover Rate",
           "Current Minimum Step Size"]


def load_golden():
    """The reference's 24 recorded generation files (tests/golden/make_dea_golden.py)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dea_golden.json.gz")
    with gzip.open(path, "rt") as f:
        return json.load(f)["generations"]


class GslStream:
    def __init__(self, seed=None, state=None):
        self.bg = np.random.MT19937()
        if state is not None:
            self.load(state)
        else:
            s = int(seed) & 0xFFFFFFFF
            if s == 0:
                s = 4357  # gsl mt.c
            self.bg.state = np.random.RandomState(s).get_state(legacy=False)
        self.words = 0

    def load(self, state):
        if isinstance(state, str):
            state = bytes.fromhex(state)
        assert len(state) == 5000
        key = np.frombuffer(state[:624 * 8], dtype="<u8").astype(np.uint32)
        (mti,) = struct.unpack("<i", state[624 * 8:624 * 8 + 4])
        self.bg.state = {"bit_generator": "MT19937", "state": {"key": key, "pos": mti}}

    def export(self):
        st = self.bg.state["state"]
        return st["key"].astype("<u8").tobytes() + struct.pack("<i", int(st["pos"])) + b"\0\0\0\0"

    def hex(self):
        return self.export().hex().upper()

    def uniform(self):
        self.words += 1
        return int(self.bg.random_raw()) / 4294967296.0


def negative_rosenbrock(x):
    res = 0.0
    for i in range(len(x) - 1):
        res += 100 * (x[i + 1] - x[i] ** 2) ** 2 + (1 - x[i]) ** 2
    return -res


def negative_sphere(x):
    res = 0.0
    for v in x:
        res += v ** 2
    return -0.5 * res


class DeaRef:
    FIELDS = VECTORS + SCALARS

    def __init__(self, N, P, lower, upper, crossover_rate=0.9, mutation_rate=0.5, mutation_rule="Fixed",
                 parent_rule="Random", accept_rule="Greedy", fix_infeasible=True, uniform_seed=0, max_attempts=10**6):
        self.N, self.P = int(N), int(P)
        self.lb = np.broadcast_to(np.asarray(lower, dtype=np.float64), (self.N,)).copy()
        self.ub = np.broadcast_to(np.asarray(upper, dtype=np.float64), (self.N,)).copy()
        self.s = {"Crossover Rate": float(crossover_rate), "Mutation Rate": float(mutation_rate),
                  "Model Evaluation Count": 0, "Infeasible Sample Count": 0, "Best Sample Index": 0}
        self.mutation_rule, self.parent_rule, self.accept_rule = mutation_rule, parent_rule, accept_rule
        self.fix = bool(fix_infeasible)
        self.rng = GslStream(seed=uniform_seed)
        self.max_attempts = max_attempts

    def __getitem__(self, k):
        return self.s[k]

    def __setitem__(self, k, v):
        if isinstance(self.s.get(k), np.ndarray) or isinstance(v, (list, np.ndarray)):
            v = np.array(v, dtype=np.float64)
        self.s[k] = v

    # setInitialConfiguration (:15-61) with initSamples (:87-97)
    def initialize(self):
        N, P, s = self.N, self.P, self.s
        X = np.empty((P, N))
        for i in range(P):
            for d in range(N):
                width = self.ub[d] - self.lb[d]
                X[i, d] = self.lb[d] + width * self.rng.uniform()
        s["Candidate Population"] = X.copy()
        s["Sample Population"] = X
        s["Value Vector"] = np.full(P, -INF)
        s["Previous Value Vector"] = np.zeros(P)
        for k in ("Previous Mean", "Best Ever Variables", "Current Best Variables", "Max Distances"):
            s[k] = np.zeros(N)
        s["Infeasible Sample Count"] = 0
        s["Best Sample Index"] = 0
        for k in ("Previous Best Value", "Current Best Value", "Previous Best Ever Value", "Best Ever Value"):
            s[k] = -INF
        s["Current Minimum Step Size"] = INF
        s["Current Mean"] = self._mean()

    def _mean(self):
        X, P = self.s["Sample Population"], self.P
        m = np.zeros(self.N)
        for i in range(P):
            m = m + X[i] / float(P)  # per d: a true division, then the add, in order over i
        return m

    def _feasible(self, x):  # Optimizer::isSampleFeasible
        return bool(np.all(np.isfinite(x)) and not np.any(x < self.lb) and not np.any(x > self.ub))

    def _index(self, n):
        return int(self.rng.uniform() * n)

    def _mutate(self, i):  # mutateSingle (:118-176)
        s, P, N, X = self.s, self.P, self.N, self.s["Sample Population"]
        while True:
            a = self._index(P)
            if a != i:
                break
        while True:
            b = self._index(P)
            if b != i and b != a:
                break
        if self.mutation_rule == "Self Adaptive":
            rd2 = self.rng.uniform()
            rd3 = self.rng.uniform()
            if rd2 < 0.1:
                s["Mutation Rate"] = 0.1 + self.rng.uniform() * 0.9
            if rd3 < 0.1:
                s["Crossover Rate"] = self.rng.uniform()
        if self.parent_rule == "Random":
            while True:
                c = self._index(P)
                if c != i and c != a and c != b:
                    break
            parent = X[c]
        else:
            parent = X[int(s["Best Sample Index"])]
        rn = self._index(N)
        u = np.array([self.rng.uniform() for _ in range(N)])
        take = (u < s["Crossover Rate"]) | (np.arange(N) == rn)
        mut = parent + s["Mutation Rate"] * (X[a] - X[b])
        s["Candidate Population"][i] = np.where(take, mut, X[i])

    def _fix(self, i):  # fixInfeasible (:178-190)
        c, x = self.s["Candidate Population"][i], self.s["Sample Population"][i]
        length = np.zeros(self.N)
        length = np.where(c < self.lb, c - self.lb, length)
        length = np.where(c > self.ub, c - self.ub, length)
        u = np.array([self.rng.uniform() for _ in range(self.N)])
        self.s["Candidate Population"][i] = x - length * u

    # prepareGeneration (:99-116)
    def prepare(self, generation):
        s = self.s
        if generation > 1:
            s["Candidate Population"] = np.array(s["Candidate Population"], dtype=np.float64)
            for i in range(self.P):
                feasible, attempts = True, 0
                while True:
                    self._mutate(i)
                    if self.fix and not feasible:
                        self._fix(i)
                    feasible = self._feasible(s["Candidate Population"][i])
                    if feasible:
                        break
                    s["Infeasible Sample Count"] += 1
                    attempts += 1
                    if attempts > self.max_attempts:
                        raise RuntimeError("no feasible candidate")
        s["Previous Value Vector"] = np.array(s["Value Vector"], dtype=np.float64)

    def candidates(self):
        return self.s["Candidate Population"]

    # the evaluation loop of runGeneration (:70-82) + updateSolver (:192-278)
    def update(self, F):
        s, P, N = self.s, self.P, self.N
        s["Model Evaluation Count"] += P
        F = np.array(F, dtype=np.float64)
        X, C = s["Sample Population"], s["Candidate Population"]
        s["Value Vector"] = F
        best = int(np.argmax(F))  # first maximum, as std::max_element
        s["Best Sample Index"] = best
        s["Previous Best Ever Value"] = s["Best Ever Value"]
        s["Previous Best Value"] = s["Current Best Value"]
        s["Current Best Value"] = float(F[best])
        s["Current Best Variables"] = C[best].copy()
        s["Previous Mean"] = s["Current Mean"].copy()
        if s["Current Best Value"] > s["Best Ever Value"]:
            s["Best Ever Variables"] = C[best].copy()
        prev = s["Previous Value Vector"]
        rule = self.accept_rule
        if rule == "Best":
            if s["Current Best Value"] > s["Best Ever Value"]:
                X[best] = C[best]
                s["Best Ever Value"] = s["Current Best Value"]
        elif rule == "Greedy":  # against the previous generation's candidate value
            for i in range(P):
                if F[i] > prev[i]:
                    X[i] = C[i]
            if s["Current Best Value"] > s["Best Ever Value"]:
                s["Best Ever Value"] = s["Current Best Value"]
        elif rule == "Improved":
            for i in range(P):
                if F[i] > s["Best Ever Value"]:
                    X[i] = C[i]
            if s["Current Best Value"] > s["Best Ever Value"]:
                s["Best Ever Value"] = s["Current Best Value"]
        elif rule == "Iterative":
            for i in range(P):
                if F[i] > s["Best Ever Value"]:
                    X[i] = C[i]
                    s["Best Ever Value"] = float(F[i])
        else:
            raise ValueError("Accept Rule (%s) not recognized." % rule)
        s["Current Mean"] = self._mean()
        s["Max Distances"] = X.max(axis=0) - X.min(axis=0)
        # :276-277 resets the step size and discards std::min's result
        s["Current Minimum Step Size"] = INF

    def generation(self, generation, objective):
        if generation == 1:
            self.initialize()
        self.prepare(generation)
        self.update([objective(x) for x in self.candidates()])


def from_golden(gen, variables=None):
    """A DeaRef holding the recorded state of one generation file."""
    sv = gen["Solver"]
    vs = variables if variables is not None else gen["Variables"]
    r = DeaRef(len(vs), sv["Population Size"], [v["Lower Bound"] for v in vs], [v["Upper Bound"] for v in vs],
               sv["Crossover Rate"], sv["Mutation Rate"], sv["Mutation Rule"], sv["Parent Selection Rule"],
               sv["Accept Rule"], bool(sv["Fix Infeasible"]))
    for k in DeaRef.FIELDS:
        r[k] = sv[k]
    r.rng.load(sv["Uniform Generator"]["Range"])
    return r
