"""The "MFMA" covariance update (k_rankmu_tile on v_mfma_f64_16x16x4f64, then
k_adaptC_combine, or k_part_reduce and the caller's sum all-reduce when
sharded) against the exact rational result, element by element, at the shapes
where each piece of the kernel's geometry first exists.

Every element of the lower triangle must lie within rankmu_ref's derived
bound of the exact value (tests/rankmu_ref.py: the any-order summation bound,
not a measured figure), and the upper triangle must mirror it bit for bit.
The worst err/tol of each case is printed.

Data families:
  sampled  rows m + sigma L z, m random O(1);
  offset   m = 1e6 with a spread of 1e-3 (a reordering that multiplies before
           centring loses ~1e-7 relative here);
  marker   selected row k is m except column k mod N, which is m + (k + 1);
           the last selected row also in column N-1, the first in column 0;
           unselected rows are junk (1e3).  A dropped, duplicated,
           mis-weighted or unselected row moves an identifiable element by
           O(1) relative; elements no row contributes to keep the base term.
"""
import numpy as np
import pytest

import rankmu_ref as RR

pytestmark = pytest.mark.gpu

# (N, lambda, mu): the smallest shapes at which each piece of geometry exists
SHAPES = [
    (1, 8, 4),         # odd N, a single element
    (2, 10, 3),        # mu < 4; per rounds 1 -> 4; seven empty slices
    (15, 40, 20),      # odd N < 16
    (16, 66, 33),      # per = 8; a slice with one row; slices 5-7 empty
    (17, 64, 32),      # odd N
    (63, 130, 65),     # odd N
    (64, 128, 64),
    (65, 258, 129),    # a second 64-tile row with one column; odd N
    (129, 70, 35),     # six 64-tiles; N > mu
    (130, 600, 300),   # per = 40: one 32-row chunk and a partial one per slice
]
LARGE = [
    (18, 8200, 4100),    # 16 slices; per = 260; the last slice short
    (33, 16390, 8195),   # 32 slices; odd N
]
FAMILIES = ["sampled", "offset", "marker"]
TWO = [(17, 64), (65, 258)]


def spd(rng, N):
    A = rng.standard_normal((N, N))
    C = A @ A.T / N + 0.5 * np.eye(N)
    return np.tril(C) + np.tril(C, -1).T  # symmetric bit for bit


def fitness(rng, lam):
    """A random permutation (larger is better) with a run of ties, which the
    sort resolves by index."""
    F = rng.permutation(lam).astype(np.float64)
    a = int(rng.integers(0, max(1, lam - 4)))
    F[a:a + 3] = F[int(rng.integers(0, lam))]
    return F


def ranking(F):
    return np.lexsort((np.arange(F.size), -F))


def population(rng, family, N, lam, mu, idx, m, sigma, C_old):
    if family == "sampled":
        L = np.linalg.cholesky(C_old)
        return m + sigma * rng.standard_normal((lam, N)) @ L.T
    if family == "offset":
        return m + 1e-3 * rng.standard_normal((lam, N))
    assert family == "marker"
    X = np.full((lam, N), 1e3)
    for k in range(mu):
        row = m.copy()
        row[k % N] += k + 1
        X[idx[k]] = row
    X[idx[mu - 1], N - 1] = m[N - 1] + mu
    X[idx[0], 0] = m[0] + 1
    return X


def family_mean(rng, family, N):
    return np.full(N, 1e6) if family == "offset" else rng.uniform(-2.0, 2.0, N)


def make_device(N, lam, **kw):
    from korali_amd.native import CmaesDevice
    kw.setdefault("cov_mode", "mfma")
    dev = CmaesDevice(N, lam, initial_value=np.zeros(N), initial_std=np.ones(N), normal_seed=11, uniform_seed=12, **kw)
    dev.initialize()
    return dev


def write_state(dev, X, m, C_old, sigma):
    dev["Sample Population"] = X
    dev["Current Mean"] = m
    dev["Covariance Matrix"] = C_old
    dev["Sigma"] = [sigma]


def reference_inputs(dev, N, X, idx, sigma, C_old):
    """The inputs of the exact reference, read from the handle after the update."""
    mu = dev.mu
    return dict(N=N, Xsel=X[idx[:mu]], w=dev["Mu Weights"], m_prev=dev["Previous Mean"], sigma=sigma, C_old=C_old,
                pc=dev["Evolution Path"], hsig=dev["Hsig"][0], cc=dev["Cumulative Covariance"][0],
                mueff=dev["Effective Mu"][0])


def one_update(dev, rng, family, N, lam, gen=1, sigma=0.7, label="", diagonal=False):
    """Write a state, run one update, check every element; returns the worst err/tol."""
    mu = dev.mu
    F = fitness(rng, lam)
    idx = ranking(F)
    m = family_mean(rng, family, N)
    C_in = spd(rng, N)
    X = population(rng, family, N, lam, mu, idx, m, sigma, C_in)
    write_state(dev, X, m, C_in, sigma)
    sigma_d, C_old = float(dev["Sigma"][0]), dev["Covariance Matrix"].reshape(N, N)
    assert sigma_d == sigma and np.array_equal(C_old, C_in)
    dev.set_fitness(F)
    dev.update(gen)
    dev.synchronize()
    assert np.array_equal(dev.sorting_index(), idx)
    assert np.array_equal(dev["Sample Population"].reshape(lam, N), X)
    assert np.array_equal(dev["Previous Mean"], m)
    C = dev["Covariance Matrix"].reshape(N, N)
    ref = RR.covariance(**reference_inputs(dev, N, X, idx, sigma_d, C_old))
    r = ref.ratios(C)
    worst = float(np.diag(r).max() if diagonal else r.max())
    print(f"rankmu mfma {label or family} N={N} lam={lam} mu={mu} gen={gen}: worst err/tol {worst:.4f}")
    if diagonal:
        off = ~np.eye(N, dtype=bool)
        assert np.all(np.diag(r) <= 1.0), (np.diag(r).max(), int(np.argmax(np.diag(r))))
        assert np.array_equal(C[off], C_old[off]), "diagonal covariance: an off-diagonal element changed"
        return float(np.diag(r).max())
    assert np.all(r <= 1.0), (worst, np.unravel_index(np.argmax(r), r.shape))
    assert np.array_equal(C, C.T), "upper triangle is not the mirror of the lower one"
    return worst


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,lam,mu", SHAPES)
def test_covariance_elementwise(N, lam, mu, family):
    dev = make_device(N, lam, mu=mu)
    assert dev.mu == mu
    try:
        one_update(dev, np.random.default_rng(1000 * N + lam), family, N, lam)
    finally:
        dev.close()


@pytest.mark.parametrize("N,lam,mu", LARGE)
def test_covariance_elementwise_many_slices(N, lam, mu):
    dev = make_device(N, lam, mu=mu)
    try:
        one_update(dev, np.random.default_rng(N + lam), "sampled", N, lam)
    finally:
        dev.close()


@pytest.mark.parametrize("mu_type", ["Equal", "Linear", "Proportional"])
@pytest.mark.parametrize("family", ["sampled", "marker"])
@pytest.mark.parametrize("N,lam", TWO)
def test_mu_types(N, lam, family, mu_type):
    """Weights and mu_eff are read after the update: Proportional weights are
    rewritten by k_update_best in the update that uses them."""
    dev = make_device(N, lam, mu_type=mu_type)
    try:
        one_update(dev, np.random.default_rng(7 * N + len(mu_type)), family, N, lam, label=f"{mu_type}/{family}")
        w = dev["Mu Weights"]
        assert np.all(w > 0)
        if mu_type == "Equal":
            assert np.all(w == w[0])
    finally:
        dev.close()


@pytest.mark.parametrize("family", ["sampled", "marker"])
@pytest.mark.parametrize("N,lam,mu", [(17, 64, 5), (65, 258, 31)])
def test_explicit_mu(N, lam, mu, family):
    dev = make_device(N, lam, mu=mu)
    try:
        one_update(dev, np.random.default_rng(N * mu), family, N, lam, label=f"mu={mu}/{family}")
    finally:
        dev.close()


@pytest.mark.parametrize("family", ["sampled", "marker"])
@pytest.mark.parametrize("N,lam", TWO)
def test_diagonal_covariance(N, lam, family):
    """The diagonal within tol, every off-diagonal element untouched."""
    dev = make_device(N, lam, diagonal=True)
    try:
        one_update(dev, np.random.default_rng(N + 5), family, N, lam, label=f"diagonal/{family}", diagonal=True)
    finally:
        dev.close()


@pytest.mark.parametrize("sigma", [3e-7, 2e5])
@pytest.mark.parametrize("N,lam", TWO)
def test_extreme_sigma(N, lam, sigma):
    dev = make_device(N, lam)
    try:
        one_update(dev, np.random.default_rng(N + 9), "sampled", N, lam, sigma=sigma, label=f"sigma={sigma:g}")
    finally:
        dev.close()


@pytest.mark.parametrize("N,lam", TWO)
def test_two_consecutive_updates(N, lam):
    """Different data and fitness in each: stale partial sums (covPart) or a
    mis-reused evY / evC event would show in the second."""
    dev = make_device(N, lam)
    rng = np.random.default_rng(N + 21)
    try:
        one_update(dev, rng, "sampled", N, lam, gen=1, label="first")
        one_update(dev, rng, "marker", N, lam, gen=2, sigma=1.3, label="second/marker")
        one_update(dev, rng, "offset", N, lam, gen=3, sigma=0.2, label="third/offset")
    finally:
        dev.close()


# ---------------------------------------------------------------- sharded
def shard_fitness(rng, pattern, S, lam, mu):
    """random; none: the mu best all lie outside the last rank's rows; one:
    exactly one of them inside."""
    F = fitness(rng, lam)
    if pattern == "random":
        return F
    per = lam // S
    last = np.arange((S - 1) * per, lam)
    others = np.arange(0, (S - 1) * per)
    assert others.size >= mu
    F = np.empty(lam)
    F[others] = rng.permutation(others.size) + 10.0 * lam  # every one of them beats the last rank's
    F[last] = rng.permutation(last.size)
    a = int(others[3])
    F[a:a + 3] = F[a]  # ties among the selected
    if pattern == "one":
        F[last[per // 2]] = 20.0 * lam  # the best of all: selection rank 0
    return F


@pytest.mark.parametrize("pattern", ["random", "none", "one"])
@pytest.mark.parametrize("S,N,lam", [(2, 17, 64), (3, 65, 258), (4, 130, 600)])
def test_sharded_partials_single_process(S, N, lam, pattern):
    """S handles on one device play the ranks; the sum all-reduce of the
    "Shard Partials" is a NumPy sum in rank order, written to every handle as
    the host transport does."""
    rng = np.random.default_rng(100 * S + N + len(pattern))
    devs = [make_device(N, lam, shard_rank=r, shard_count=S) for r in range(S)]
    try:
        mu = devs[0].mu
        F = shard_fitness(rng, pattern, S, lam, mu)
        idx = ranking(F)
        per = lam // S
        owned = [int(np.sum((idx[:mu] >= r * per) & (idx[:mu] < (r + 1) * per))) for r in range(S)]
        if pattern == "none":
            assert owned[-1] == 0
        if pattern == "one":
            assert owned[-1] == 1
        sigma = 0.7
        m = family_mean(rng, "sampled", N)
        C_in = spd(rng, N)
        X = population(rng, "sampled", N, lam, mu, idx, m, sigma, C_in)
        for d in devs:
            write_state(d, X, m, C_in, sigma)
            d["Value Vector"] = F
        sigma_d, C_old = float(devs[0]["Sigma"][0]), devs[0]["Covariance Matrix"].reshape(N, N)
        for d in devs:
            d.update_partial(1)
        parts = []
        for d in devs:
            d.synchronize()
            parts.append(d["Shard Partials"])
        total = parts[0].copy()
        for p in parts[1:]:
            total = total + p
        for d in devs:
            d["Shard Partials"] = total
            d.update_finalize(1)
        for d in devs:
            d.synchronize()
        d0 = devs[0]
        assert np.array_equal(d0.sorting_index(), idx)
        C = d0["Covariance Matrix"].reshape(N, N)
        ref = RR.covariance(**reference_inputs(d0, N, X, idx, sigma_d, C_old), extra=S)
        r = ref.ratios(C)
        rm = RR.mean(N, X[idx[:mu]], d0["Mu Weights"], extra=S).ratios(d0["Current Mean"])
        print(f"rankmu mfma sharded S={S} N={N} lam={lam} {pattern} owned={owned}: worst err/tol "
              f"C {r.max():.4f} mean {rm.max():.4f}")
        assert np.all(r <= 1.0), (float(r.max()), np.unravel_index(np.argmax(r), r.shape))
        assert np.array_equal(C, C.T)
        assert np.all(rm <= 1.0), float(rm.max())
        assert np.array_equal(d0["Current Best Variables"], X[idx[0]])
        for d in devs[1:]:
            for key in ("Current Mean", "Covariance Matrix", "Sigma"):
                assert np.array_equal(d[key], d0[key]), (key, d.shard_rank)
    finally:
        for d in devs:
            d.close()
