"""rankmu_ref (the exact adaptC reference and its derived bound) against the
CPU oracle's sequential update: the oracle's exact-order sum obeys the same
any-order bound, so every element of its covariance lies within tol of the
exact value; a reference fed one selected row too few must not."""
import numpy as np
import pytest

import rankmu_ref as RR
import refcpu as R


def oracle_update(N, lam, mu, x0=0.0, s0=1.0, diagonal=False, seed=77):
    """One oracle generation with a random (tied) fitness; the inputs of its
    adaptC and the covariance it produced."""
    o = R.CMAES(N, lam, mu)
    o["Initial Value"] = np.full(N, x0)
    o["Initial Standard Deviation"] = np.full(N, s0)
    if diagonal:
        o.option("Diagonal Covariance", 1)
    R.lib().kr_rng_seed(o.rng(0).ptr, seed)
    R.lib().kr_rng_seed(o.rng(1).ptr, seed + 1)
    o.initialize()
    o.prepare()
    o.sample()
    rng = np.random.default_rng(seed)
    F = rng.permutation(lam).astype(np.float64)
    F[1:3] = F[0]  # ties
    o["Value Vector"] = F
    sigma, C_old = float(o["Sigma"][0]), o["Covariance Matrix"].copy().reshape(N, N)
    o.update(1)
    idx = o.sorting_index()[:o.mu]
    X = o["Sample Population"].reshape(lam, N)
    return dict(N=N, Xsel=X[idx].copy(), w=o["Mu Weights"].copy(), m_prev=o["Previous Mean"].copy(), sigma=sigma,
                C_old=C_old, pc=o["Evolution Path"].copy(), hsig=o["Hsig"][0], cc=o["Cumulative Covariance"][0],
                mueff=o["Effective Mu"][0]), o["Covariance Matrix"].copy().reshape(N, N), o["Current Mean"].copy()


CASES = [(2, 10, 3, 0.0, 1.0), (17, 64, 32, 0.0, 1.0), (17, 64, 32, 1e6, 1e-3), (65, 258, 129, 0.0, 1.0)]


@pytest.mark.parametrize("N,lam,mu,x0,s0", CASES)
def test_oracle_covariance_within_derived_bound(N, lam, mu, x0, s0):
    args, C, mean = oracle_update(N, lam, mu, x0, s0)
    ref = RR.covariance(**args)
    r = ref.ratios(C)
    print(f"adaptC oracle N={N} lam={lam} mu={mu} x0={x0}: worst err/tol {r.max():.4f}")
    assert np.all(r <= 1.0), (r.max(), np.unravel_index(np.argmax(r), r.shape))
    assert np.array_equal(C, C.T)
    # the double-rounded exact value is what the integers say
    assert np.all(np.abs(C - ref.want)[np.tril_indices(N)] <= 1.0000001 * ref.tol[np.tril_indices(N)])
    rm = RR.mean(N, args["Xsel"], args["w"]).ratios(mean)
    print(f"mean   oracle N={N}: worst err/tol {rm.max():.4f}")
    assert np.all(rm <= 1.0), rm.max()


def test_oracle_diagonal_covariance_within_derived_bound():
    N, lam, mu = 17, 64, 32
    args, C, _ = oracle_update(N, lam, mu, diagonal=True)
    r = RR.covariance(**args).ratios(C)
    assert np.all(np.diag(r) <= 1.0), np.diag(r).max()
    off = ~np.eye(N, dtype=bool)
    assert np.array_equal(C[off], args["C_old"][off])


@pytest.mark.parametrize("N,lam,mu", [(2, 10, 3), (17, 64, 32)])
def test_dropped_row_is_rejected(N, lam, mu):
    """The bound is sharp enough to see one selected row (the last, with the
    smallest weight) missing from the sum."""
    args, C, mean = oracle_update(N, lam, mu)
    args["Xsel"], args["w"] = args["Xsel"][:-1], args["w"][:-1]
    r = RR.covariance(**args).ratios(C)
    assert r.max() > 1e3, r.max()
    assert RR.mean(N, args["Xsel"], args["w"]).ratios(mean).max() > 1e3


def test_exactness_of_the_integer_arithmetic():
    """Values a double sum loses: 2^60 + 1 - 2^60 survives, and a zero bound
    demands equality."""
    N = 2
    Xsel = np.array([[2.0 ** 30, 1.0], [1.0, 0.0], [-(2.0 ** 30), 1.0]])
    w = np.array([0.5, 0.25, 0.25])
    ref = RR.covariance(N, Xsel, w, np.zeros(N), 1.0, np.zeros((N, N)), np.zeros(N), 1, 0.5, 2.0)
    _, cmu = RR.ccov(N, 2.0)
    from fractions import Fraction
    S = {(0, 0): 3 * 2 ** 58 + Fraction(1, 4), (1, 0): Fraction(2 ** 28), (1, 1): Fraction(3, 4)}
    for (d, e), s in S.items():
        assert Fraction(int(ref.num[d, e]), ref.den << ref.K) == Fraction(cmu) * s
    # no contributing row and no base term: tol == 0, only the exact value passes
    Z = RR.covariance(N, np.zeros((3, N)), w, np.zeros(N), 1.0, np.zeros((N, N)), np.zeros(N), 1, 0.5, 2.0)
    assert np.all(Z.tol == 0) and Z.ratios(np.zeros((N, N))).max() == 0.0
    assert np.isinf(Z.ratios(np.full((N, N), 1e-300))[1, 0])
