"""tests/hier_theta_ref.py (the restatement of the Hierarchical/Theta
log-likelihood, theta.cpp.base:59-124) in closed form at M = K = 1, against an
independent NumPy / SciPy formulation, and at a -inf denominator.

The bound of the independent check is test_hier_ref_cpu.py's for ThetaNew
(BOUND = 1e-12, relative): it is there to catch a wrong formula, not rounding."""
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.special
import scipy.stats

import hier_ref as H
import hier_theta_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12  # test_hier_ref_cpu.py: BOUND, as test_theta_new_against_mpmath applies it


@pytest.fixture(scope="module", autouse=True)
def oracle_library():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


@pytest.mark.parametrize("libm", [False, True])
@pytest.mark.parametrize("sub_ll", [-3.25, None])
def test_closed_form_at_one_row_each(libm, sub_ll):
    log, _ = H.functions(libm)
    a, b, s, lp, x = 0.3, 1.7, -0.45, -2.125, 0.9
    kinds, index, const = [H.NORMAL], [[0, 1]], [[0.0, 0.0]]
    psi_db, sub_db, lps = [[a, b]], [[s]], [lp]
    cn = H.prior_const(H.NORMAL, a, b, log)
    log_n = lambda v: H.log_density(H.NORMAL, v, a, b, cn, log)
    den = T.theta_denominators(kinds, index, const, psi_db, sub_db, lps, libm=libm)
    assert den == [log_n(s) - lp]
    got = T.theta_loglik([x], sub_ll, kinds, index, const, psi_db, sub_db, lps, libm=libm)
    assert got == (0.0 if sub_ll is None else sub_ll) + (log_n(x) - den[0])
    # den handed over: the same double
    assert got == T.theta_loglik([x], sub_ll, kinds, index, const, psi_db, den=den, libm=libm)


# all six kinds; Psi database columns supply every parameter but two constants
KINDS = [H.UNIFORM, H.NORMAL, H.EXPONENTIAL, H.LAPLACE, H.CAUCHY, H.LOGNORMAL]
INDEX = [[0, 1], [2, 3], [-1, 4], [5, -1], [6, 7], [8, 9]]
CONST = [[0.0, 0.0], [0.0, 0.0], [-0.5, 0.0], [0.0, 1.3], [0.0, 0.0], [0.0, 0.0]]


def scipy_logpdf(kind, x, a, b):
    st = scipy.stats
    if kind == H.UNIFORM:
        return st.uniform.logpdf(x, loc=a, scale=b - a)
    if kind == H.NORMAL:
        return st.norm.logpdf(x, loc=a, scale=b)
    if kind == H.EXPONENTIAL:
        return st.expon.logpdf(x, loc=a, scale=b)
    if kind == H.LAPLACE:
        return st.laplace.logpdf(x, loc=a, scale=b)
    if kind == H.CAUCHY:
        return st.cauchy.logpdf(x, loc=a, scale=b)
    return st.lognorm.logpdf(x, s=b, scale=np.exp(a))


def inputs(M, K, seed):
    rng = np.random.default_rng(seed)
    psi = rng.normal(0.0, 0.7, (M, 10))
    for ib in (1, 3, 4, 7, 9):
        psi[:, ib] = rng.uniform(0.4, 2.5, M)
    psi[:, 0], psi[:, 1] = rng.uniform(-6.0, -4.0, M), rng.uniform(4.0, 6.0, M)

    def points(n):
        cols = [rng.normal(0.0, 1.0, n) for _ in KINDS]
        cols[2] = rng.uniform(0.2, 3.0, n)
        cols[5] = np.exp(rng.normal(0.0, 0.5, n))
        return np.stack(cols, axis=1)

    return psi, points(K), rng.uniform(-8.0, -0.5, K), points(3), rng.uniform(-9.0, -1.0, 3)


@pytest.mark.parametrize("K", [1, 7, 300])
@pytest.mark.parametrize("M", [1, 7, 300])
def test_against_scipy(M, K):
    psi, sub, lps, X, sub_ll = inputs(M, K, 1000 * M + K)
    par = np.array([[[r[i] if i >= 0 else c for i, c in zip(ix, cs)] for ix, cs in zip(INDEX, CONST)] for r in psi])
    # den_i = -log K + logsumexp_j( sum_k logpdf_k(S_jk | psi_i) - lpS_j )
    w = sum(scipy_logpdf(kd, sub[None, :, k], par[:, k, 0, None], par[:, k, 1, None]) for k, kd in enumerate(KINDS))
    den = -np.log(K) + scipy.special.logsumexp(w - lps[None, :], axis=1)
    got_den = T.theta_denominators(KINDS, INDEX, CONST, psi, sub, lps, libm=True)
    r = np.max(np.abs(np.array(got_den) - den) / np.abs(den))
    print("theta den M=%d K=%d relative difference %.3e" % (M, K, r))
    assert r <= BOUND
    for x, s in zip(X, sub_ll):
        v = sum(scipy_logpdf(kd, x[k], par[:, k, 0], par[:, k, 1]) for k, kd in enumerate(KINDS))
        want = s - np.log(M) + scipy.special.logsumexp(v - den)
        got = T.theta_loglik(x, s, KINDS, INDEX, CONST, psi, sub, lps, libm=True)
        r = abs(got - want) / abs(want)
        print("theta M=%d K=%d relative difference %.3e" % (M, K, r))
        assert r <= BOUND


@pytest.mark.parametrize("libm", [False, True])
def test_minus_inf_denominator(libm):
    # Psi row 1's Uniform holds none of the sub-samples: every w_j is -inf and
    # so is den_1.  A point outside that row's support: (-inf) - (-inf) is a NaN
    # term beside finite ones, the sum of exponentials is NaN.  A point inside
    # it: the term is +inf and logSumExp returns the +inf maximum.
    kinds, index, const = [H.UNIFORM], [[0, 1]], [[0.0, 0.0]]
    psi_db = [[-1.0, 1.0], [5.0, 6.0], [-2.0, 2.0]]
    sub_db, lps = [[0.5], [-0.25], [0.75]], [-1.0, -1.5, -2.0]
    den = T.theta_denominators(kinds, index, const, psi_db, sub_db, lps, libm=libm)
    assert math.isfinite(den[0]) and den[1] == -math.inf and math.isfinite(den[2])
    assert math.isnan(T.theta_loglik([0.1], -1.0, kinds, index, const, psi_db, sub_db, lps, libm=libm))
    assert T.theta_loglik([5.5], -1.0, kinds, index, const, psi_db, sub_db, lps, libm=libm) == math.inf
