"""tests/hier_ref.py (the restatement of the Hierarchical/Psi and /ThetaNew
log-likelihoods) against an independent mpmath evaluation at 200 bits, each
density in closed form, and the inf / NaN rules of logSumExp
(auxiliar/math.hpp:205-225).  The bound (relative 1e-12) is there to catch a
wrong formula, not rounding."""
import math
import os
import subprocess

import mpmath
import numpy as np
import pytest

import hier_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-12


@pytest.fixture(scope="module", autouse=True)
def oracle_library():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def mp_density(kind, x, a, b):
    mp = mpmath.mp
    x, a, b = mp.mpf(x), mp.mpf(a), mp.mpf(b)
    if kind == H.NORMAL:
        return -mp.log(b * mp.sqrt(2 * mp.pi)) - (x - a) ** 2 / (2 * b * b)
    if kind == H.LOGNORMAL:
        return -mp.log(x * b * mp.sqrt(2 * mp.pi)) - (mp.log(x) - a) ** 2 / (2 * b * b)
    raise AssertionError(kind)


def mp_lse(values):
    mp = mpmath.mp
    return mp.log(mp.fsum(mp.exp(v) for v in values))


def make_inputs(K, seed):
    rng = np.random.default_rng(seed)
    kinds = [H.NORMAL, H.LOGNORMAL]
    groups, lps = [], []
    for g in range(3):
        x0 = rng.normal(0.5 * g, 1.5, K)
        x1 = np.exp(rng.normal(0.2, 0.6, K))
        groups.append(np.stack([x0, x1], axis=1))
        lps.append(rng.uniform(-6.0, -1.0, K))
    return kinds, groups, lps


# Psi: variables (mean, sd, mu) feed the Normal and the LogNormal's Mu; Sigma is a constant
PSI_INDEX = [[0, 1], [2, -1]]
PSI_CONST = [[0.0, 0.0], [0.0, 0.7]]
PSI_POINT = [0.3, 1.7, -0.1]


def rel(a, b):
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("K", [1, 64, 257])
@pytest.mark.parametrize("libm", [False, True])
def test_psi_against_mpmath(K, libm):
    mpmath.mp.prec = 200
    kinds, groups, lps = make_inputs(K, 100 + K)
    got = H.psi_loglik(PSI_POINT, kinds, PSI_INDEX, PSI_CONST, groups, lps, libm=libm)
    par = [(PSI_POINT[0], PSI_POINT[1]), (PSI_POINT[2], 0.7)]
    want = mpmath.mpf(0)
    for rows, lp in zip(groups, lps):
        want += mp_lse([-mpmath.mpf(float(lp[j])) + sum(mp_density(kinds[k], float(rows[j][k]), *par[k])
                                                        for k in range(2)) for j in range(K)])
    r = rel(mpmath.mpf(got), want)
    print("psi K=%d libm=%s relative difference %.3e" % (K, libm, float(r)))
    assert r <= BOUND


@pytest.mark.parametrize("K", [1, 64, 257])
@pytest.mark.parametrize("libm", [False, True])
def test_theta_new_against_mpmath(K, libm):
    mpmath.mp.prec = 200
    rng = np.random.default_rng(7 + K)
    kinds = [H.NORMAL, H.LOGNORMAL]
    # database columns: mean, sd, mu, sigma
    db = np.stack([rng.normal(0, 1, K), rng.uniform(0.5, 2, K), rng.normal(0, 0.3, K), rng.uniform(0.4, 1, K)], axis=1)
    index, const = [[0, 1], [2, 3]], [[0.0, 0.0], [0.0, 0.0]]
    point = [0.4, 1.3]
    got = H.theta_new_loglik(point, kinds, index, const, db, libm=libm)
    want = -mpmath.log(K) + mp_lse([mp_density(H.NORMAL, point[0], float(r[0]), float(r[1])) +
                                    mp_density(H.LOGNORMAL, point[1], float(r[2]), float(r[3])) for r in db])
    r = rel(mpmath.mpf(got), want)
    print("thetaNew K=%d libm=%s relative difference %.3e" % (K, libm, float(r)))
    assert r <= BOUND


@pytest.mark.parametrize("K", [1, 64, 257])
def test_libm_variant_agrees_with_cr(K):
    kinds, groups, lps = make_inputs(K, 200 + K)
    a = H.psi_loglik(PSI_POINT, kinds, PSI_INDEX, PSI_CONST, groups, lps)
    b = H.psi_loglik(PSI_POINT, kinds, PSI_INDEX, PSI_CONST, groups, lps, libm=True)
    assert abs(a - b) / abs(a) <= BOUND


@pytest.mark.parametrize("libm", [False, True])
def test_log_sum_exp_inf_and_nan_rules(libm):
    inf, nan = math.inf, math.nan
    assert H.log_sum_exp([-inf, -inf, -inf], libm) == -inf
    assert H.log_sum_exp([0.5, inf, -1.0], libm) == inf
    assert H.log_sum_exp([nan, inf], libm) == inf  # NaN never wins `>`: the max decides first
    assert math.isnan(H.log_sum_exp([1.0, nan, 0.0], libm))
    assert math.isnan(H.log_sum_exp([nan, 1.0], libm))
    assert H.log_sum_exp([-inf, 2.0, -inf], libm) == 2.0
    assert H.log_sum_exp([], libm) == -inf


def test_group_of_minus_inf_and_single_terms():
    # a LogNormal x <= 0 and an Exponential below its location are -inf terms;
    # a group made only of them is -inf, and so is the sum over groups
    kinds = [H.LOGNORMAL, H.EXPONENTIAL]
    index, const = [[0, 1], [-1, 2]], [[0.0, 0.0], [1.0, 0.0]]
    point = [0.1, 0.8, 2.0]
    ok = np.array([[1.5, 1.2], [0.7, 3.0]])
    dead = np.array([[-1.0, 1.2], [0.7, 0.5], [0.0, 0.0]])
    lp = [np.array([-1.0, -2.0]), np.array([-1.0, -2.0, -3.0])]
    assert math.isfinite(H.psi_loglik(point, kinds, index, const, [ok, ok], [lp[0], lp[0]]))
    assert H.psi_loglik(point, kinds, index, const, [ok, dead], lp) == -math.inf
    mixed = np.array([[1.5, 1.2], [-1.0, 1.2], [0.7, 0.5]])
    assert math.isfinite(H.psi_loglik(point, kinds, index, const, [ok, mixed], lp))


def test_uniform_without_width():
    # Maximum - Minimum <= 0: the constant is NaN (uniform.cpp.base:38-44), but
    # only x = Minimum = Maximum is inside.  Psi: every other row is -inf, the
    # max stays -inf and so does the result; ThetaNew: one such row among rows
    # that hold the point is a NaN term that is not the maximum
    kinds = [H.UNIFORM]
    groups = [np.array([[1.5], [2.0]]), np.array([[1.2]])]
    lps = [np.array([-1.0, -1.0]), np.array([-1.0])]
    assert H.psi_loglik([2.0, 2.0], kinds, [[0, 1]], [[0.0, 0.0]], groups, lps) == -math.inf
    db = np.array([[0.0, 3.0], [2.0, 2.0], [1.0, 4.0]])
    assert math.isnan(H.theta_new_loglik([2.0], kinds, [[0, 1]], [[0.0, 0.0]], db))
    assert math.isfinite(H.theta_new_loglik([2.5], kinds, [[0, 1]], [[0.0, 0.0]], db))
