"""The numerics every solver shares (korali_amd/csrc/kg_gsl.hpp) without a
solver around them: the workgroup Cholesky (kg_debug_cholesky) against the
oracle's kr_cholesky, and the univariate priors' log-densities
(kg_debug_prior_logdens) against tests/nested_ref.py.  Every comparison is on
the bits."""
import ctypes

import numpy as np
import pytest

import nested_ref as nr
from oracle import refcpu
from test_gpu_tmcmc import PRIOR_SETS

pytestmark = pytest.mark.gpu


def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ Cholesky
def device_cholesky(A):
    from korali_amd.native import lib
    A = np.ascontiguousarray(A, dtype=np.float64)
    out = np.zeros_like(A)
    failed = ctypes.c_int(-1)
    assert lib().kg_debug_cholesky(0, A.shape[0], _vp(A), _vp(out), ctypes.byref(failed)) == 0
    return failed.value, out


def positive_definite(N):
    M = np.random.default_rng(1000 + N).standard_normal((N, N))
    return M @ M.T + N * np.eye(N)


def check_against_oracle(A, want_status):
    """flag and lower triangle as kr_cholesky leaves them, upper triangle untouched"""
    N = A.shape[0]
    st, F = refcpu.cholesky(A)
    assert (st != 0) == want_status
    failed, out = device_cholesky(A)
    assert failed == (1 if want_status else 0)
    il, iu = np.tril_indices(N), np.triu_indices(N, 1)
    assert np.array_equal(bits(out)[il], bits(F)[il])
    assert np.array_equal(bits(out)[iu], bits(A)[iu])
    return out


# 120 and 128: the TMCMC and MOCMAES caps; 63..65 around one wavefront of rows
@pytest.mark.parametrize("N", [1, 2, 3, 63, 64, 65, 120, 128])
def test_cholesky_positive_definite(N):
    out = check_against_oracle(positive_definite(N), False)
    assert np.all(np.isfinite(out)) and np.all(np.diag(out) > 0)


@pytest.mark.parametrize("column,pivot", [(0, 0.0), (0, -1.0), (2, -1.0), (4, -1.0)])
def test_cholesky_stops_at_a_non_positive_pivot(column, pivot):
    """GSL's partial factor (error handler off): columns before `column`
    factored, column `column` updated and not scaled, the rest as they were"""
    A = positive_definite(5)
    A[column, column] = pivot  # the pivot is this minus a sum of squares
    out = check_against_oracle(A, True)
    assert out[column, column] <= 0.0
    assert np.array_equal(bits(out[column + 1:, column + 1:]), bits(A[column + 1:, column + 1:]))


def test_cholesky_nan_pivot_is_no_failure():
    """`ajj <= 0.0` is false for a NaN: the factorisation runs to the end and
    the NaN spreads through every later column"""
    A = positive_definite(5)
    A[2, 2] = np.nan
    out = check_against_oracle(A, False)
    assert np.all(np.isfinite(out[:, :2])) and np.all(np.isnan(out[2:, 2:][np.tril_indices(3)]))


# -------------------------------------------------------------------- priors
# kind -> (a, b): PRIOR_SETS["all"] has Exponential, Laplace, Cauchy, LogNormal
# and Normal; the Uniform is PRIOR_SETS["normal"]'s
def prior_parameters():
    out = {}
    for name in ("normal", "all"):
        _, kinds, pmin, pmax = PRIOR_SETS[name]
        for k, a, b in zip(kinds, pmin, pmax):
            out.setdefault(k, (a, b))
    return out


PRIORS = prior_parameters()


def test_prior_parameters_cover_the_six_kinds():
    assert sorted(PRIORS) == [0, 1, 2, 3, 4, 5]


def prior_points(a, b):
    inf = np.inf
    x = [a, b, np.nextafter(a, -inf), np.nextafter(a, inf), np.nextafter(b, -inf), np.nextafter(b, inf),
         0.0, 5e-324, -1.0, 1e300, -1e300, inf, -inf]
    return np.array(x, dtype=np.float64)


@pytest.mark.parametrize("kind", sorted(nr.KINDS.values()), ids=sorted(nr.KINDS, key=nr.KINDS.get))
def test_prior_logdens_equals_the_restatement(kind):
    from korali_amd.native import lib
    a, b = PRIORS[kind]
    ref = nr.NestedRef(1, 4, [a], [b], method="Box", prior_kinds=[kind], lower_bound=[0.0], upper_bound=[1.0])
    x = prior_points(a, b)
    want = np.array([ref._logdens(0, float(v)) for v in x], dtype=np.float64)
    got = np.full(x.size, 123.0)
    cn = ctypes.c_double(123.0)
    assert lib().kg_debug_prior_logdens(0, kind, a, b, _vp(x), x.size, ctypes.byref(cn), _vp(got)) == 0
    assert bits(np.array([cn.value])) == bits(np.array([ref.cst[0]]))
    for v, g, w in zip(x, got, want):
        print("kind %d x %r device %r (%016x) restatement %r (%016x)" % (kind, v, g, bits([g])[0], w, bits([w])[0]))
    assert np.array_equal(bits(got), bits(want))  # NaNs compare as their bits
