"""The matrix families of eigen_cases.py against the CPU oracle and NumPy.

test_gpu_eigen_forced.py compares the device eigensolver with the oracle bit
for bit; this file keeps that from being a comparison of two copies of one
mistake: the oracle's (ev, B) must be an eigendecomposition of M within the
backward error of a QR eigensolver, 16 N eps, and agree with LAPACK's
eigenvalues to the same bound.
"""
import numpy as np
import pytest

import eigen_cases as E
import refcpu as R

EPS = np.finfo(np.float64).eps
ORDERS = (1, 2, 3, 5, 17, 64, 65, 96, 129, 200)


@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("kind", E.KINDS)
def test_oracle_decomposes_family(kind, N):
    M = E.family(kind, N)
    assert M.shape == (N, N) and np.array_equal(M, M.T)
    ev, B = R.eigen_symmv(M)
    bound = 16 * N * EPS
    scale = np.max(np.abs(ev))
    residual = np.max(np.abs(M @ B - B * ev))  # (not divided: singular at N = 1 is the zero matrix)
    orthogonality = np.max(np.abs(B.T @ B - np.eye(N)))
    print("%s N=%d residual / max|ev| %.3g orthogonality %.3g bound %.3g"
          % (kind, N, residual / scale if scale else residual, orthogonality, bound))
    assert residual <= bound * scale
    assert orthogonality <= bound
    assert np.max(np.abs(np.sort(ev) - np.linalg.eigvalsh(M))) <= bound * scale


def test_families_are_seeded():
    for kind in E.KINDS:
        assert np.array_equal(E.family(kind, 17, 3), E.family(kind, 17, 3))
    assert not np.array_equal(E.family("graded", 17, 3), E.family("graded", 17, 4))


@pytest.mark.parametrize("N", ORDERS)
def test_zero_patterns(N):
    """The exact zeros the device tests rely on: block's off-diagonal blocks,
    zerocol's cleared row and column, diagplus's single pair."""
    assert E.zero_index("zerocol", N) == N // 3
    for kind, d in (("zerocol", 2.0), ("singular", 0.0)):
        M = E.family(kind, N)
        k = E.zero_index(kind, N)
        assert M[k, k] == d
        assert not np.any(np.delete(M[k], k)) and not np.any(np.delete(M[:, k], k))
    a = N // 3
    M = E.family("block", N)
    assert not np.any(M[:a, a:]) and not np.any(M[a:2 * a, 2 * a:])
    M = E.family("diagplus", N)
    off = M - np.diag(np.diag(M))
    assert np.count_nonzero(off) == (2 if N > 3 else 0)
    assert not np.any(E.family("diagonal", N) - np.diag(np.arange(1.0, N + 1.0)))


@pytest.mark.parametrize("N", ORDERS)
@pytest.mark.parametrize("kind", E.FAILING)
def test_oracle_counts_the_eigen_failure(kind, N):
    """min eigenvalue <= 0: one "Eigen Failures", B and D kept.  singular's
    minimum is exactly +-0.0 (the equality side of mn <= 0.0), no tolerance."""
    M = E.family(kind, N)
    ev, _ = R.eigen_symmv(M)
    if kind == "singular":
        assert np.min(ev) == 0.0
    else:
        assert np.min(ev) < 0.0
    o = R.CMAES(N, 8, 0)
    o["Initial Value"] = np.zeros(N)
    o["Initial Standard Deviation"] = np.ones(N)
    o.initialize()
    B0, D0 = o["Covariance Eigenvector Matrix"].copy(), o["Axis Lengths"].copy()
    mn0, mx0 = o["Minimum Covariance Eigenvalue"].copy(), o["Maximum Covariance Eigenvalue"].copy()
    assert o["Eigen Failures"][0] == 0.0
    o["Covariance Matrix"] = M
    o.prepare()
    assert o["Eigen Failures"][0] == 1.0
    assert np.array_equal(o["Covariance Eigenvector Matrix"], B0) and np.array_equal(o["Axis Lengths"], D0)
    assert np.array_equal(o["Minimum Covariance Eigenvalue"], mn0)
    assert np.array_equal(o["Maximum Covariance Eigenvalue"], mx0)
