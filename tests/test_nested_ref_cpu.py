"""The NumPy restatement of Sampler/Nested (tests/nested_ref.py): invariants
of a run, and the evidence and posterior of a Gaussian with a known answer.
CPU only."""
import math

import numpy as np
import pytest

import nested_ref as nr


def permutation(seed, n):
    """any fixed permutation serves these tests (the device tests take the
    library's std::shuffle)"""
    return np.random.RandomState(seed).permutation(n)


@pytest.mark.parametrize("method,L,N,B", [("Box", 40, 2, 3), ("Ellipse", 64, 3, 2), ("Ellipse", 4, 4, 1)])
def test_invariants_of_a_run(method, L, N, B):
    r = nr.NestedRef(N, L, -5.0, 5.0, batch_size=B, method=method, proposal_update_frequency=10, uniform_seed=5,
                     normal_seed=6)
    r.first_generation()
    for _ in range(40):
        r.generation()
        assert np.all((r.cand >= 0.) & (r.cand <= 1.))
        assert r.s["LogVolume"] == pytest.approx(-r.s["Accepted Samples"] * math.log((L + 1.) / L), abs=1e-12)
        if method == "Ellipse":
            assert np.abs(r.cov @ r.inv_cov - np.eye(N)).max() < 1e-9
    key = np.asarray(r.dead_lpw) + np.asarray(r.dead_ll)
    assert key.size > 0 and np.all(np.diff(key) >= 0)
    assert r.rank == sorted(range(L), key=lambda i: r.live_lpw[i] + r.live_ll[i])


@pytest.mark.parametrize("L,N", [(64, 3), (257, 64), (4, 4)])
def test_the_ellipse_holds_every_live_point(L, N):
    r = nr.NestedRef(N, L, -5.0, 5.0, method="Ellipse", uniform_seed=9, normal_seed=10)
    r.first_generation()
    r.update_bounds()
    assert np.abs(r.cov @ r.inv_cov - np.eye(N)).max() < 1e-9
    dif = r.live - r.mean
    dist = np.einsum("si,ij,sj->s", dif, r.inv_cov, dif)
    assert dist.max() <= 1 + 1e-12
    # cholesky_decomp1's layout: L L^T = cov below, cov itself above the diagonal
    Lc = np.tril(r.axes)
    assert np.allclose(Lc @ Lc.T, r.cov, rtol=1e-10, atol=0)
    if L > N:  # (the variance branch leaves zeros there)
        iu = np.triu_indices(N, 1)
        ratio = r.axes[iu] / r.cov[iu]  # both are the fitted covariance, rescaled by sqrt(ef) and by ef
        assert np.allclose(ratio, ratio[0], rtol=1e-12, atol=0)


def test_lu_inverse_and_determinant():
    rs = np.random.RandomState(1)
    A = rs.standard_normal((7, 7))
    lu, perm, signum = nr.lu_decomp(A)
    assert nr.lu_det(lu, signum) == pytest.approx(np.linalg.det(A), rel=1e-12)
    assert np.abs(nr.lu_invert(lu, perm) @ A - np.eye(7)).max() < 1e-12
    assert signum in (-1.0, 1.0) and sorted(perm) == list(range(7))


def test_ellipse_constant_is_the_unit_ball_volume():
    for n in range(1, 65):
        assert nr.ellipse_constant(n) == pytest.approx(math.pi ** (n / 2.) / math.gamma(n / 2. + 1.), rel=1e-13)


# The analytic pin: log-likelihood -0.5 |x|^2 on U[-a, a]^N.
A, N, L = 5.0, 3, 500
SEED = 2  # a seed for which the restatement passes (found by running seeds 1, 2, 3: all three pass)
LOG_Z = N * math.log(math.sqrt(2 * math.pi) * math.erf(A / math.sqrt(2)) / (2 * A))
H = N * (math.log(2 * A) - 0.5 * math.log(2 * math.pi * math.e))  # the information, analytic
BOUND = 4 * math.sqrt(H / L)  # Skilling's error estimate, four standard deviations


@pytest.fixture(scope="module")
def gaussian_run():
    r = nr.NestedRef(N, L, -A, A, uniform_seed=SEED, normal_seed=SEED + 100, shuffle_seed=SEED + 200)
    generations = r.run()
    r.finalize(permutation)
    return r, generations


def test_gaussian_evidence(gaussian_run):
    r, generations = gaussian_run
    assert r.terminated(generations) == ["Min Log Evidence Delta"]
    assert abs(r.s["LogEvidence"] - LOG_Z) <= BOUND
    assert r.s["Information"] == pytest.approx(H, abs=0.5)


def test_gaussian_posterior(gaussian_run):
    r, _ = gaussian_run
    P = np.asarray(r.post)
    assert P.shape[0] > 500 and P.shape[1] == N
    # the reference's own tests allow 0.05 at L = 1500; sqrt(1500 / 500) of it, rounded up
    assert np.all(np.abs(P.mean(axis=0)) <= 0.1)
    assert np.all(np.abs(P.std(axis=0, ddof=1) - 1.0) <= 0.1)
    assert len(r.post_lp) == len(r.post_ll) == P.shape[0]
