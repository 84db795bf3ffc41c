"""Hard symmetric matrices for the eigensolver tests (NumPy only, seeded).

family(kind, N, seed) returns an N x N symmetric matrix.  The families reach
what a seeded CMA-ES run from C = I never does: graded and clustered spectra,
exact zeros that deflate the tridiagonal in the middle, Householder steps with
tau == 0 between ordinary ones, scales near the ends of the double range, and
matrices that are not positive definite (an eigen failure).

test_eigen_cases_cpu.py pins every family against the CPU oracle and NumPy;
test_gpu_eigen_forced.py walks the device eigensolver kernels through them.
"""
import numpy as np

# the order of the GPU walk: each failing family is followed by an ordinary
# one, which proves that a failure leaves the solver usable
WALK = ("graded", "indefinite", "clustered", "block", "singular", "diagplus", "diagonal", "zerocol", "tiny", "huge")
FAILING = ("indefinite", "singular")
KINDS = WALK


def _orthogonal(N, rng):
    return np.linalg.qr(rng.standard_normal((N, N)))[0]


def _from_spectrum(lam, rng):
    lam = np.asarray(lam, dtype=np.float64)
    Q = _orthogonal(lam.size, rng)
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)


def zero_index(kind, N):
    """The row and column that zerocol / singular clear.  singular clears the
    first: the oracle's minimum eigenvalue has to be exactly 0.0, and a zero
    row in the middle is mixed into the others by the Householder step that
    starts on it (its eigenvalue comes out as +-1e-15).  Row 0 gives a first
    step with tau == 0 ahead of ordinary ones, d[0] = sd[0] = 0.0 exactly, and
    a chase whose only window starts at row 1."""
    return 0 if kind == "singular" else N // 3


def family(kind, N, seed=0):
    rng = np.random.default_rng([seed, N])
    if kind == "graded":
        return _from_spectrum(np.logspace(0, -14, N), rng)
    if kind == "clustered":
        lam = np.concatenate([np.full(N // 2, 1.0), np.full(N - N // 2, 2.0)])
        return _from_spectrum(lam * (1.0 + 1e-13 * rng.standard_normal(N)), rng)
    if kind == "block":
        M = np.zeros((N, N))
        a = 0
        for n in (N // 3, N // 3, N - 2 * (N // 3)):
            if n:
                M[a:a + n, a:a + n] = _from_spectrum(np.linspace(0.5, 2.0, n), rng)
            a += n
        return M
    if kind in ("diagplus", "diagonal"):
        M = np.diag(np.arange(1.0, N + 1.0))
        if kind == "diagplus" and N > 3:
            M[N - 1, 1] = M[1, N - 1] = 0.25
        return M
    if kind in ("zerocol", "singular"):
        M = _from_spectrum(np.linspace(0.5, 2.0, N), rng)
        k = zero_index(kind, N)
        M[k, :] = 0.0
        M[:, k] = 0.0
        M[k, k] = 2.0 if kind == "zerocol" else 0.0
        return M
    if kind == "tiny":
        return _from_spectrum(np.linspace(0.5, 2.0, N) * 1e-280, rng)
    if kind == "huge":
        return _from_spectrum(np.linspace(0.5, 2.0, N) * 1e140, rng)
    if kind == "indefinite":
        return _from_spectrum(np.linspace(-0.5, 2.0, N), rng)
    raise ValueError("unknown family: %s" % kind)
