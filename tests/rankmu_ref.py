"""Exact reference for one CMA-ES covariance update (adaptC) and the rounding
bound any summation order of it obeys.  Plain Python / NumPy, no device.

Every double is taken as the exact rational it is.  Arrays are scaled to
Python integers (x = I * 2**-K, exact) and the rank-mu products are formed
with object-dtype NumPy matmul, so the result carries no rounding at all.

For the lower triangle (e <= d), with c1 and cmu formed in double as the
kernels do (CMAES.cpp.base:693-694) and then taken as exact:

  want[d][e] = (1-c1-cmu) C_old + c1 (pc_d pc_e + (1-hsig) cc (2-cc) C_old)
               + (cmu/sigma^2) sum_k w_k (x_kd - m_d)(x_ke - m_e)
  tol[d][e]  = (mu + 16 + extra) 2^-53 ( (cmu/sigma^2) sum_k |w_k| |x_kd - m_d| |x_ke - m_e|
                                         + 2 |C_old| + c1 |pc_d pc_e| )

tol is the any-order summation bound gamma_{mu-1} * sum|terms| plus a fixed
allowance (16) for the per-term roundings: the two subtractions, scale * w,
(scale w) * y, the rounded sigma^2 and the base expression.  `extra` is the
number of partial sums added by somebody else (the shard count).  The bound is
derived, not measured; where tol == 0 a value must equal want exactly.

The mean: sum_k w_k x_k exact, bound (mu + 16 + extra) 2^-53 sum_k |w_k| |x_k|.
"""
from fractions import Fraction

import numpy as np

U = 53  # 2^-53: the unit roundoff of binary64


def ccov(N, mueff):
    """(ccov1, ccovmu) in double, operation for operation as k_paths /
    k_rankmu_tile / the oracle form them."""
    N, mueff = float(N), float(mueff)
    ca, cb = N + 1.3, N + 2.0
    c1 = 2.0 / (ca * ca + mueff)
    cmu = 2.0 * (mueff - 2.0 + 1.0 / mueff) / (cb * cb + mueff)
    if 1.0 - c1 < cmu:
        cmu = 1.0 - c1
    return c1, cmu


def dyadic(a):
    """(I, K): object array of Python ints and an int with a == I * 2**-K exactly."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("rankmu_ref: non-finite input")
    m, e = np.frexp(a)
    mi = np.ldexp(m, U).astype(np.int64)  # |m| 2^53 is an integer below 2^53
    ex = e.astype(np.int64) - U
    nz = mi != 0
    K = max(0, int(-ex[nz].min())) if nz.any() else 0
    sh = np.where(nz, ex + K, 0)
    out = np.empty(a.size, dtype=object)
    out[:] = [int(v) << int(s) for v, s in zip(mi.ravel().tolist(), sh.ravel().tolist())]
    return out.reshape(a.shape), K


def _frac(x):
    """(int, K) of a dyadic Fraction"""
    x = Fraction(x)
    K = x.denominator.bit_length() - 1
    assert x.denominator == 1 << K
    return x.numerator, K


def _add(a, b):
    (ia, ka), (ib, kb) = a, b
    K = max(ka, kb)
    return ia * (1 << (K - ka)) + ib * (1 << (K - kb)), K


def _mul(a, b):
    return a[0] * b[0], a[1] + b[1]


def _absobj(a):
    return np.where(a < 0, -a, a) if a.size else a


def _gram_lower(A, B, blocks=6):
    """A^T B (object ints) on the lower triangle, by row blocks; entries above
    the diagonal blocks stay 0."""
    N = A.shape[1]
    out = np.zeros((N, N), dtype=object)
    if A.shape[0] == 0:
        return out
    b = max(1, -(-N // blocks))
    for i0 in range(0, N, b):
        i1 = min(N, i0 + b)
        out[i0:i1, :i1] = np.matmul(A[:, i0:i1].T, B[:, :i1])
    return out


_RATIO = np.frompyfunc(lambda e, t: (e / t) if t else (0.0 if e == 0 else np.inf), 2, 1)


class Bounded:
    """want = num * 2**-K / den (elementwise), tol likewise with tnum: the
    exact value and its bound on one scale.  den is a positive int."""

    def __init__(self, num, tnum, K, den, lower):
        self.num, self.tnum, self.K, self.den, self.lower = num, tnum, K, den, lower

    def _floats(self, n):
        d = self.den << self.K
        return np.array([float(Fraction(int(v), d)) for v in n.ravel().tolist()]).reshape(n.shape)

    @property
    def want(self):
        """want rounded to double (for printing; the checks use the integers)"""
        return self._floats(self.num)

    @property
    def tol(self):
        return self._floats(self.tnum)

    def ratios(self, got):
        """err / tol for every element of `got` (float array; a matrix is
        read on its lower triangle, the rest returned as 0): 0 where both are
        0, inf where tol == 0 and the value differs from want."""
        got = np.asarray(got, dtype=np.float64).reshape(self.num.shape)
        gi, gk = dyadic(got)
        # got = gi 2^-gk; want = num 2^-K / den  ->  compare gi den 2^-gk with num 2^-K
        K = max(gk, self.K)
        err = _absobj(gi * (self.den << (K - gk)) - self.num * (1 << (K - self.K)))
        tol = self.tnum * (1 << (K - self.K))
        r = _RATIO(err, tol).astype(np.float64)
        return np.tril(r) if self.lower else r

    def worst(self, got):
        return float(self.ratios(got).max()) if self.num.size else 0.0


def covariance(N, Xsel, w, m_prev, sigma, C_old, pc, hsig, cc, mueff, extra=0):
    """The exact adaptC result and its bound (module docstring).  Xsel: the mu
    selected rows in selection order (mu x N); sigma: pre-update; pc, hsig,
    cc, mueff: post-update.  Returns a Bounded over the N x N matrix; only its
    lower triangle (e <= d) is filled in."""
    Xsel = np.asarray(Xsel, dtype=np.float64).reshape(-1, N)
    mu = Xsel.shape[0]
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size != mu:
        raise ValueError("rankmu_ref: one weight per selected row")
    m_prev = np.asarray(m_prev, dtype=np.float64).reshape(N)
    C_old = np.asarray(C_old, dtype=np.float64).reshape(N, N)
    pc = np.asarray(pc, dtype=np.float64).reshape(N)
    c1, cmu = ccov(N, mueff)
    # rank-mu: Y on one scale with m_prev, S = Y^T diag(w) Y
    xm, Kx = dyadic(np.concatenate([Xsel.reshape(-1), m_prev]))
    Y = xm[:mu * N].reshape(mu, N) - xm[mu * N:][None, :]
    wi, Kw = dyadic(w)
    S = _gram_lower(Y * wi[:, None], Y)
    Y = _absobj(Y)
    Sabs = _gram_lower(Y * _absobj(wi)[:, None], Y)
    Ks = 2 * Kx + Kw
    # sigma^2 = s2 2^-K2 exactly; everything below is multiplied by sigma^2
    si, Ksig = dyadic(np.array([sigma]))
    s2, K2 = int(si[0]) ** 2, 2 * Ksig
    if s2 == 0:
        raise ValueError("rankmu_ref: sigma == 0")
    fc1, fcmu, fcc = Fraction(c1), Fraction(cmu), Fraction(float(cc))
    a = 1 - fc1 - fcmu + fc1 * (1 - int(hsig)) * fcc * (2 - fcc)
    Ci, Kc = dyadic(C_old)
    pi, Kp = dyadic(pc)
    PP = np.multiply.outer(pi, pi)
    sig2 = (s2, K2)
    base = _add(_mul(_mul((Ci, Kc), _frac(a)), sig2), _mul(_mul((PP, 2 * Kp), _frac(fc1)), sig2))
    num, K = _add(base, _mul((S, Ks), _frac(fcmu)))
    babs = _add(_mul(_mul((_absobj(Ci), Kc), (2, 0)), sig2), _mul(_mul((_absobj(PP), 2 * Kp), _frac(fc1)), sig2))
    tn, Kt = _add(babs, _mul((Sabs, Ks), _frac(fcmu)))
    tn, Kt = tn * (mu + 16 + int(extra)), Kt + U
    # one scale for both; den = s2 2^-K2
    Kc2 = max(K, Kt)
    num, tn = num * (1 << (Kc2 - K)), tn * (1 << (Kc2 - Kt))
    # value = num 2^-Kc2 / (s2 2^-K2) = num 2^-(Kc2-K2) / s2
    Kout = Kc2 - K2
    if Kout < 0:
        num, tn, Kout = num * (1 << -Kout), tn * (1 << -Kout), 0
    return Bounded(num, tn, Kout, s2, lower=True)


def mean(N, Xsel, w, extra=0):
    """sum_k w_k x_k exact, with its bound; a Bounded over N elements."""
    Xsel = np.asarray(Xsel, dtype=np.float64).reshape(-1, N)
    mu = Xsel.shape[0]
    xi, Kx = dyadic(Xsel)
    wi, Kw = dyadic(np.asarray(w, dtype=np.float64).reshape(mu))
    if mu:
        num = np.matmul(wi, xi)
        tn = np.matmul(_absobj(wi), _absobj(xi)) * (mu + 16 + int(extra))
    else:
        num = np.zeros(N, dtype=object)
        tn = num.copy()
    K = Kx + Kw
    return Bounded(num * (1 << U), tn, K + U, 1, lower=False)


def float_bound(N, Ysel, w, sigma, C_old, pc, mueff, extra=0):
    """The covariance bound in plain float64, for comparing two device runs
    that both carry the error (factor 2); the sum of magnitudes is inflated by
    1.01 to cover its own rounding.  Ysel: the selected rows minus m_prev."""
    Ysel = np.abs(np.asarray(Ysel, dtype=np.float64).reshape(-1, N))
    mu = Ysel.shape[0]
    w = np.abs(np.asarray(w, dtype=np.float64).reshape(mu))
    C_old = np.asarray(C_old, dtype=np.float64).reshape(N, N)
    pc = np.asarray(pc, dtype=np.float64).reshape(N)
    c1, cmu = ccov(N, mueff)
    S = 1.01 * (cmu / (float(sigma) * float(sigma))) * ((Ysel * w[:, None]).T @ Ysel)
    return 2.0 * (mu + 16 + int(extra)) * 2.0 ** -U * (S + 2.0 * np.abs(C_old) + c1 * np.abs(np.outer(pc, pc)))
