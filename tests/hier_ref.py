"""Plain Python restatement of the reference's Hierarchical/Psi and
Hierarchical/ThetaNew log-likelihoods, in the reference's loop order:

  Psi::evaluateLogLikelihood       problem/hierarchical/psi/psi.cpp.base:120-141
  ThetaNew::evaluateLogLikelihood  problem/hierarchical/thetaNew/thetaNew.cpp.base:35-54
  logSumExp                        auxiliar/math.hpp:205-225
  getLogDensity / updateDistribution of the six univariate distributions

IEEE double arithmetic, one rounding per operation.  log and exp are the
oracle library's correctly rounded kr_log_cr / kr_exp_cr (the convention of
every likelihood here); libm=True uses math.log / math.exp as the reference's
own binary would.
"""
import ctypes
import math
import os

INF = float("inf")
NAN = float("nan")

UNIFORM, NORMAL, EXPONENTIAL, LAPLACE, CAUCHY, LOGNORMAL = range(6)

_LIB = None


def _oracle():
    global _LIB
    if _LIB is None:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "librefcpu.so")
        L = ctypes.CDLL(path)
        for f in (L.kr_log_cr, L.kr_exp_cr):
            f.restype = ctypes.c_double
            f.argtypes = [ctypes.c_double]
        _LIB = L
    return _LIB


def _libm_log(x):
    if x != x:
        return x
    if x == 0.0:
        return -INF
    if x < 0.0:
        return NAN
    return math.log(x) if x != INF else INF


def _libm_exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def functions(libm=False):
    if libm:
        return _libm_log, _libm_exp
    L = _oracle()
    return L.kr_log_cr, L.kr_exp_cr


def log_sum_exp(values, libm=False):
    log, exp = functions(libm)
    m = -INF
    for v in values:
        if v > m:
            m = v
    if math.isinf(m):
        return m
    s = 0.0
    for v in values:
        s += exp(v - m)
    return m + log(s)


def prior_const(kind, a, b, log):
    """The distribution's constant after updateDistribution (Exponential:
    the -log(mean) of its getLogDensity)."""
    if kind in (NORMAL, LOGNORMAL):
        return -0.5 * log(2 * math.pi) - log(b)
    if kind == EXPONENTIAL:
        return -log(b)
    if kind == LAPLACE:
        return -log(2. * b)
    if kind == CAUCHY:
        return -log(b * math.pi)
    return NAN if b - a <= 0.0 else -log(b - a)


def _div(x, y):
    try:
        return x / y
    except ZeroDivisionError:
        if x != x or x == 0.0:
            return NAN
        return math.copysign(INF, x) * math.copysign(1.0, y)


def log_density(kind, x, a, b, cn, log):
    if kind == NORMAL:
        d = _div(x - a, b)
        return cn - 0.5 * d * d
    if kind == EXPONENTIAL:
        if x - a < 0:
            return -INF
        return cn - _div(x - a, b)
    if kind == LAPLACE:
        return cn - _div(abs(x - a), b)
    if kind == CAUCHY:
        return cn - log(1. + _div((x - a) * (x - a), b * b))
    if kind == LOGNORMAL:
        if x <= 0:
            return -INF
        lx = log(x)
        d = _div(lx - a, b)
        return cn - lx - 0.5 * d * d
    return cn if (x >= a and x <= b) else -INF


def _params(kinds, param_index, param_const, source, log):
    out = []
    for k, kind in enumerate(kinds):
        a = source[param_index[k][0]] if param_index[k][0] >= 0 else param_const[k][0]
        b = source[param_index[k][1]] if param_index[k][1] >= 0 else param_const[k][1]
        a, b = float(a), float(b)
        out.append((a, b, prior_const(kind, a, b, log)))
    return out


def psi_loglik(point, kinds, param_index, param_const, groups, log_priors, libm=False):
    """groups[g]: K_g x D samples of sub-experiment g; log_priors[g]: their K_g log-priors."""
    log, _ = functions(libm)
    par = _params(kinds, param_index, param_const, point, log)
    ll = 0.0
    for rows, lps in zip(groups, log_priors):
        values = []
        for row, lp in zip(rows, lps):
            v = -float(lp)
            for k, kind in enumerate(kinds):
                v += log_density(kind, float(row[k]), par[k][0], par[k][1], par[k][2], log)
            values.append(v)
        ll += log_sum_exp(values, libm)
    return ll


def theta_new_params(kinds, param_index, param_const, database, libm=False):
    """updateConditionalPriors at every database row (the same doubles whether
    formed once or at every evaluation)."""
    log, _ = functions(libm)
    return [_params(kinds, param_index, param_const, row, log) for row in database]


def theta_new_loglik(point, kinds, param_index, param_const, database, libm=False, params=None):
    """database: the Psi experiment's M x Npsi 'Sample Database'."""
    log, _ = functions(libm)
    if params is None:
        params = theta_new_params(kinds, param_index, param_const, database, libm)
    values = []
    for par in params:
        v = 0.
        for k, kind in enumerate(kinds):
            v += log_density(kind, float(point[k]), par[k][0], par[k][1], par[k][2], log)
        values.append(v)
    return -log(float(len(database))) + log_sum_exp(values, libm)


def invalid_parameter(kinds, param_index, param_const, point):
    """First conditional prior whose updateDistribution check fails at `point`, or None."""
    for k, kind in enumerate(kinds):
        b = point[param_index[k][1]] if param_index[k][1] >= 0 else param_const[k][1]
        if kind in (NORMAL, LOGNORMAL, LAPLACE, CAUCHY) and b <= 0.0:
            return k
    return None
