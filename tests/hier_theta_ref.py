"""Plain Python restatement of the reference's Hierarchical/Theta
log-likelihood (problem/hierarchical/theta/theta.cpp.base), in the reference's
loop order, on tests/hier_ref.py's densities, parameters and logSumExp:

  Theta::initialize             :64-83    den_i = -log(K) + LSE_j( (0.0 + sum_k logdens_k(S[j][k]; i)) - lpS[j] )
  Theta::evaluateLogLikelihood  :97-124   LL(x) = (subLL(x) - log(M)) + LSE_i( (0.0 + sum_k logdens_k(x[k]; i)) - den_i )

S (K x D) / lpS (K): the sub-experiment's 'Sample Database' / 'Sample LogPrior
Database'; i runs over the M rows of the Psi experiment's 'Sample Database',
whose conditional priors (a_i, b_i, cn_i) are hier_ref.theta_new_params's.
Everything is computed as written, infinities and NaN included.
"""
import hier_ref as H


def theta_denominators(kinds, param_index, param_const, psi_db, sub_db, sub_log_priors, libm=False, params=None):
    """The M precomputed log-denominators."""
    log, _ = H.functions(libm)
    if params is None:
        params = H.theta_new_params(kinds, param_index, param_const, psi_db, libm)
    neg_log_k = -log(float(len(sub_db)))
    den = []
    for par in params:
        values = []
        for row, lp in zip(sub_db, sub_log_priors):
            v = 0.
            for k, kind in enumerate(kinds):
                v += H.log_density(kind, float(row[k]), par[k][0], par[k][1], par[k][2], log)
            values.append(v - float(lp))
        den.append(neg_log_k + H.log_sum_exp(values, libm))
    return den


def theta_loglik(x, sub_ll, kinds, param_index, param_const, psi_db, sub_db=None, sub_log_priors=None, libm=False,
                 params=None, den=None):
    """LL(x) with the sub-problem's own log-likelihood sub_ll (None: 0.0).
    params / den: theta_new_params / theta_denominators formed once (the same
    doubles whether formed once or at every evaluation)."""
    log, _ = H.functions(libm)
    if params is None:
        params = H.theta_new_params(kinds, param_index, param_const, psi_db, libm)
    if den is None:
        den = theta_denominators(kinds, param_index, param_const, psi_db, sub_db, sub_log_priors, libm, params)
    values = []
    for par, d in zip(params, den):
        v = 0.
        for k, kind in enumerate(kinds):
            v += H.log_density(kind, float(x[k]), par[k][0], par[k][1], par[k][2], log)
        values.append(v - d)
    sub_ll = 0.0 if sub_ll is None else float(sub_ll)
    return (sub_ll - log(float(len(params)))) + H.log_sum_exp(values, libm)
