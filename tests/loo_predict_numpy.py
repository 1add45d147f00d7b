"""Numpy statement of the PSIS-LOO predictive checks (the yardstick of bayes_drt_amd/csrc/bdrt_loo_predict.hip).

The likelihood of every model text is `Z ~ normal(Z_hat, sigma_tot)`, so the leave-one-out predictive distribution of a scalar
observation is the mixture of the draws' normals under the Pareto-smoothed importance weights of its unit (tests/psis_numpy.py:
`psislw`; Vehtari, Gelman, Gabry 2017).  Its mean, its sd and its cdf at the datum -- the LOO probability integral transform
of Gelfand, Dey and Chang (1992) -- are weighted sums over the draws: no replicated data and no random numbers.  The same sums
with equal weights 1 / S are the in-sample posterior predictive (`*_post`).

A unit is n scalars left out together: n = 1 a point, n = 2 the real and the imaginary part of one frequency.  Conventions the
kernel shares:
  * a unit with a non-finite log-likelihood gives NaN in every output and n_tail = 0;
  * a unit whose log-likelihoods are all equal keeps equal weights: k = inf and n_tail = 0;
  * ties: `psislw` orders the tail with a stable argsort, so among equal log ratios the draw with the smaller index gets the
    smaller smoothed weight.  That is part of the definition (the draws of such a pair may predict differently).
"""
import numpy as np
from scipy.special import erfc

from tests import psis_numpy as pn

FIELDS = ('mean', 'sd', 'pit', 'mean_post', 'sd_post', 'pit_post')


def _moments(w, mu, sg, z):
    """mean, sd and cdf at z of the mixture sum_s w_s normal(mu_s, sg_s), per scalar: w [S], mu, sg [S, n], z [n]"""
    d = mu - z                                                               # centred on the datum: no cancellation
    w = w[:, None]
    m1 = np.sum(w * d, axis=0)
    m2 = np.sum(w * (sg * sg + d * d), axis=0)
    pit = np.sum(w * (0.5 * erfc(d / (sg * np.sqrt(2.0)))), axis=0)
    return z + m1, np.sqrt(m2 - m1 * m1), pit


def predict_unit(mu, sg, z, reff=1.0):
    """One unit: mu, sg [S, n], z [n] -> dict of mean, sd, pit, mean_post, sd_post, pit_post [n], pareto_k and n_tail."""
    mu, sg = np.asarray(mu, dtype=float), np.asarray(sg, dtype=float)
    z = np.asarray(z, dtype=float).reshape(-1)
    S, n = mu.shape
    ll = pn.pointwise_log_lik(mu, sg, z).sum(axis=1)
    if not np.all(np.isfinite(ll)):
        out = {k: np.full(n, np.nan) for k in FIELDS}
        out.update(pareto_k=np.nan, n_tail=0)
        return out
    if np.all(ll == ll[0]):
        lw, k, n_tail = np.full(S, -np.log(S)), np.inf, 0
    else:
        lw, k, n_tail = pn.psislw(-ll, reff)
    with np.errstate(all='ignore'):
        loo = _moments(np.exp(lw), mu, sg, z)
        post = _moments(np.full(S, 1.0 / S), mu, sg, z)
    out = dict(zip(FIELDS, loo + post))
    out.update(pareto_k=k, n_tail=n_tail)
    return out


def predict(Zhat, sig, z, unit='frequency', reff=None):
    """One fit: Zhat, sig [S, 2 Nf], z [2 Nf]; unit 'frequency' (scalars i and i + Nf are one unit) or 'point'; reff None (1),
    a number or one per unit.  Returns the six per-scalar arrays [2 Nf] and pareto_k (float), n_tail (int32) per unit."""
    Zhat, sig, z = np.asarray(Zhat, dtype=float), np.asarray(sig, dtype=float), np.asarray(z, dtype=float)
    S, N2 = Zhat.shape
    pair = unit == 'frequency'
    U = N2 // 2 if pair else N2
    r = np.broadcast_to(np.asarray(1.0 if reff is None else reff, dtype=float), (U,))
    out = {k: np.empty(N2) for k in FIELDS}
    out.update(pareto_k=np.empty(U), n_tail=np.empty(U, dtype=np.int32))
    for j in range(U):
        cols = [j, j + U] if pair else [j]
        u = predict_unit(Zhat[:, cols], sig[:, cols], z[cols], r[j])
        for k in FIELDS:
            out[k][cols] = u[k]
        out['pareto_k'][j], out['n_tail'][j] = u['pareto_k'], u['n_tail']
    return out

