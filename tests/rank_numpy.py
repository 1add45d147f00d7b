"""Numpy statement of the rank-normalised convergence diagnostics (the yardstick of bayes_drt_amd/csrc/bdrt_rank.hip).

Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), "Rank-normalization, folding, and localization: an improved R-hat for
assessing convergence of MCMC": rank-normalised, folded split R-hat, bulk and tail effective sample size, ESS and MCSE of the
mean.  Everything works on the SPLIT chains, the convention of Stan's `posterior` package and of arviz.  Neither is available
to compare against, so no bit-parity with them is claimed; what the two would differ in: this statement takes the ESS from the
project's Geyer estimator (tests/diag_numpy.py `ess`, Stan 2.19's, applied to the 2M split chains) and caps it at S log10 S.

`y` is one column: [M chains, N draws]; `probs` = (p_lo, p_hi) are the tail probabilities of ess_tail.
"""
import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from tests import diag_numpy as dn

PROBS = (0.05, 0.95)
KEYS = ('rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'sd')


def split(y):
    """Chain m -> rows 2m (first n draws) and 2m + 1 (last n draws), n = N // 2: an odd N drops the middle draw."""
    y = np.asarray(y, dtype=np.float64)
    M, N = y.shape
    n = N // 2
    return np.concatenate([y[:, :n], y[:, N - n:]], axis=1).reshape(2 * M, n)


def zscale(Y):
    """Ranks over ALL entries of Y (average rank for ties), mapped through the normal quantile function."""
    r = rankdata(Y.ravel(), method='average').reshape(Y.shape)
    return ndtri((r - 0.375) / (Y.size + 0.25))


def rhat_plain(Y):
    """R-hat with the rows of Y as the chains, no further split.  NaN for n < 2."""
    H, n = Y.shape
    if n < 2:
        return np.nan
    # a row of equal values (a chain that did not move) has that value as its mean and variance 0 exactly: the rounding of
    # n additions would otherwise decide between W = 0 (R-hat inf) and W ~ 1e-32 (R-hat ~ 1e16)
    const = np.all(Y == Y[:, :1], axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        B = n * np.var(np.where(const, Y[:, 0], Y.mean(axis=1)), ddof=1)
        W = np.mean(np.where(const, 0.0, np.var(Y, axis=1, ddof=1)))
        return np.sqrt((B / W + n - 1.0) / n)


def ess_capped(Y):
    """The project's Geyer estimator (dn.ess: NaN for n < 4 and for a constant or non-finite series), capped at S log10 S."""
    with np.errstate(divide='ignore', invalid='ignore'):
        e = dn.ess(Y)
    S = Y.size
    return min(e, S * np.log10(S)) if np.isfinite(e) else np.nan


def nan_max(a, b):
    return np.nan if (np.isnan(a) or np.isnan(b)) else max(a, b)


def nan_min(a, b):
    return np.nan if (np.isnan(a) or np.isnan(b)) else min(a, b)


def series(y, probs=PROBS):
    """The six series whose ESS / R-hat the diagnostics take: z, folded z, the two indicators, Y (each [2M, n]), or None for a
    column that gives NaN everywhere."""
    Y = split(y)
    if Y.size == 0 or not np.all(np.isfinite(Y)) or np.all(Y == Y[0, 0]):
        return None
    q_lo, q_hi = (np.percentile(Y, 100 * p) for p in probs)
    return {'z': zscale(Y), 'zfold': zscale(np.abs(Y - np.median(Y))), 'lo': (Y <= q_lo).astype(float),
            'hi': (Y <= q_hi).astype(float), 'Y': Y}


def column_stats(y, probs=PROBS):
    """dict of rhat, ess_bulk, ess_tail, ess_mean, mcse_mean, sd of one column y [M, N]."""
    s = series(y, probs)
    if s is None:                                   # a non-finite draw or a constant Y: NaN everywhere
        return dict.fromkeys(KEYS, np.nan)
    Y = s['Y']
    ess_mean = ess_capped(Y)
    sd = np.std(Y.ravel(), ddof=1)
    return {'rhat': nan_max(rhat_plain(s['z']), rhat_plain(s['zfold'])),
            'ess_bulk': ess_capped(s['z']),
            'ess_tail': nan_min(ess_capped(s['lo']), ess_capped(s['hi'])),
            'ess_mean': ess_mean,
            'mcse_mean': sd / np.sqrt(ess_mean),
            'sd': sd}


def min_margin(y, probs=PROBS):
    """The smallest Geyer pair-sum margin (dn.ess_and_margin) over the four ESS series of one column; inf for a NaN column."""
    s = series(y, probs)
    if s is None:
        return np.inf
    return min(dn.ess_and_margin(s[k])[1] for k in ('z', 'lo', 'hi', 'Y'))


def diagnostics(X, probs=PROBS):
    """X [G groups, M chains, N draws, C columns] -> dict of [G, C] arrays."""
    X = np.asarray(X, dtype=np.float64)
    G, M, N, Cc = X.shape
    out = {k: np.empty((G, Cc)) for k in KEYS}
    for g in range(G):
        for c in range(Cc):
            st = column_stats(X[g, :, :, c], probs)
            for k in KEYS:
                out[k][g, c] = st[k]
    return out
