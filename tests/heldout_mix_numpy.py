"""Numpy statement of prediction at held-out frequencies under the outlier error models (the yardstick of
bayes_drt_amd/csrc/bdrt_heldout_mix.hip and of `loo.sigma_out_table`).

Under an outlier error model every training point has its own sigma_out; a held-out point has none, but the prior of sigma_out is
fixed by data, not by parameters:

  * mode 1 (`Series*_outliers`): sigma_out = 0.05 raw scale, raw ~ exponential(lam), scale ~ inv_gamma(alpha, beta).  1 / scale is
    gamma(alpha, rate beta), and the exponential's survival exp(-lam t / (0.05 scale)) averaged over it is the gamma's
    moment-generating function: P(y > t) = (1 + t / s)^-alpha, s = 0.05 beta / lam -- a Lomax distribution, with density
    (alpha / s) (1 + y / s)^-(alpha + 1) and E[y^2] = 2 s^2 / ((alpha - 1) (alpha - 2)) (+inf for alpha <= 2).  One y is shared by the real
    and the imaginary scalar of a frequency.
  * mode 2 (the other outlier families): sigma_out = 0.05 raw, raw ~ exponential(lam), per stacked row: y is exponential of scale
    s = 0.05 / lam, E[y^2] = 2 s^2.

So for a draw with mean mu and base scale s_b (sigma_tot without sigma_out: `tests/heldout_numpy.transformed`) the predictive of
a new scalar z is the scale mixture m(z) = int p(y) N(z | mu, s_b^2 + y^2) dy, the same mixture for every draw and point.  With
a table of nodes y_j and weights w_j (`table`: the trapezoid rule in ln y, w_j = step y_j p(y_j)):

    density of a scalar      m_s = sum_j w_j N(z | mu_s, s_b,s^2 + y_j^2)
    a pair unit              mode 1: sum_j w_j N(z_re | ...) N(z_im | ...) (the same y_j in both); mode 2: the product of the two m_s
    lpd_unit                 log((1 / S) sum_s m_s)
    mean                     (1 / S) sum_s mu_s                          (the mixture is symmetric)
    sd^2                     (1 / S) sum_s (s_b,s^2 + d_s^2) + E[y^2] - (mean - z)^2,  d_s = mu_s - z
    pit                      (1 / S) sum_s sum_j w_j Phi((z - mu_s) / sqrt(s_b,s^2 + y_j^2)), per scalar: always the marginal

`reduce` works with logarithms of the terms, so no residual underflows it in float64.  It takes the floating-point type
(float64 or np.longdouble; scipy's erfc has no wider form, so the argument of Phi is formed in the type and Phi itself in
float64) and the direction of its sums, so that a test can measure the statement's own rounding error and hold the kernel to a
multiple of it.
"""
import numpy as np
from scipy.special import erfc

FIELDS = ('mean', 'sd', 'pit')
LO, HI_MIN, HI_MAX, HI_EXP = -36.0, 10.0, 27.5, 5.0


def scale(mode, lam, alpha=5.0, beta=1.0):
    return 0.05 * beta / lam if mode == 1 else 0.05 / lam


def survival(mode, t, lam, alpha=5.0, beta=1.0):
    """P(sigma_out > t), closed form"""
    x = np.asarray(t, dtype=float) / scale(mode, lam, alpha, beta)
    return (1.0 + x) ** -alpha if mode == 1 else np.exp(-x)


def density(mode, y, lam, alpha=5.0, beta=1.0):
    """p(y) of sigma_out, closed form"""
    s = scale(mode, lam, alpha, beta)
    x = np.asarray(y, dtype=float) / s
    return (alpha / s) * (1.0 + x) ** -(alpha + 1.0) if mode == 1 else np.exp(-x) / s


def second_moment(mode, lam, alpha=5.0, beta=1.0):
    s = scale(mode, lam, alpha, beta)
    if mode == 1:
        return 2.0 * s * s / ((alpha - 1.0) * (alpha - 2.0)) if alpha > 2 else np.inf
    return 2.0 * s * s


def table(mode, lam, alpha=5.0, beta=1.0, step=0.125, dtype=np.float64):
    """(y [Q], w [Q], E[y^2], shared) in `dtype`: the trapezoid rule on the uniform grid u = LO, LO + step, ... in u = ln(y / s),
    w_j = step y_j p(y_j), halved at the two ends.  The grid ends at the first node at or beyond: mode 2, u = 5; mode 1, the
    larger of 10, ln(1e14) / alpha (the mass beyond is below 1e-14) and, for alpha > 2, ln(1e11 alpha (alpha - 1) / 2) / (alpha - 2)
    (the part of E[y^2] beyond is below 1e-11 of it), but 27.5 at most."""
    T = dtype
    if mode == 1:
        hi = max(HI_MIN, np.log(1e14) / alpha)
        if alpha > 2:
            hi = max(hi, (np.log(1e11) + np.log(alpha * (alpha - 1) / 2)) / (alpha - 2))
        hi = min(hi, HI_MAX)
    else:
        hi = HI_EXP
    n = int(np.ceil((hi - LO) / step)) + 1
    u = T(LO) + T(step) * np.arange(n).astype(T)
    t = np.exp(u)
    if mode == 1:
        w = T(step) * np.exp((np.log(T(alpha)) + u) - T(alpha + 1.0) * np.log1p(t))
    else:
        w = T(step) * np.exp(u - t)
    w[0] *= T(0.5)
    w[-1] *= T(0.5)
    return T(scale(mode, lam, alpha, beta)) * t, w, second_moment(mode, lam, alpha, beta), mode == 1


def _sum(a, axis, reverse):
    return np.sum(np.flip(a, axis) if reverse else a, axis=axis)


def _logsumexp(a, axis, reverse):
    mx = np.max(a, axis=axis, keepdims=True)
    return np.squeeze(mx, axis) + np.log(_sum(np.exp(a - mx), axis, reverse))


def log_density(mu, sb, z, y, w, shared, dtype=np.float64, reverse=False):
    """log m_s of one unit: mu, sb [S, n] (n = 1: a point; n = 2: a pair), z [n], table y, w [Q] -> [S]"""
    T = dtype
    mu, sb, z, y, w = [np.asarray(a).astype(T) for a in (mu, sb, z, y, w)]
    c0 = T(-0.5) * np.log(T(2.0) * T(np.pi))
    sg = np.sqrt((sb * sb)[:, :, None] + (y * y)[None, None, :])             # [S, n, Q]
    q = (z[None, :] - mu)[:, :, None] / sg
    ll = (c0 - np.log(sg)) - T(0.5) * (q * q)
    lw = np.log(w)[None, :]
    if shared:
        return _logsumexp(lw + np.sum(ll, axis=1), 1, reverse)
    return np.sum(_logsumexp(lw[:, None, :] + ll, 2, reverse), axis=1)


def reduce_unit(mu, sb, z, y, w, ey2, shared, dtype=np.float64, reverse=False):
    """One held-out unit: mu, sb [S, n], z [n] -> (lpd, mean [n], sd [n], pit [n]) in `dtype`; NaN when a term is not finite."""
    T = dtype
    mu, sb = np.asarray(mu, dtype=float), np.asarray(sb, dtype=float)
    z = np.asarray(z, dtype=float).reshape(-1)
    S, n = mu.shape
    nan = np.full(n, np.nan)
    if not np.all(np.isfinite(sb) & (sb > 0) & np.isfinite(mu)):
        return np.nan, nan, nan, nan
    with np.errstate(all='ignore'):
        lm = log_density(mu, sb, z, y, w, shared, T, reverse)
        if not np.all(np.isfinite(lm)):
            return np.nan, nan, nan, nan
        lpd = _logsumexp(lm, 0, reverse) - np.log(T(S))
        mu, sb, zT, yT, wT = [np.asarray(a).astype(T) for a in (mu, sb, z, y, w)]
        wS = T(1.0) / T(S)
        d = mu - zT
        m1 = _sum(wS * d, 0, reverse)
        m2 = _sum(wS * (sb * sb + d * d), 0, reverse) + T(ey2)
        sg = np.sqrt((sb * sb)[:, :, None] + (yT * yT)[None, None, :])
        phi = (0.5 * erfc((d[:, :, None] / (sg * np.sqrt(T(2.0)))).astype(float))).astype(T)
        pit = _sum(wS * _sum(wT[None, None, :] * phi, 2, reverse), 0, reverse)
        return lpd, zT + m1, np.sqrt(m2 - m1 * m1), pit


def reduce(Zhat, sig_base, z, tab, unit='frequency', dtype=np.float64, reverse=False):
    """One group: Zhat, sig_base [S, N2], z [N2]; tab = (y, w, E[y^2], shared); unit 'frequency' (scalars i and i + N2 / 2 are
    one unit) or 'point'.  Returns a dict of lpd [units] and mean, sd, pit [N2] in `dtype`."""
    y, w, ey2, shared = tab
    Zhat, sig_base, z = np.asarray(Zhat, dtype=float), np.asarray(sig_base, dtype=float), np.asarray(z, dtype=float)
    N2 = Zhat.shape[1]
    pair = unit == 'frequency'
    U = N2 // 2 if pair else N2
    out = dict({k: np.empty(N2, dtype=dtype) for k in FIELDS}, lpd=np.empty(U, dtype=dtype))
    for j in range(U):
        cols = [j, j + U] if pair else [j]
        out['lpd'][j], m, s, p = reduce_unit(Zhat[:, cols], sig_base[:, cols], z[cols], y, w, ey2, shared, dtype, reverse)
        out['mean'][cols], out['sd'][cols], out['pit'][cols] = m, s, p
    return out
