"""Numpy statement of prediction at held-out frequencies (the yardstick of bayes_drt_amd/csrc/bdrt_heldout.hip).

A fold of a cross-validation is a sampling fit on a training grid.  For its posterior draws theta_s, s = 1 .. S, and a held-out
frequency f with datum z = (z_re, z_im) on the fold's scale:

  * Z_hat(theta_s, f): the sum over blocks of v_b = A_b(f) x_b (series) or conj(v_b) / |v_b|^2 (parallel), x_b the constrained
    coefficients times x_scale, plus Rinf + i 2 pi f induc -- what `Inverter.predict_Z_distribution` and bdrt_model_terms.h
    (`lik_consts`, `parallel_fwd`) state, in scaled units;
  * sigma_tot(theta_s, f): the error model of `lik_point<false>`,
        s2_re = sigma_res^2 + sigma_min^2 + alpha_prop^2 zr^2 + alpha_re^2 zr^2 + alpha_im^2 zi^2,
        s2_im the same with alpha_prop^2 zi^2, (zr, zi) = Z_hat;
  * the predictive of a held-out unit: the equal-weight mixture of the draws' normals: lpd = logsumexp_s(ll_s) - log S, where
    for unit='frequency' ll_s is the real plus the imaginary log density of the draw; mean, sd and PIT are
    tests/loo_predict_numpy.py's `_moments` with w = 1 / S.

The outlier error models have no statement here: every training point has its own sigma_out and a held-out point has none.

`transformed` takes the floating-point type to compute in (float64 or np.longdouble) and the direction of the sum over the basis
functions, so that a test can measure the statement's own rounding error and hold the kernel to a multiple of it.
"""
import numpy as np

from tests.loo_predict_numpy import _moments
from tests.psis_numpy import pointwise_log_lik

FIELDS = ('mean', 'sd', 'pit')


def layout(Ks, outlier_rows=0):
    """Offsets in the parameter vector (Stan declaration order, include/bdrt.h): Rinf_raw, induc_raw, the blocks' x, the four
    error raws, (2 Nf outlier parameters,) the blocks' ups, the blocks' three strengths."""
    o, x = 2, []
    for K in Ks:
        x.append(o)
        o += K
    return dict(x=x, err=o, D=o + 4 + outlier_rows + sum(Ks) + 3 * len(Ks))


def _dot(x, A, reverse):
    """x [B, K] . A [H, K]^T, the K terms of every entry added one after the other from the first (or the last) on"""
    if reverse is None:
        return x @ A.T
    prod = x[:, None, :] * A[None, :, :]
    if reverse:
        prod = prod[:, :, ::-1]
    acc = np.zeros(prod.shape[:2], dtype=prod.dtype)
    for k in range(prod.shape[2]):
        acc = acc + prod[:, :, k]
    return acc


def transformed(blocks, params, freq_test, A_test_blocks, sigma_min=0.002, induc_scale=1.0, dtype=np.float64, reverse=None):
    """Z_hat, sigma_tot [B, 2 H] (real halves, then imaginary halves) of constrained parameter rows params [B, D].
    blocks: dicts with K (or A), parallel, x_scale; A_test_blocks: per block the stacked prediction rows [2 H, K] (real rows,
    then imaginary rows).  reverse: None (numpy's matrix product), False / True (explicit sums, forward / reversed)."""
    T = dtype
    params = np.atleast_2d(np.asarray(params, dtype=float)).astype(T)
    f = np.asarray(freq_test, dtype=float).reshape(-1).astype(T)
    H = len(f)
    Ks = [int(b['K']) if 'K' in b else int(np.shape(b['A'])[1]) for b in blocks]
    lay = layout(Ks)
    zr, zi = np.zeros((len(params), H), dtype=T), np.zeros((len(params), H), dtype=T)
    for b, (blk, A) in enumerate(zip(blocks, A_test_blocks)):
        A = np.asarray(A, dtype=float).astype(T)
        assert A.shape == (2 * H, Ks[b])
        x = params[:, lay['x'][b]:lay['x'][b] + Ks[b]] * T(float(blk.get('x_scale', 1.0)))
        vr, vi = _dot(x, A[:H], reverse), _dot(x, A[H:], reverse)
        if blk.get('parallel', False):
            dn = vr * vr + vi * vi
            vr, vi = vr / dn, -vi / dn
        zr, zi = zr + vr, zi + vi
    e = lay['err']
    Rinf, induc = T(100.0) * params[:, 0], params[:, 1] * T(float(induc_scale))
    s_res, a_p, a_r, a_i = [T(0.05) * params[:, e + q] for q in range(4)]
    zr = zr + Rinf[:, None]
    zi = zi + induc[:, None] * (T(2.0) * T(np.pi) * f)[None, :]
    c0 = (s_res * s_res + T(float(sigma_min)) * T(float(sigma_min)))[:, None]
    common = (a_r * a_r)[:, None] * zr * zr + (a_i * a_i)[:, None] * zi * zi
    s2_re = c0 + (a_p * a_p)[:, None] * zr * zr + common
    s2_im = c0 + (a_p * a_p)[:, None] * zi * zi + common
    return np.concatenate([zr, zi], axis=1), np.sqrt(np.concatenate([s2_re, s2_im], axis=1))


def reduce_unit(mu, sg, z):
    """One held-out unit: mu, sg [S, n], z [n] -> (lpd, mean [n], sd [n], pit [n]); NaN when a log-likelihood is not finite."""
    mu, sg = np.asarray(mu, dtype=float), np.asarray(sg, dtype=float)
    z = np.asarray(z, dtype=float).reshape(-1)
    S, n = mu.shape
    ll = pointwise_log_lik(mu, sg, z).sum(axis=1)
    if not np.all(np.isfinite(ll)):
        return np.nan, np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    mx = ll.max()
    with np.errstate(all='ignore'):
        return (mx + np.log(np.sum(np.exp(ll - mx)))) - np.log(S), *_moments(np.full(S, 1.0 / S), mu, sg, z)


def reduce(Zhat, sig, z, unit='frequency'):
    """One group: Zhat, sig [S, N2], z [N2]; unit 'frequency' (scalars i and i + N2 / 2 are one unit) or 'point'.  Returns a dict
    of lpd [units] and mean, sd, pit [N2]."""
    Zhat, sig, z = np.asarray(Zhat, dtype=float), np.asarray(sig, dtype=float), np.asarray(z, dtype=float)
    N2 = Zhat.shape[1]
    pair = unit == 'frequency'
    U = N2 // 2 if pair else N2
    out = dict({k: np.empty(N2) for k in FIELDS}, lpd=np.empty(U))
    for j in range(U):
        cols = [j, j + U] if pair else [j]
        out['lpd'][j], m, s, p = reduce_unit(Zhat[:, cols], sig[:, cols], z[cols])
        out['mean'][cols], out['sd'][cols], out['pit'][cols] = m, s, p
    return out
