"""Log-posterior and gradient of the Series / Series_pos models (one distribution, with or without an outlier error model) on
the unconstrained scale, each with the sum of the absolute values of its additive terms -- an independent numpy statement of what
every log-posterior evaluator of csrc/ computes, written from the Stan text (bayes_drt/stan_model_files/Series_pos_modelcode.txt:24-69,
Series_pos_outliers_modelcode.txt:22-73) for the tests; held to central differences of itself and to tests/hessian_numpy.py by
tests/test_logp_reference_host.py.  Test infrastructure, not the product.

Layout of the unconstrained vector y (Stan declaration order, include/bdrt.h), D = 2 K + 9 (+ 2 nf with an outlier model):
  0 Rinf_raw, 1 induc_raw, 2 .. 2+K x, sigma_res_raw, alpha_prop_raw, alpha_re_raw, alpha_im_raw, [2 nf outlier parameters,]
  ups_raw[K], d0, d1, d2.
Every parameter but x is <lower=0> (y = log raw); x is <lower=0> for Series_pos, free for Series.
Outlier parameters (oracle/bdrt_oracle.c, bayes_drt_amd/model.py::layout):
  outlier_mode 1  sigma_out_raw[nf] ~ exponential(so_lambda), sigma_out_scale[nf] ~ inv_gamma(so_alpha, so_beta),
                  sigma_out = 0.05 raw .* scale, the same for both parts of a frequency (the package's Stan files);
  outlier_mode 2  sigma_out_raw[2 nf] ~ exponential(so_lambda), sigma_out = 0.05 raw, one per stacked row (the paper's files).

The measure.  A gradient component is one sum of additive terms: the likelihood's contributions frequency by frequency and part by
part, the rows of each L_i^T ( . ) product, each piece of each prior, the Jacobian's 1.  gabs_j is the same sum with every term
replaced by its absolute value (carried through the positive chain-rule factors: the scale of the raw parameter and, on the log
scale, the raw parameter itself): what the rounding error of ANY order of summation of these terms is relative to.  lp_abs is the
same for lp.  The intermediates (L_i x, Z_hat, e = Z - Z_hat, S = sigma_tot^2) enter with their computed values: their own inner
cancellation is in the measured ratio of the float64 references (tests/test_logp_reference_host.py::REF), not in gabs."""
import numpy as np

CLASSES = ('R', 'I', 'x', 'err', 'so', 'ups', 'd')


def class_slices(K, nf, outlier_mode=0):
    """index classes of the unconstrained vector; 'so' exists with an outlier model only"""
    nso = 2 * nf if outlier_mode else 0
    sl = {'R': slice(0, 1), 'I': slice(1, 2), 'x': slice(2, 2 + K), 'err': slice(2 + K, 6 + K)}
    if nso:
        sl['so'] = slice(6 + K, 6 + K + nso)
    sl['ups'] = slice(6 + K + nso, 6 + 2 * K + nso)
    sl['d'] = slice(6 + 2 * K + nso, 9 + 2 * K + nso)
    return sl


def _sum(T, axis, reverse):
    """the terms T added along axis; reverse: in the opposite order"""
    if reverse:
        T = np.ascontiguousarray(np.flip(T, axis))
    return T.sum(axis=axis)


def series_logp(y, A, L, Z, w, sigma_min, ups_alpha, ups_beta, induc_scale=1.0, pos=True, jacobian=False, outlier_mode=0,
                so_lambda=10.0, so_alpha=5.0, so_beta=1.0, dtype=float, reverse=False, drop=None):
    """(lp, lp_abs, g [D], gabs [D]) at the unconstrained point y.  A [2 nf, K] stacked (re; im), L = (L0, L1, L2) mode-scaled
    [K, K], Z [2 nf] stacked, w [nf] = 2 pi f.

    dtype: np.longdouble evaluates the same statement in extended precision from the float64 inputs converted.
    reverse: every reduction adds its terms in the opposite order (another float64 reference; no other difference).
    drop: (n, k), the mutation of tests/test_logp_reference_host.py: the likelihood term of frequency n (both parts) is left out
    of the gradient component of x_k.  Never the statement."""
    dt = dtype
    A = np.asarray(A, dtype=dt); nf = len(w); K = A.shape[1]
    L = [np.asarray(Li, dtype=dt) for Li in L]; Z = np.asarray(Z, dtype=dt); w = np.asarray(w, dtype=dt)
    sigma_min, ups_alpha, ups_beta, induc_scale = dt(sigma_min), dt(ups_alpha), dt(ups_beta), dt(induc_scale)
    so_lambda, so_alpha, so_beta = dt(so_lambda), dt(so_alpha), dt(so_beta)
    sl = class_slices(K, nf, outlier_mode)
    D = sl['d'].stop
    sx, se, su, sd = sl['x'], sl['err'], sl['ups'], sl['d']
    y = np.asarray(y, dtype=dt)
    assert y.shape == (D,)
    is_exp = np.ones(D, dtype=bool)
    if not pos:
        is_exp[sx] = False
    r = np.where(is_exp, np.exp(y), y)                                     # raw (constrained) parameters
    c = np.ones(D, dtype=dt)                                               # physical variables phi = c r
    c[0], c[1] = 100.0, induc_scale
    c[se] = 0.05
    c[su] = 0.15
    phi = c * r
    Rinf, induc = phi[0], phi[1]
    x = phi[sx]
    sres, ap, ar, ai = phi[se]
    u = phi[su]
    d = phi[sd]
    g = np.zeros(D, dtype=dt); ga = np.zeros(D, dtype=dt)                  # w.r.t. phi; the raw-scale priors join after the chain rule
    lp_terms = []                                                          # arrays of lp's additive terms

    def S_(T, axis=0):
        return _sum(T, axis, reverse)

    # ---- q ~ normal(0, ups):  sum_k -log u_k - 1/2 q_k^2 / u_k^2,  q_k^2 = sum_i d_i (L_i x)_k^2
    v = [S_(Li * x[None, :], 1) for Li in L]
    iu2 = 1.0 / u ** 2
    q2 = d[0] * v[0] ** 2 + d[1] * v[1] ** 2 + d[2] * v[2] ** 2
    lp_terms += [-np.log(u), -0.5 * q2 * iu2]
    for i in range(3):
        T = L[i] * (v[i] * iu2)[:, None]                                   # [k, m]: the rows of L_i^T (v_i / u^2)
        g[sx] += -d[i] * S_(T); ga[sx] += d[i] * S_(np.abs(T))
        t = S_(v[i] ** 2 * iu2)
        g[sd.start + i] += -0.5 * t; ga[sd.start + i] += 0.5 * t
    g[su] += -1.0 / u + q2 / u ** 3; ga[su] += 1.0 / u + q2 / u ** 3
    # ---- dups ~ std_normal:  D_k = 1/2 (u_{k+1} - 1/2 (u_k + u_{k+2})) / u_{k+1},  k = 0 .. K-3
    s2 = u[:-2] + u[2:]; um = u[1:-1]
    Dk = 0.5 * (um - 0.5 * s2) / um
    lp_terms.append(-0.5 * Dk * Dk)
    side = Dk * 0.25 / um                                                  # -D_k dD_k/du_k = -D_k dD_k/du_{k+2}
    mid = -Dk * 0.25 * s2 / um ** 2                                        # -D_k dD_k/du_{k+1}
    for sgn, dst in ((1.0, g), (0.0, ga)):
        a, b = (side, mid) if sgn else (np.abs(side), np.abs(mid))
        dst[su.start:su.stop - 2] += a; dst[su.start + 2:su.stop] += a; dst[su.start + 1:su.stop - 1] += b
    # ---- likelihood: Z ~ normal(Z_hat, sigma_tot), per frequency and part -1/2 log S - 1/2 e^2 / S
    Are, Aim = A[:nf], A[nf:]
    zr = S_(Are * x[None, :], 1) + Rinf
    zi = S_(Aim * x[None, :], 1) + induc * w
    so_re = so_im = np.zeros(nf, dtype=dt)
    if outlier_mode == 1:
        so_raw, so_scale = r[sl['so']][:nf], r[sl['so']][nf:]
        so_re = so_im = dt(0.05) * so_raw * so_scale
    elif outlier_mode == 2:
        so_re, so_im = dt(0.05) * r[sl['so']][:nf], dt(0.05) * r[sl['so']][nf:]
    c0 = sigma_min ** 2 + sres ** 2
    S_re = c0 + (ap * zr) ** 2 + (ar * zr) ** 2 + (ai * zi) ** 2 + so_re ** 2
    S_im = c0 + (ap * zi) ** 2 + (ar * zr) ** 2 + (ai * zi) ** 2 + so_im ** 2
    e_re, e_im = Z[:nf] - zr, Z[nf:] - zi
    lp_terms += [-0.5 * np.log(S_re), -0.5 * e_re ** 2 / S_re, -0.5 * np.log(S_im), -0.5 * e_im ** 2 / S_im]
    # d/de = -e / S (de/dz = -1);  d/dS = -1/(2 S) + e^2 / (2 S^2), absolute terms 1/(2 S) + e^2 / (2 S^2)
    fS_re, fS_im = -0.5 / S_re + 0.5 * e_re ** 2 / S_re ** 2, -0.5 / S_im + 0.5 * e_im ** 2 / S_im ** 2
    aS_re, aS_im = 0.5 / S_re + 0.5 * e_re ** 2 / S_re ** 2, 0.5 / S_im + 0.5 * e_im ** 2 / S_im ** 2
    Gr = e_re / S_re + fS_re * (2 * (ap ** 2 + ar ** 2) * zr) + fS_im * (2 * ar ** 2 * zr)
    Gi = e_im / S_im + fS_im * (2 * (ap ** 2 + ai ** 2) * zi) + fS_re * (2 * ai ** 2 * zi)
    Gr_a = np.abs(e_re) / S_re + aS_re * (2 * (ap ** 2 + ar ** 2) * np.abs(zr)) + aS_im * (2 * ar ** 2 * np.abs(zr))
    Gi_a = np.abs(e_im) / S_im + aS_im * (2 * (ap ** 2 + ai ** 2) * np.abs(zi)) + aS_re * (2 * ai ** 2 * np.abs(zi))
    g[0] += S_(Gr); ga[0] += S_(Gr_a)
    g[1] += S_(Gi * w); ga[1] += S_(Gi_a * w)
    Tr, Ti = Are * Gr[:, None], Aim * Gi[:, None]                          # [n, k]: the frequencies' terms of A^T G
    Tr_a, Ti_a = np.abs(Are) * Gr_a[:, None], np.abs(Aim) * Gi_a[:, None]
    if drop is not None:
        Tr[drop[0], drop[1]] = 0.0; Ti[drop[0], drop[1]] = 0.0
    g[sx] += S_(Tr) + S_(Ti); ga[sx] += S_(Tr_a) + S_(Ti_a)
    for j, (t_re, t_im) in enumerate(((2 * sres, 2 * sres), (2 * ap * zr ** 2, 2 * ap * zi ** 2), (2 * ar * zr ** 2, 2 * ar * zr ** 2),
                                      (2 * ai * zi ** 2, 2 * ai * zi ** 2))):
        g[se.start + j] += S_(fS_re * t_re + fS_im * t_im); ga[se.start + j] += S_(aS_re * t_re + aS_im * t_im)
    # ---- chain rule phi -> raw (diagonal scaling), then what is stated on the raw scale
    g_raw = c * g; ga_raw = c * ga
    if outlier_mode == 1:
        o = sl['so'].start
        dso, dso_a = 2 * so_re * (fS_re + fS_im), 2 * so_re * (aS_re + aS_im)
        g_raw[o:o + nf] += dt(0.05) * so_scale * dso - so_lambda; ga_raw[o:o + nf] += dt(0.05) * so_scale * dso_a + so_lambda
        g_raw[o + nf:o + 2 * nf] += dt(0.05) * so_raw * dso - (so_alpha + 1.0) / so_scale + so_beta / so_scale ** 2
        ga_raw[o + nf:o + 2 * nf] += dt(0.05) * so_raw * dso_a + (so_alpha + 1.0) / so_scale + so_beta / so_scale ** 2
        lp_terms += [-so_lambda * so_raw, -(so_alpha + 1.0) * np.log(so_scale), -so_beta / so_scale]
    elif outlier_mode == 2:
        o = sl['so'].start
        g_raw[o:o + nf] += dt(0.05) * 2 * so_re * fS_re - so_lambda; ga_raw[o:o + nf] += dt(0.05) * 2 * so_re * aS_re + so_lambda
        g_raw[o + nf:o + 2 * nf] += dt(0.05) * 2 * so_im * fS_im - so_lambda
        ga_raw[o + nf:o + 2 * nf] += dt(0.05) * 2 * so_im * aS_im + so_lambda
        lp_terms.append(-so_lambda * r[sl['so']])
    std = np.array([0, 1, se.start, se.start + 1, se.start + 2, se.start + 3])   # ~ std_normal on the raw scale
    lp_terms.append(-0.5 * r[std] ** 2)
    g_raw[std] += -r[std]; ga_raw[std] += r[std]
    rd = r[sd]                                                             # d ~ inv_gamma(5, 5)
    lp_terms += [-6.0 * np.log(rd), -5.0 / rd]
    g_raw[sd] += -6.0 / rd + 5.0 / rd ** 2; ga_raw[sd] += 6.0 / rd + 5.0 / rd ** 2
    ru = r[su]                                                             # ups_raw ~ inv_gamma(ups_alpha, ups_beta)
    lp_terms += [-(ups_alpha + 1.0) * np.log(ru), -ups_beta / ru]
    g_raw[su] += -(ups_alpha + 1.0) / ru + ups_beta / ru ** 2; ga_raw[su] += (ups_alpha + 1.0) / ru + ups_beta / ru ** 2
    # ---- raw -> unconstrained: y = log raw where <lower=0>; the Jacobian's log-determinant is the sum of those y
    t = np.where(is_exp, r, dt(1.0))
    g_y = t * g_raw; ga_y = t * ga_raw
    if jacobian:
        lp_terms.append(y[is_exp])
        g_y = g_y + np.where(is_exp, dt(1.0), dt(0.0)); ga_y = ga_y + np.where(is_exp, dt(1.0), dt(0.0))
    parts = np.array([S_(np.atleast_1d(T)) for T in lp_terms], dtype=dt)
    parts_a = np.array([S_(np.abs(np.atleast_1d(T))) for T in lp_terms], dtype=dt)
    return S_(parts), S_(parts_a), g_y, ga_y


def reference(P, y, jacobian, dtype=np.longdouble, reverse=False, drop=None):
    """the statement at a problem of tests/logp_cases.py (dict A, L, Z, w, pos, K, nf, kw): what logp_mismatch compares against"""
    lp, lp_abs, g, gabs = series_logp(y, P['A'], P['L'], P['Z'], P['w'], pos=P['pos'], jacobian=jacobian, dtype=dtype, reverse=reverse,
                                      drop=drop, **P['kw'])
    return dict(lp=lp, lp_abs=lp_abs, g=g, gabs=gabs, slices=class_slices(P['K'], P['nf'], P['kw'].get('outlier_mode', 0)))


def logp_mismatch(lp, g, ref):
    """{'lp': |lp - lp_ref| / lp_abs, class: max_j |g_j - g_ref_j| / gabs_j} against ref (reference()); a non-finite value, or
    an error where the sum of absolute terms is zero, gives inf."""
    ld = np.longdouble
    g = np.asarray(g)
    out = {}
    with np.errstate(all='ignore'):
        v = abs(ld(lp) - ref['lp']) / ref['lp_abs']
        out['lp'] = float(v) if np.isfinite(v) and np.isfinite(lp) else np.inf
        dg = np.abs(g.astype(ld) - ref['g'])
        for name, s in ref['slices'].items():
            num, den = dg[s], ref['gabs'][s]
            if not np.all(np.isfinite(np.asarray(g[s], dtype=float))) or np.any((den == 0) & (num != 0)) or not np.all(np.isfinite(num)):
                out[name] = np.inf
                continue
            nz = den != 0
            out[name] = float(np.max(num[nz] / den[nz])) if np.any(nz) else 0.0
    return out
