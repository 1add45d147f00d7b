"""Power-scaling prior and likelihood sensitivity of sampling fits, reduced on the GPU.

The model behind `Inverter.fit(mode='sample')` is a regularisation prior against a noisy spectrum, and for every parameter one
wants to know whether the data put its posterior there or the prior did.  The check of Kallioinen, Paananen, Buerkner and
Vehtari ("Detecting and diagnosing prior and likelihood sensitivity with power-scaling", Statistics and Computing 2023; R
package priorsense) answers without a refit: raise the prior to a power alpha near 1, re-weight the draws by Pareto-smoothed
importance sampling, measure how far every marginal posterior moves (the cumulative Jensen-Shannon distance between its ECDF
and the re-weighted one), and do the same with the likelihood.  Definitions: tests/powerscale_numpy.py.  The kernels are in
bdrt_powerscale.hip: the component sums, one workgroup per (fit, component, alpha) for the weights, one per (fit, parameter)
for the distances.  Messages go to logging.getLogger('bayes_drt_amd').

Components: L_lik is the sum of the pointwise log-likelihoods of the points the fit used (the columns `Inverter.loo(part=...)`
selects, on the scaled data), L_pri = lp0 - L_lik with lp0 the log density without the Jacobian term.  The statistic does not
change under an affine map of a column, so x_scale, the Z scale and the raw-scale factors need no undoing: the columns are the
constrained parameters in the layout `Problem.transformed` writes.

Sensitivity of a parameter to a component: (sqrt(cjs2_lower) + sqrt(cjs2_upper)) / (2 log2(upper_alpha)).  Diagnosis with a
threshold of 0.05: prior and likelihood sensitive: 'prior-data conflict'; the prior alone: 'strong prior / weak likelihood';
else '-'.  A Pareto k above 0.7 of a weight vector says that the re-weighting itself is unreliable.

On a sampler's draws (`sampler_powerscale`, `Sampler.powerscale`, `fit(..., powerscale=True)`): everything runs where the
sampler left the draws and only the result planes come back; `powerscale` / `powerscale_many` run the same kernels on host
draws and give the same bits.

Out of scope: `parallel.sample_sharded(powerscale=...)`; sensitivities of derived curves (gamma at eval_tau, Z_hat); selective
power-scaling of single prior terms; moment matching for high k-hat.
"""
import logging

import numpy as np

from . import _lib
from .loo import K_THRESHOLD, PARTS, _draw_count, _sampler_draw_count, _unit_groups, chunk_or_default, part_columns

logger = logging.getLogger('bayes_drt_amd')

# the `powerscale=` request of the engine: every key, with its default
POWERSCALE_DEFAULTS = dict(chains=None, part='both', lower_alpha=0.99, upper_alpha=1.01, threshold=0.05, chunk_bytes=None)
POWERSCALE_KEYS = tuple(POWERSCALE_DEFAULTS)
POWERSCALE_KW = ('lower_alpha', 'upper_alpha', 'threshold')         # what of it `fit_many(powerscale_kw=...)` accepts
LABELS = ('prior-data conflict', 'strong prior / weak likelihood', '-')
COMPONENTS = ('prior', 'likelihood')


class PowerscaleResult(dict):
    """Result of `powerscale`: a dict whose entries also read as attributes -- names, prior, likelihood [D], diagnosis [D],
    cjs2 [D, 2, 2] and pareto_k, n_tail [2, 2] (component x alpha), alphas, threshold, n_draws."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def flagged(self):
        """Names of the parameters whose prior or likelihood sensitivity is at or above the threshold."""
        with np.errstate(invalid='ignore'):
            hit = (np.asarray(self['prior']) >= self['threshold']) | (np.asarray(self['likelihood']) >= self['threshold'])
        return [n for n, h in zip(self['names'], hit) if h]

    def __str__(self):
        rows = ['power-scaling sensitivity: %d draws, alpha = %g, %g, threshold %g; Pareto k prior %.2f, %.2f, likelihood %.2f, %.2f'
                % ((self['n_draws'],) + tuple(self['alphas']) + (self['threshold'],) + tuple(np.asarray(self['pareto_k']).reshape(-1)))]
        flagged = set(self.flagged())
        shown = [i for i, n in enumerate(self['names']) if n in flagged]
        width = max([len('parameter')] + [len(self['names'][i]) for i in shown])
        rows.append('%-*s %10s %10s  %s' % (width, 'parameter', 'prior', 'likelihood', 'diagnosis'))
        for i in shown:
            rows.append('%-*s %10.3g %10.3g  %s' % (width, self['names'][i], self['prior'][i], self['likelihood'][i], self['diagnosis'][i]))
        rows.append('%d of %d parameters at or above the threshold' % (len(shown), len(self['names'])))
        return '\n'.join(rows)


def max_draws():
    """Largest number of draws per fit the distance kernel holds."""
    return int(_lib.load_library().bdrt_powerscale_max_draws())


def check_alphas(lower_alpha, upper_alpha, threshold, who):
    """0 < lower_alpha < 1 < upper_alpha and a threshold >= 0 -> the three as floats; ValueError otherwise."""
    try:
        lo, hi, thr = float(lower_alpha), float(upper_alpha), float(threshold)
    except (TypeError, ValueError):
        raise ValueError('%s: lower_alpha, upper_alpha and threshold must be numbers' % who) from None
    if not (0.0 < lo < 1.0 < hi and np.isfinite(hi)):
        raise ValueError('%s: the powers need 0 < lower_alpha < 1 < upper_alpha (got %r, %r)' % (who, lower_alpha, upper_alpha))
    if not (thr >= 0.0 and np.isfinite(thr)):
        raise ValueError('%s: threshold must be a non-negative number (got %r)' % (who, threshold))
    return lo, hi, thr


def powerscale_request(d, who, need_chains, keys=POWERSCALE_KEYS):
    """The `powerscale=` request of `engine.sample_units` (need_chains), checked without a GPU -> a dict with EVERY key of
    POWERSCALE_KEYS, defaults filled in and 'chains' None where it is not needed: behind this nobody reads a key with a
    default.  keys: what the caller's request may carry."""
    kw = dict(d or {})
    keys = [k for k in keys if need_chains or k != 'chains']
    unknown = sorted(set(kw) - set(keys))
    if unknown:
        raise ValueError('%s: unknown keys %s (%s %s)' % (who, unknown, 'powerscale needs chains and takes' if need_chains else 'known:', keys))
    if need_chains and 'chains' not in kw:
        raise ValueError('%s: powerscale needs chains (got %s)' % (who, sorted(kw)))
    req = dict(POWERSCALE_DEFAULTS, **kw)
    if req['part'] not in PARTS:
        raise ValueError("part must be 'both', 'real' or 'imag'")
    req['lower_alpha'], req['upper_alpha'], req['threshold'] = check_alphas(req['lower_alpha'], req['upper_alpha'], req['threshold'], who)
    chunk_or_default(req['chunk_bytes'])
    return req


def check_powerscale_kw(powerscale_kw, part='both'):
    """`fit_many(powerscale_kw=...)` -> dict(part, lower_alpha, upper_alpha, threshold), checked without a GPU; the part is
    the fit's."""
    req = powerscale_request(powerscale_kw, 'powerscale_kw', False, POWERSCALE_KW)
    if part not in PARTS:
        raise ValueError("part must be 'both', 'real' or 'imag'")
    return dict(part=part, lower_alpha=req['lower_alpha'], upper_alpha=req['upper_alpha'], threshold=req['threshold'])


def sensitivity(cjs2, upper_alpha):
    """cjs2 [..., 2] (alpha lower, upper) -> (sqrt(lower) + sqrt(upper)) / (2 log2(upper_alpha))."""
    cjs2 = np.asarray(cjs2, dtype=float)
    with np.errstate(invalid='ignore'):
        return (np.sqrt(cjs2[..., 0]) + np.sqrt(cjs2[..., 1])) / (2.0 * np.log2(upper_alpha))


def diagnose(prior, likelihood, threshold):
    """The label of every parameter; a NaN sensitivity compares false, so it reads '-'."""
    out = []
    for p, l in zip(np.atleast_1d(prior), np.atleast_1d(likelihood)):
        out.append(LABELS[2] if not p >= threshold else (LABELS[0] if l >= threshold else LABELS[1]))
    return out


def parameter_names(problem, model=None):
    """Flat names of the D constrained parameters in the layout `Problem.transformed` writes: the model's Stan names when the
    `StanModel` is given, block-numbered ones otherwise."""
    from .diagnostics import flatnames
    lay, nb = problem.layout(), len(problem.Ks)
    n = getattr(model, '_names', None)
    raw = n['raw'] if n else ['x%d' % b for b in range(nb)]
    ups = n['ups'] if n else ['ups%d_raw' % b for b in range(nb)]
    dn = n['d'] if n else [tuple('d%d_%d_strength' % (i, b) for i in range(3)) for b in range(nb)]
    names = [None] * problem.D
    names[0], names[1] = 'Rinf_raw', 'induc_raw'
    for b, K in enumerate(problem.Ks):
        names[lay['x'][b]:lay['x'][b] + K] = flatnames(raw[b], K, False)
        names[lay['ups'][b]:lay['ups'][b] + K] = flatnames(ups[b], K, False)
        names[lay['d'][b]:lay['d'][b] + 3] = list(dn[b])
    names[lay['err']:lay['err'] + 4] = ['sigma_res_raw', 'alpha_prop_raw', 'alpha_re_raw', 'alpha_im_raw']
    mode, nf, so = int(problem.dat.outlier_mode), problem.nf, lay['so']
    if mode == 1:
        names[so:so + nf] = flatnames('sigma_out_raw', nf, False)
        names[so + nf:so + 2 * nf] = flatnames('sigma_out_scale', nf, False)
    elif mode:
        names[so:so + 2 * nf] = flatnames('sigma_out_raw', 2 * nf, False)
    assert all(nm is not None for nm in names) and len(names) == problem.D
    return names


def _result(cjs2, pareto_k, n_tail, names, lower_alpha, upper_alpha, threshold, S, prefix='', part='both'):
    """Kernel outputs of one fit (cjs2 [D, 4], pareto_k, n_tail [4]) -> PowerscaleResult; logs one line."""
    cjs2 = np.array(cjs2, dtype=float).reshape(-1, 2, 2)
    k, nt = np.array(pareto_k, dtype=float).reshape(2, 2), np.array(n_tail, dtype=np.int32).reshape(2, 2)
    sens = sensitivity(cjs2, upper_alpha)
    res = PowerscaleResult(names=list(names), prior=sens[:, 0], likelihood=sens[:, 1],
                           diagnosis=diagnose(sens[:, 0], sens[:, 1], threshold), cjs2=cjs2, pareto_k=k, n_tail=nt,
                           alphas=(float(lower_alpha), float(upper_alpha)), threshold=float(threshold), n_draws=int(S), part=part)
    n_conf, n_strong = res['diagnosis'].count(LABELS[0]), res['diagnosis'].count(LABELS[1])
    with np.errstate(invalid='ignore'):
        bad = bool(np.any(np.isnan(k)) or np.any(k[np.isfinite(k)] > K_THRESHOLD))
    logger.log(logging.WARNING if bad else logging.INFO,
               '%spower-scaling sensitivity: %d of %d parameters in prior-data conflict, %d with a strong prior / weak likelihood '
               '(threshold %g); Pareto k of the weights %s%s', prefix, n_conf, len(res['names']), n_strong, threshold,
               np.array2string(k.reshape(-1), precision=2),
               ': above %.1f the re-weighting is unreliable' % K_THRESHOLD if bad else '')
    return res


# ---------------------------------------------------------------------------------------------------- device reductions
def debug_cjs(X, w):
    """The distance kernel on constructed input (bdrt_debug_powerscale_cjs): columns X [C, S] and weights w [4, S], taken as
    they are -> cjs2 [C, 4]."""
    X, w = np.atleast_2d(_lib.f64(X)), _lib.f64(w)
    C, S = X.shape
    if w.shape != (4, S):
        raise ValueError('debug_cjs: w must be [4, %d], not %s' % (S, w.shape))
    _draw_count(S, 'powerscale', max_draws, 'fit')
    lib = _lib.require_gpu()
    out = np.empty((C, 4))
    _lib.check(lib.bdrt_debug_powerscale_cjs(_lib.ptr(X), _lib.ptr(w), C, S, _lib.ptr(out)), 'bdrt_debug_powerscale_cjs')
    return out


def debug_weights(L, lower_alpha=0.99, upper_alpha=1.01):
    """The weights kernel on constructed components (bdrt_debug_powerscale_weights): L [G, 2, S] (or [2, S]: G = 1) -> dict of
    lw, w [G, 4, S], pareto_k (float) and n_tail (int) [G, 4], in the order (prior, likelihood) x (lower, upper)."""
    L = _lib.f64(L)
    one = L.ndim == 2
    if one:
        L = L[None]
    if L.ndim != 3 or L.shape[1] != 2:
        raise ValueError('debug_weights: L must be [G, 2, S] or [2, S]')
    G, _, S = L.shape
    lo, hi, _ = check_alphas(lower_alpha, upper_alpha, 0.0, 'powerscale')
    _draw_count(S, 'powerscale', max_draws, 'fit')
    lib = _lib.require_gpu()
    lw, w = np.empty((G, 4, S)), np.empty((G, 4, S))
    k, nt = np.empty((G, 4)), np.empty((G, 4), dtype=np.int32)
    _lib.check(lib.bdrt_debug_powerscale_weights(_lib.ptr(L), G, S, lo, hi, _lib.ptr(lw), _lib.ptr(w), _lib.ptr(k), _lib.ptr(nt)),
               'bdrt_debug_powerscale_weights')
    res = dict(lw=lw, w=w, pareto_k=k, n_tail=nt)
    return {key: v[0] for key, v in res.items()} if one else res


def host_powerscale(problem, draws, chains, spec=None, part='both', lower_alpha=0.99, upper_alpha=1.01, chunk_bytes=None,
                    components=False):
    """What `sampler_powerscale` computes, on host-resident unconstrained draws [G, chains * n_draws, D] (bdrt_powerscale):
    spec [G] is the spectrum of the problem each fit was sampled against (None: 0).  Returns a dict of cjs2 [G, D, 4],
    pareto_k (float) and n_tail (int) [G, 4]; components=True adds 'L' [G, 2, S]: L_pri and L_lik of every draw."""
    who = 'powerscale'
    if part not in PARTS:
        raise ValueError("part must be 'both', 'real' or 'imag'")
    lo, hi, _ = check_alphas(lower_alpha, upper_alpha, 0.0, who)
    draws = _lib.f64(draws)
    if draws.ndim != 3 or draws.shape[2] != problem.D:
        raise ValueError('%s: draws must be [G, S, %d], not %s' % (who, problem.D, draws.shape))
    G, S, D = draws.shape
    chains = int(chains)
    if chains < 1 or S % chains:
        raise ValueError('%s: %d draws do not split into %d chains' % (who, S, chains))
    _draw_count(S, who, max_draws, 'fit')
    sp = None
    if spec is not None:
        sp = np.ascontiguousarray(np.asarray(spec, dtype=np.int32))
        if sp.shape != (G,):
            raise ValueError('%s: spec must have one entry per fit' % who)
    col0, ncols = part_columns(part, problem.nf)
    cjs2, k, nt = np.empty((G, D, 4)), np.empty((G, 4)), np.empty((G, 4), dtype=np.int32)
    L = np.empty((G, 2, S)) if components else None
    _lib.check(problem._lib.bdrt_powerscale(problem.handle, _lib.ptr(draws), _lib.ptr(sp), G, chains, S // chains, col0, ncols, lo, hi,
                                            chunk_or_default(chunk_bytes), _lib.ptr(cjs2), _lib.ptr(k), _lib.ptr(nt), _lib.ptr(L)),
               'bdrt_powerscale')
    res = dict(cjs2=cjs2, pareto_k=k, n_tail=nt)
    if components:
        res['L'] = L
    return res


def sampler_powerscale(sampler, unit_lo, unit_hi, chains, part='both', lower_alpha=0.99, upper_alpha=1.01, chunk_bytes=None):
    """The check on the draws a sampler holds in HBM (bdrt_sampler_powerscale): units [unit_lo, unit_hi) in groups of `chains`
    consecutive units that sampled one spectrum; the data are the problem's own device copy of that spectrum.  part: 'both', or
    'real' / 'imag' when only that half of the scalar observations is the likelihood.  Neither the draws nor anything evaluated
    on them leaves the device, which works in chunks of groups whose scratch stays within `chunk_bytes` (None: 1 GiB).  Returns
    a dict of cjs2 [G, D, 4] -- per constrained parameter (prior, likelihood) x (lower, upper) --, pareto_k and n_tail [G, 4];
    every entry equals `host_powerscale` on the downloaded draws bit for bit."""
    who = 'powerscale'
    if part not in PARTS:
        raise ValueError("part must be 'both', 'real' or 'imag'")
    lo, hi, _ = check_alphas(lower_alpha, upper_alpha, 0.0, who)
    unit_lo, unit_hi, chains, G = _unit_groups(sampler, unit_lo, unit_hi, chains, who)
    _sampler_draw_count(sampler, chains, who, max_draws, 'fit')
    col0, ncols = part_columns(part, sampler.problem.nf)
    D = sampler.problem.D
    cjs2, k, nt = np.empty((G, D, 4)), np.empty((G, 4)), np.empty((G, 4), dtype=np.int32)
    _lib.check(sampler._lib.bdrt_sampler_powerscale(sampler.handle, unit_lo, unit_hi, chains, col0, ncols, lo, hi,
                                                    chunk_or_default(chunk_bytes), _lib.ptr(cjs2), _lib.ptr(k), _lib.ptr(nt)),
               'bdrt_sampler_powerscale')
    return dict(cjs2=cjs2, pareto_k=k, n_tail=nt)


# ---------------------------------------------------------------------------------------------------- fits
def _fit_job(fit, who):
    """(problem, model, unconstrained draws [S, D], chains) of a live sampling fit."""
    model, theta = getattr(fit, '_model', None), getattr(fit, 'theta', None)
    if model is None or getattr(model, 'problem', None) is None or theta is None:
        raise ValueError('%s needs a live sampling fit (the log density of the draws is evaluated on the GPU); a fit restored '
                         'from a file carries the result it was saved with, not the model' % who)
    return model.problem, model, np.asarray(theta, dtype=float), int(getattr(fit, 'chains', 1))


def _part_of(columns, nf, who):
    """The part a `columns` slice of `Inverter._loo_job` stands for."""
    if columns is None:
        return 'both'
    for part in ('real', 'imag'):
        col0, ncols = part_columns(part, nf)
        if isinstance(columns, slice) and (columns.start, columns.stop, columns.step) in ((col0, col0 + ncols, None), (col0, col0 + ncols, 1)):
            return part
    raise ValueError('%s: columns must be None or the slice of the real or the imaginary half' % who)


def _fit_z(problem, z, who):
    z = np.asarray(z, dtype=float).reshape(-1)
    if z.shape[0] != 2 * problem.nf:
        raise ValueError('%s: the data must have %d entries, not %d' % (who, 2 * problem.nf, z.shape[0]))
    return z


def powerscale_many(fits, zs, columns=None, lower_alpha=0.99, upper_alpha=1.01, threshold=0.05, chunk_bytes=None, spec=None):
    """`powerscale` of many fits: fits that share their problem and their number of draws go through one call of the kernels.
    The data a fit is weighed against are its problem's own device copy of the spectrum it was sampled against: spec gives, per
    fit, which one that is (None: 0 for all; `Inverter.powerscale_many` passes the views' own), and zs is checked for its length
    only.  Results in input order, each equal to the single-fit `powerscale` bit for bit."""
    who = 'powerscale'
    lo, hi, thr = check_alphas(lower_alpha, upper_alpha, threshold, who)
    n = len(fits)
    spec = [0] * n if spec is None else [int(s) for s in spec]
    jobs = [_fit_job(f, who) for f in fits]
    groups = {}
    for i, (prob, model, theta, ch) in enumerate(jobs):
        _fit_z(prob, zs[i], who)
        groups.setdefault((id(prob), theta.shape, ch), []).append(i)
    out = [None] * n
    for idx in groups.values():
        prob, model, _, ch = jobs[idx[0]]
        part = _part_of(columns, prob.nf, who)
        names = parameter_names(prob, model)
        r = host_powerscale(prob, np.stack([jobs[i][2] for i in idx]), ch, [spec[i] for i in idx], part, lo, hi, chunk_bytes)
        for g, i in enumerate(idx):
            out[i] = _result(r['cjs2'][g], r['pareto_k'][g], r['n_tail'][g], names, lo, hi, thr, jobs[i][2].shape[0],
                             'fit %d: ' % i if n > 1 else '', part)
    return out


def powerscale(fit, z, columns=None, lower_alpha=0.99, upper_alpha=1.01, threshold=0.05, spec=0):
    """Power-scaling sensitivity of a sampling fit (`StanFit`) against the data z [2 Nf] it was fitted to, which its problem
    holds as spectrum `spec`.  columns: None, or the slice of the real or the imaginary half when only that half is the
    likelihood (`Inverter._loo_job`).  Returns a `PowerscaleResult`."""
    return powerscale_many([fit], [z], columns, lower_alpha, upper_alpha, threshold, None, [spec])[0]
