"""Model comparison and predictive checks of sampling fits: PSIS-LOO and WAIC (`loo`, `compare`) and the leave-one-out
predictive distribution of every observation (`loo_predict`: LOO-PIT and LOO residuals), reduced on the GPU.

Stan users rank fits of one data set by the expected log pointwise predictive density, estimated by leave-one-out
cross-validation of the posterior with Pareto-smoothed importance sampling (Vehtari, Gelman, Gabry 2017), and by WAIC.  Every
model text ends in `Z ~ normal(Z_hat, sigma_tot)`, so the pointwise log-likelihood of a draw follows from `fit['Z_hat']` and
`fit['sigma_tot']`.  The reductions run in bdrt_loo.hip (`bdrt_pointwise_loglik`, `bdrt_psis_loo`: one workgroup per
observation); the definitions are written out in tests/psis_numpy.py.  Messages go to logging.getLogger('bayes_drt_amd').

Units: an observation is one frequency (`unit='frequency'`: real plus imaginary part, the default) or one scalar
(`unit='point'`).  The Pareto shape k-hat of an observation says how much the posterior hinges on it: above 0.7 the
importance-sampling estimate for that observation is unreliable (and the observation is influential).

Predictive checks (`loo_predict`): the LOO predictive distribution of a scalar observation is the mixture of the draws'
normals under the smoothed weights of its unit, so its mean, its sd and its cdf at the datum (the LOO-PIT, uniform on (0, 1)
when the error model is calibrated) are weighted sums over the draws (bdrt_loo_predict.hip, `bdrt_psis_predict`; definitions in
tests/loo_predict_numpy.py).  The residual (z - mean) / sd judges a point by a fit that has not seen it, unlike the in-sample
z-score of `Inverter.check_outliers`.  Among equal log ratios in the tail the draw with the smaller index gets the smaller
smoothed weight.

On a sampler's draws (`sampler_psis_loo`, `sampler_psis_predict`; `Sampler.loo`, `Sampler.loo_predict`): the same two reductions
where the sampler left the draws, in HBM (bdrt_sampler_loo, bdrt_sampler_loo_predict).  The batch evaluator gives Z_hat and
sigma_tot of the draws in chunks of spectra, the kernels above reduce them against the problem's own device copy of each
spectrum, and only the per-observation results come back.  `Inverter.fit_many(..., loo=True, loo_predict=True)` and
`parallel.sample_sharded(..., loo=...)` use it, the latter with each rank reducing its own spectra, so that gather='summary' has
a LOO result although no draw leaves a GPU.  With reff None, a number or an array the results equal the host path on the
downloaded draws bit for bit (`host_psis_loo`, `host_psis_predict` are that path on stacked draws); reff='auto' is reduced on the
device too (exp(ll - max ll) per observation, then the kernel of `column_diagnostics`), and since the device's exp is not numpy's,
the relative efficiency may differ from `relative_efficiency` in its last bits: the result carries the 'reff' that was used.

Held-out frequencies (`heldout_transformed`, `heldout_reduce`; `sampler_heldout`, `host_heldout`; `Sampler.heldout`): what the
draws of a fit on a training grid predict at frequencies that are not on it -- Z_hat and sigma_tot of every draw there
(bdrt_heldout.hip), then the equal-weight mixture of the draws' normals: lpd, mean, sd and PIT per held-out unit.  This is the
exact remedy for observations PSIS flags: `Inverter.reloo` refits without each of them, `Inverter.kfold_many` runs K folds of
many spectra as K batches; both give `LooResult`s that `compare` ranks.  Definitions: tests/heldout_numpy.py.  Outlier error
models are refused by default: every training point has its own sigma_out and a held-out point has none.  With the keyword
sigma_out='prior' a held-out point's sigma_out is integrated over its prior, which data alone fix (`sigma_out_prior_table`,
`heldout_mix_reduce`, bdrt_heldout_mix.hip; tests/heldout_mix_numpy.py).

Out of scope: moment matching for high-k observations; a marginal PSIS-LOO for the outlier error models (the point's own
sigma_out integrated out of the importance ratios); stacking weights; LOO of
MAP or ridge fits; predictive checks with replicated data, plots, and a `fit_many` that keeps no draws at all.
"""
import logging

import numpy as np

from . import _lib

logger = logging.getLogger('bayes_drt_amd')

K_THRESHOLD = 0.7
UNITS = ('frequency', 'point')
CHUNK_BYTES = 1 << 30                                # loo_many: host bytes of one chunk's stacked arrays


class LooResult(dict):
    """Result of `loo`: a dict whose entries also read as attributes."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class LooPredictResult(LooResult):
    """Result of `loo_predict`: a dict whose entries also read as attributes."""


def max_draws():
    """Largest number of draws per observation the kernel holds."""
    return int(_lib.load_library().bdrt_psis_loo_max_draws())


def predict_max_draws():
    """Largest number of draws per unit `psis_predict` holds."""
    return int(_lib.load_library().bdrt_psis_predict_max_draws())


def _pair(unit):
    if unit not in UNITS:
        raise ValueError("unit must be 'frequency' or 'point', not %r" % (unit,))
    return 1 if unit == 'frequency' else 0


# ---------------------------------------------------------------------------------------------------- device reductions
def _stacked(who, Zhat, sig, z, unit):
    """Zhat, sig [G, S, N2] and z [G, N2] (or [S, N2] and [N2]: G = 1, `one`) as contiguous float64 arrays of three and two
    dimensions -> (pair, Zhat, sig, z, one)."""
    pair = _pair(unit)
    Zhat, sig, z = _lib.f64(Zhat), _lib.f64(sig), _lib.f64(z)
    one = Zhat.ndim == 2
    if one:
        Zhat, sig, z = Zhat[None], sig[None], z[None]
    if Zhat.ndim != 3 or sig.shape != Zhat.shape or z.shape != (Zhat.shape[0], Zhat.shape[2]):
        raise ValueError('%s: shapes %s, %s, %s do not fit' % (who, Zhat.shape, sig.shape, z.shape))
    if pair and Zhat.shape[2] % 2:
        raise ValueError("%s: unit='frequency' needs an even number of columns, not %d" % (who, Zhat.shape[2]))
    return pair, Zhat, sig, z, one


def pointwise_log_lik(Zhat, sig, z, unit='frequency'):
    """Log-likelihood of `Z ~ normal(Z_hat, sigma_tot)` per draw and observation on the GPU: Zhat, sig [G, S, 2 Nf] and z
    [G, 2 Nf] (or [S, 2 Nf] and [2 Nf]: G = 1) -> [G, S, Nf] (unit='frequency': real plus imaginary part) or [G, S, 2 Nf]
    (unit='point').  A non-positive or non-finite sig gives NaN."""
    pair, Zhat, sig, z, one = _stacked('pointwise_log_lik', Zhat, sig, z, unit)
    G, S, N2 = Zhat.shape
    lib = _lib.require_gpu()
    out = np.empty((G, S, N2 // 2 if pair else N2))
    _lib.check(lib.bdrt_pointwise_loglik(_lib.ptr(Zhat), _lib.ptr(sig), _lib.ptr(z), G, S, N2, pair, _lib.ptr(out)),
               'bdrt_pointwise_loglik')
    return out[0] if one else out


def psis_loo(ll, reff=None):
    """PSIS-LOO and WAIC per column of ll [G, S, N] (or [S, N]: G = 1) on the GPU.  reff: None (1), a number, or [G, N].
    Returns a dict of lpd, elpd_loo, p_loo, pareto_k, p_waic, elpd_waic (float) and n_tail (int), each [G, N] ([N])."""
    ll = _lib.f64(ll)
    one = ll.ndim == 2
    if one:
        ll = ll[None]
    if ll.ndim != 3:
        raise ValueError('psis_loo: ll must be [S, N] or [G, S, N]')
    G, S, N = ll.shape
    _draw_count(S, 'psis_loo', max_draws, 'observation')
    r = None
    if reff is not None:
        r = _lib.f64(np.broadcast_to(np.asarray(reff, dtype=float), (G, N)))
        if not np.all(np.isfinite(r) & (r > 0)):
            raise ValueError('psis_loo: reff must be positive and finite')
    lib = _lib.require_gpu()
    outs = [np.empty((G, N)) for _ in range(4)]
    n_tail = np.empty((G, N), dtype=np.int32)
    _lib.check(lib.bdrt_psis_loo(_lib.ptr(ll), G, S, N, _lib.ptr(r), *[_lib.ptr(o) for o in outs], _lib.ptr(n_tail)),
               'bdrt_psis_loo')
    lpd, elpd, k, pw = [o[0] for o in outs] if one else outs
    return {'lpd': lpd, 'elpd_loo': elpd, 'p_loo': lpd - elpd, 'pareto_k': k, 'p_waic': pw, 'elpd_waic': lpd - pw,
            'n_tail': n_tail[0] if one else n_tail}


PREDICT_FIELDS = ('mean', 'sd', 'pit', 'mean_post', 'sd_post', 'pit_post')


def psis_predict(Zhat, sig, z, unit='frequency', reff=None):
    """LOO predictive moments per scalar observation on the GPU: Zhat, sig [G, S, 2 Nf] and z [G, 2 Nf] (or [S, 2 Nf] and
    [2 Nf]: G = 1).  A unit is one frequency (real plus imaginary part left out together) or one point; reff: None (1), a
    number, or [G, units].  Returns a dict of mean, sd, pit (LOO) and mean_post, sd_post, pit_post (equal weights), each
    [G, 2 Nf], and pareto_k (float), n_tail (int) [G, units] -- those two equal `psis_loo(pointwise_log_lik(...), reff)`'s."""
    pair, Zhat, sig, z, one = _stacked('psis_predict', Zhat, sig, z, unit)
    G, S, N2 = Zhat.shape
    _draw_count(S, 'psis_predict', predict_max_draws)
    U = N2 // 2 if pair else N2
    r = None
    if reff is not None:
        r = _lib.f64(np.broadcast_to(np.asarray(reff, dtype=float), (G, U)))
        if not np.all(np.isfinite(r) & (r > 0)):
            raise ValueError('psis_predict: reff must be positive and finite')
    lib = _lib.require_gpu()
    outs = [np.empty((G, N2)) for _ in PREDICT_FIELDS]
    k, n_tail = np.empty((G, U)), np.empty((G, U), dtype=np.int32)
    _lib.check(lib.bdrt_psis_predict(_lib.ptr(Zhat), _lib.ptr(sig), _lib.ptr(z), G, S, N2, pair, _lib.ptr(r),
                                     *[_lib.ptr(o) for o in outs], _lib.ptr(k), _lib.ptr(n_tail)), 'bdrt_psis_predict')
    res = dict(zip(PREDICT_FIELDS, outs), pareto_k=k, n_tail=n_tail)
    return {key: v[0] for key, v in res.items()} if one else res


# ---------------------------------------------------------------------------------------------------- on a sampler's draws
PARTS = ('both', 'real', 'imag')
# the `loo=` and `heldout=` requests of the engine: every key, with its default or among those that must be given
LOO_DEFAULTS = dict(chains=None, loo=True, predict=False, unit='frequency', part='both', reff='auto', chunk_bytes=None)
LOO_KEYS = tuple(LOO_DEFAULTS)
LOO_KW = ('unit', 'reff')                            # what of it `fit_many(loo_kw=...)` accepts
HELDOUT_NEEDS = ('chains', 'freq_test', 'A_test_blocks', 'z_test')
HELDOUT_DEFAULTS = dict(unit='frequency', part='both', chunk_bytes=None, sigma_out=None)
HELDOUT_KEYS = HELDOUT_NEEDS + tuple(HELDOUT_DEFAULTS)


def effective_unit(unit, part):
    """A fit (or a request) of one part has points for units."""
    return 'point' if part != 'both' else unit


def part_columns(part, n):
    """(first column, number of columns) of a part among 2 n columns, real halves first; the slice is
    slice(col0, col0 + ncols)."""
    return {'both': (0, 2 * n), 'real': (0, n), 'imag': (n, n)}[part]


def check_device_args(unit='frequency', part='both', reff='auto', who='loo'):
    """The checks of the device path that need neither a GPU nor the draws: (pair, reff mode 0 / 1 / 2).  Messages are the
    host path's."""
    pair = _pair(unit)
    if part not in PARTS:
        raise ValueError("part must be 'both', 'real' or 'imag'")
    if pair and part != 'both':
        raise ValueError("%s: unit='frequency' needs part='both' (a half of the columns has points for units)" % who)
    if isinstance(reff, str):
        if reff != 'auto':
            raise ValueError("reff must be 'auto', None, a number or an array")
        return pair, 2
    if reff is not None and not np.all(np.isfinite(np.asarray(reff, dtype=float)) & (np.asarray(reff, dtype=float) > 0)):
        raise ValueError('%s: reff must be positive and finite' % who)
    return pair, 0 if reff is None else 1


def chunk_or_default(chunk_bytes):
    """`chunk_bytes` of the device path: None -> 0, the library's default (1 GiB of device scratch per chunk)."""
    if chunk_bytes is None:
        return 0
    if int(chunk_bytes) < 0:
        raise ValueError('chunk_bytes must not be negative')
    return int(chunk_bytes)


def loo_request(loo, who, need_chains, keys=LOO_KEYS):
    """The `loo=` request of `engine.sample_units` (need_chains) and `parallel.sample_sharded` (the chains are an argument of
    its own there), checked without a GPU -> a dict with EVERY key of LOO_KEYS, defaults filled in and 'chains' None where it
    is not needed: behind this nobody reads a key with a default.  keys: what the caller's request may carry."""
    kw = dict(loo or {})
    keys = [k for k in keys if need_chains or k != 'chains']
    unknown = sorted(set(kw) - set(keys))
    if unknown:
        raise ValueError('%s: unknown keys %s (%s %s)' % (who, unknown, 'loo needs chains and takes' if need_chains else 'known:', keys))
    if need_chains and 'chains' not in kw:
        raise ValueError('%s: loo needs chains (got %s)' % (who, sorted(kw)))
    req = dict(LOO_DEFAULTS, **kw)
    check_device_args(req['unit'], req['part'], req['reff'], who)
    chunk_or_default(req['chunk_bytes'])
    return req


def check_loo_kw(loo_kw, part='both'):
    """`fit_many(loo_kw=...)` -> dict(unit, reff), checked without a GPU.  A fit of one part has points for units, as `loo` of
    such a fit has."""
    req = loo_request(loo_kw, 'loo_kw', False, LOO_KW)
    unit = effective_unit(req['unit'], part)
    check_device_args(unit, part, req['reff'])
    return dict(unit=unit, reff=req['reff'])


def heldout_request(heldout, problem, who):
    """The `heldout=` request of `engine.sample_units`, checked against the problem without a GPU -> a dict with every key of
    HELDOUT_KEYS, defaults filled in."""
    kw = dict(heldout)
    if set(kw) - set(HELDOUT_KEYS) or not set(HELDOUT_NEEDS) <= set(kw):
        raise ValueError('%s: heldout needs %s and takes %s (got %s)' % (who, ', '.join(HELDOUT_NEEDS), ', '.join(HELDOUT_DEFAULTS), sorted(kw)))
    req = dict(HELDOUT_DEFAULTS, **kw)
    freq, _ = _heldout_grid(problem, req['freq_test'], req['A_test_blocks'], 'heldout', req['sigma_out'])
    _heldout_part(req['unit'], req['part'], len(freq), 'heldout')
    chunk_or_default(req['chunk_bytes'])
    return req


def _unit_groups(sampler, unit_lo, unit_hi, chains, who):
    """Units [unit_lo, unit_hi) of a sampler in groups of `chains` consecutive units -> (unit_lo, unit_hi, chains, G), ints."""
    chains, unit_lo, unit_hi = int(chains), int(unit_lo), int(unit_hi)
    if chains < 1 or unit_lo < 0 or unit_hi > sampler.n_units or unit_hi <= unit_lo or (unit_hi - unit_lo) % chains:
        raise ValueError('%s: units [%d, %d) do not split into groups of %d chains' % (who, unit_lo, unit_hi, chains))
    return unit_lo, unit_hi, chains, (unit_hi - unit_lo) // chains


def _draw_count(S, who, limit, per='unit'):
    """2 <= S <= limit(): the kernel's limit is asked of the library only when it decides."""
    if S < 2:
        raise ValueError('%s: at least 2 draws are needed' % who)
    if S > limit():
        raise ValueError('%s: %d draws per %s, the kernel holds at most %d' % (who, S, per, limit()))


def _sampler_draw_count(sampler, chains, who, limit, per='unit'):
    if sampler.n_draws < 1:
        raise ValueError('%s: the sampler holds no draws' % who)
    _draw_count(chains * sampler.n_draws, who, limit, per)


def _sampler_front(sampler, unit_lo, unit_hi, chains, unit, part, reff, chunk_bytes, who, limit):
    """Checks and the common leading arguments of the two entry points; `r` keeps the reff array alive for the call."""
    pair, mode = check_device_args(unit, part, reff, who)
    unit_lo, unit_hi, chains, G = _unit_groups(sampler, unit_lo, unit_hi, chains, who)
    _sampler_draw_count(sampler, chains, who, limit, 'observation')
    col0, ncols = part_columns(part, sampler.problem.nf)
    U = ncols // 2 if pair else ncols
    r = None
    if mode == 1:
        r = _lib.f64(np.broadcast_to(np.asarray(reff, dtype=float), (G, U)))
    front = (sampler.handle, unit_lo, unit_hi, chains, pair, col0, ncols, mode, _lib.ptr(r), chunk_or_default(chunk_bytes))
    return front, r, G, U, ncols


def sampler_psis_loo(sampler, unit_lo, unit_hi, chains, unit='frequency', part='both', reff='auto', chunk_bytes=None):
    """`psis_loo(pointwise_log_lik(...))` of the draws a sampler holds in HBM (bdrt_sampler_loo): units [unit_lo, unit_hi) in
    groups of `chains` consecutive units that sampled one spectrum; the data are the problem's own device copy of that spectrum.
    part: 'both', or 'real' / 'imag' for that half of the scalar observations (units are points then).  reff: 'auto' (the
    relative efficiency of the likelihood draws, reduced on the device), None (1), a number or [G, units].  Neither the draws
    nor Z_hat, sigma_tot or the log-likelihoods leave the device, which evaluates them in chunks of groups whose scratch stays
    within `chunk_bytes` (None: 1 GiB).  Returns `psis_loo`'s dict, each entry [G, units], plus 'reff', what was used.  With
    reff None, a number or an array every entry equals the host path on the downloaded draws bit for bit."""
    front, r, G, U, _ = _sampler_front(sampler, unit_lo, unit_hi, chains, unit, part, reff, chunk_bytes, 'psis_loo', max_draws)
    outs = [np.empty((G, U)) for _ in range(4)]
    n_tail, used = np.empty((G, U), dtype=np.int32), np.empty((G, U))
    _lib.check(sampler._lib.bdrt_sampler_loo(*front, *[_lib.ptr(o) for o in outs], _lib.ptr(n_tail), _lib.ptr(used)),
               'bdrt_sampler_loo')
    lpd, elpd, k, pw = outs
    return {'lpd': lpd, 'elpd_loo': elpd, 'p_loo': lpd - elpd, 'pareto_k': k, 'p_waic': pw, 'elpd_waic': lpd - pw,
            'n_tail': n_tail, 'reff': used}


def sampler_psis_predict(sampler, unit_lo, unit_hi, chains, unit='frequency', part='both', reff='auto', chunk_bytes=None):
    """`psis_predict` of the draws a sampler holds in HBM (bdrt_sampler_loo_predict); arguments as `sampler_psis_loo`.  Returns
    `psis_predict`'s dict -- the six per-scalar entries [G, columns of the part], pareto_k and n_tail [G, units] -- plus
    'reff'."""
    front, r, G, U, ncols = _sampler_front(sampler, unit_lo, unit_hi, chains, unit, part, reff, chunk_bytes,
                                           'psis_predict', predict_max_draws)
    outs = [np.empty((G, ncols)) for _ in PREDICT_FIELDS]
    k, n_tail, used = np.empty((G, U)), np.empty((G, U), dtype=np.int32), np.empty((G, U))
    _lib.check(sampler._lib.bdrt_sampler_loo_predict(*front, *[_lib.ptr(o) for o in outs], _lib.ptr(k), _lib.ptr(n_tail),
                                                     _lib.ptr(used)), 'bdrt_sampler_loo_predict')
    return dict(zip(PREDICT_FIELDS, outs), pareto_k=k, n_tail=n_tail, reff=used)


# ---------------------------------------------------------------------------------------------------- held-out frequencies
HELDOUT_FIELDS = ('mean', 'sd', 'pit')
OUTLIER_REFUSAL = ('held-out prediction is not defined for the outlier error models (*_outliers): every training point has its '
                   'own sigma_out and a held-out point has none')


def _outlier_mode(problem):
    return int(getattr(getattr(problem, 'dat', None), 'outlier_mode', 0))


def check_sigma_out(sigma_out, who):
    """The `sigma_out=` keyword of the held-out entries: None (the outlier error models are refused) or 'prior' (their
    sigma_out is integrated over its prior, `sigma_out_prior_table`).  ValueError for anything else."""
    if sigma_out is not None and not (isinstance(sigma_out, str) and sigma_out == 'prior'):
        raise ValueError("%s: sigma_out must be None or 'prior', not %r" % (who, sigma_out))
    return sigma_out


def sigma_out_table(mode, so_lambda, so_alpha=5.0, so_beta=1.0, step=0.125):
    """The prior of sigma_out as an integration rule -> (y [Q], w [Q], E[y^2], shared): sum_j w_j f(y_j) ~ E f(sigma_out).

    mode 1 (`Series*_outliers`): sigma_out = 0.05 raw scale, raw ~ exponential(so_lambda), scale ~ inv_gamma(so_alpha, so_beta).
    raw / (1 / scale) with 1 / scale ~ gamma(so_alpha, rate so_beta): P(y > t) = (1 + t / s)^-so_alpha, s = 0.05 so_beta /
    so_lambda -- a Lomax distribution; E[y^2] = 2 s^2 / ((so_alpha - 1) (so_alpha - 2)), +inf for so_alpha <= 2.  One y is shared by the
    real and the imaginary scalar of a frequency (shared = True).
    mode 2 (the other outlier families): sigma_out = 0.05 raw, raw ~ exponential(so_lambda) per stacked row: y ~ exponential
    of scale s = 0.05 / so_lambda, E[y^2] = 2 s^2, shared = False.

    The rule is the trapezoid rule on a uniform grid in u = ln(y / s) of the given step, w_j = step y_j p(y_j) (halved at the
    two ends); in u the integrand is analytic in a strip and decays at least exponentially both ways, so the rule converges
    geometrically in 1 / step.  The grid starts at u = -36, below which lies a mass of so_alpha e^-36 (mode 2: e^-72 / 2).  It
    ends, mode 2, at u = 5 (a mass of e^-148 beyond) and, mode 1, where the mass beyond, e^(-so_alpha u), is below 1e-14 and,
    for so_alpha > 2, the part of E[y^2] beyond, so_alpha (so_alpha - 1) / 2 e^(-(so_alpha - 2) u) of it, is below 1e-11 --
    but at u = 10 at the earliest and at u = 27.5 at the latest, which keeps Q <= 512 at the default step: so_alpha >= 1.2
    meets the first and so_alpha >= 2.95 the second; a heavier tail is cut at u = 27.5 and the sums carry what that leaves
    out (E[y^2] is returned in closed form either way).  DESIGN.md 3.5h has the measured accuracy."""
    mode, lam, alpha, beta, h = int(mode), float(so_lambda), float(so_alpha), float(so_beta), float(step)
    if mode not in (1, 2):
        raise ValueError('sigma_out_table: no outlier error model (outlier_mode %d)' % mode)
    if not (lam > 0 and np.isfinite(lam)) or not (h > 0) or (mode == 1 and not (alpha > 0 and beta > 0 and np.isfinite(alpha * beta))):
        raise ValueError('sigma_out_table: the hyper-parameters and the step must be positive finite numbers')
    lo = -36.0
    if mode == 1:
        s = 0.05 * beta / lam
        hi = max(10.0, np.log(1e14) / alpha)
        if alpha > 2:
            hi = max(hi, (np.log(1e11) + np.log(alpha * (alpha - 1) / 2)) / (alpha - 2))
        hi = min(hi, 27.5)
        ey2 = 2 * s * s / ((alpha - 1) * (alpha - 2)) if alpha > 2 else np.inf
    else:
        s, hi = 0.05 / lam, 5.0
        ey2 = 2 * s * s
    u = lo + h * np.arange(int(np.ceil((hi - lo) / h)) + 1)
    t = np.exp(u)
    if mode == 1:
        w = h * np.exp((np.log(alpha) + u) - (alpha + 1) * np.log1p(t))     # y p(y) = alpha t (1 + t)^-(alpha + 1), t = y / s
    else:
        w = h * np.exp(u - t)                                               # y p(y) = t exp(-t)
    w[0] *= 0.5
    w[-1] *= 0.5
    return s * t, w, float(ey2), mode == 1


MIX_MAX_NODES = 512                              # bdrt_heldout_mix_max_nodes()


def sigma_out_prior_table(problem):
    """`sigma_out_table` of a problem's outlier error model -- (y [Q], w [Q], E[y^2], shared), Q <= 512 -- from its
    outlier_mode, so_lambda, so_alpha and so_beta alone.  Pure numpy: no GPU.  ValueError for a problem without an outlier model."""
    mode = _outlier_mode(problem)
    if mode not in (1, 2):
        raise ValueError('sigma_out_prior_table: the problem has no outlier error model')
    d = problem.dat
    y, w, ey2, shared = sigma_out_table(mode, d.so_lambda, d.so_alpha, d.so_beta)
    assert len(y) <= MIX_MAX_NODES
    return y, w, ey2, shared


def _heldout_grid(problem, freq_test, A_test_blocks, who, sigma_out=None):
    """Checks of the held-out grid that need no GPU -> (freq [H], the prediction rows packed as bdrt_heldout_transformed takes
    them).  A_test_blocks: per block of the problem (A_re, A_im), each [H, K_b], or the two stacked, [2 H, K_b].  sigma_out:
    `check_sigma_out`; None refuses an outlier error model, 'prior' a problem without one."""
    if check_sigma_out(sigma_out, who) is None:
        if _outlier_mode(problem):
            raise NotImplementedError('%s: %s' % (who, OUTLIER_REFUSAL))
    elif not _outlier_mode(problem):
        raise ValueError("%s: sigma_out='prior' needs an outlier error model; this problem has none" % who)
    freq = np.ascontiguousarray(np.asarray(freq_test, dtype=float).reshape(-1))
    H = len(freq)
    if H < 1 or not np.all(np.isfinite(freq) & (freq > 0)):
        raise ValueError('%s: freq_test must hold at least one positive finite frequency' % who)
    Ks = list(problem.Ks)
    if len(A_test_blocks) != len(Ks):
        raise ValueError('%s: %d blocks of prediction rows for a problem of %d blocks' % (who, len(A_test_blocks), len(Ks)))
    parts = []
    for b, (A, K) in enumerate(zip(A_test_blocks, Ks)):
        if isinstance(A, (tuple, list)):
            if len(A) != 2:
                raise ValueError('%s: block %d: (A_re, A_im) expected' % (who, b))
            A = np.concatenate([np.atleast_2d(np.asarray(a, dtype=float)) for a in A])
        A = np.asarray(A, dtype=float)
        if A.shape != (2 * H, K):
            raise ValueError('%s: block %d: prediction rows %s, expected (%d, %d): real rows, then imaginary rows'
                             % (who, b, A.shape, 2 * H, K))
        parts.append(A.reshape(-1))
    return freq, np.ascontiguousarray(np.concatenate(parts))


def heldout_transformed(problem, params, freq_test, A_test_blocks, sigma_out=None):
    """Z_hat and sigma_tot [B, 2 H] (real halves, then imaginary halves) of B rows of CONSTRAINED parameters -- params [B, D]
    as `Problem.transformed` returns them -- at the frequencies freq_test [H], which need not be on the problem's grid, on the
    GPU (bdrt_heldout_transformed).  A_test_blocks: the prediction rows, per block (A_re, A_im) [H, K_b] each or stacked
    [2 H, K_b].  Block flags, x_scale, induc_scale and sigma_min are the problem's.  A row's result does not depend on what
    else is in the call.  NotImplementedError for an outlier error model, unless sigma_out='prior': the second array is then the
    base scale, sigma_tot without sigma_out (bdrt_heldout_mix_transformed), which `heldout_mix_reduce` integrates over its prior;
    ValueError with 'prior' and no outlier model."""
    who = 'heldout_transformed'
    freq, A = _heldout_grid(problem, freq_test, A_test_blocks, who, sigma_out)
    params = np.atleast_2d(_lib.f64(params))
    if params.ndim != 2 or params.shape[1] != problem.D:
        raise ValueError('%s: params must be [B, %d], not %s' % (who, problem.D, params.shape))
    B, H = params.shape[0], len(freq)
    Zh, sg = np.empty((B, 2 * H)), np.empty((B, 2 * H))
    name = 'bdrt_heldout_transformed' if sigma_out is None else 'bdrt_heldout_mix_transformed'
    _lib.check(getattr(problem._lib, name)(problem.handle, _lib.ptr(params), B, _lib.ptr(freq), H, _lib.ptr(A), _lib.ptr(Zh),
                                           _lib.ptr(sg)), name)
    return Zh, sg


def _mix_table(table, who):
    """(y, w, E[y^2], shared) of `sigma_out_prior_table`, checked without a GPU -> contiguous arrays and plain numbers"""
    try:
        y, w, ey2, shared = table
    except (TypeError, ValueError):
        raise ValueError('%s: the table must be (y [Q], w [Q], E[y^2], shared)' % who) from None
    y, w, ey2 = _lib.f64(y).reshape(-1), _lib.f64(w).reshape(-1), float(ey2)
    if len(y) < 1 or len(y) != len(w) or not np.all(np.isfinite(y) & (y >= 0) & np.isfinite(w) & (w >= 0)) or not ey2 >= 0:
        raise ValueError('%s: the table needs Q >= 1 nodes y >= 0 with weights w >= 0 and E[y^2] >= 0' % who)
    if len(y) > MIX_MAX_NODES:
        raise ValueError('%s: a table of %d nodes, the kernel holds at most %d' % (who, len(y), MIX_MAX_NODES))
    return y, w, ey2, int(bool(shared))


def _heldout_reduce(who, symbol, Zhat, sig, z, unit, *extra):
    """The body of `heldout_reduce` and `heldout_mix_reduce`: `symbol` takes the arrays, their sizes, `extra`, then the outputs."""
    pair, Zhat, sig, z, one = _stacked(who, Zhat, sig, z, unit)
    G, S, N2 = Zhat.shape
    if G < 1 or N2 < 1:
        raise ValueError('%s: empty input' % who)
    _draw_count(S, who, max_draws)
    lib = _lib.require_gpu()
    lpd = np.empty((G, N2 // 2 if pair else N2))
    outs = [np.empty((G, N2)) for _ in HELDOUT_FIELDS]
    _lib.check(getattr(lib, symbol)(_lib.ptr(Zhat), _lib.ptr(sig), _lib.ptr(z), G, S, N2, pair, *extra, _lib.ptr(lpd),
                                    *[_lib.ptr(o) for o in outs]), symbol)
    res = dict(zip(HELDOUT_FIELDS, outs), lpd=lpd)
    return {key: v[0] for key, v in res.items()} if one else res


def heldout_mix_reduce(Zhat, sig_base, z, table, unit='frequency'):
    """`heldout_reduce` under an outlier error model, on the GPU (bdrt_heldout_mix_reduce): sig_base is sigma_tot without
    sigma_out (`heldout_transformed(..., sigma_out='prior')`) and table = (y, w, E[y^2], shared) its prior as an integration rule
    (`sigma_out_prior_table`).  Per draw the density of a scalar is sum_j w_j N(z | Zhat, sig_base^2 + y_j^2); a frequency takes
    the product of its two normals under one sum (shared) or the product of the two sums; lpd is the log of the draws' mean
    density, mean is `heldout_reduce`'s, sd^2 gains E[y^2], pit is the mean of sum_j w_j Phi.  Definitions:
    tests/heldout_mix_numpy.py.  Same shapes and NaN rule as `heldout_reduce`."""
    y, w, ey2, shared = _mix_table(table, 'heldout_mix_reduce')
    return _heldout_reduce('heldout_mix_reduce', 'bdrt_heldout_mix_reduce', Zhat, sig_base, z, unit, shared, _lib.ptr(y), _lib.ptr(w),
                           len(y), ey2)


def heldout_reduce(Zhat, sig, z, unit='frequency'):
    """The predictive of held-out units under equal weights on the GPU (bdrt_heldout_reduce): Zhat, sig [G, S, N2] and z [G, N2]
    (or [S, N2] and [N2]: G = 1).  Returns a dict of lpd [G, units] = logsumexp_s(ll_s) - log S and mean, sd, pit [G, N2] of the
    mixture of the draws' normals -- `psis_loo`'s lpd and `psis_predict`'s mean_post, sd_post, pit_post to the bit, without the
    Pareto fit.  A unit with a non-finite log-likelihood gives NaN, that unit only."""
    return _heldout_reduce('heldout_reduce', 'bdrt_heldout_reduce', Zhat, sig, z, unit)


def _heldout_part(unit, part, H, who):
    """(pair, first column, columns) of the part in the 2 H held-out columns; the checks of `check_device_args`."""
    pair, _ = check_device_args(unit, part, None, who)
    return (pair,) + part_columns(part, H)


def sampler_heldout(sampler, unit_lo, unit_hi, chains, freq_test, A_test_blocks, z_test, unit='frequency', part='both',
                    chunk_bytes=None, sigma_out=None):
    """`heldout_reduce(heldout_transformed(...))` of the draws a sampler holds in HBM (bdrt_sampler_heldout): units
    [unit_lo, unit_hi) in groups of `chains` consecutive units that sampled one spectrum, against z_test [G, 2 H] (or [2 H] for
    one group), the held-out data on each group's scale.  Per chunk of groups the batch evaluator gives the constrained
    parameters of the rows, and nothing but the per-unit results comes back.  part: 'both', or 'real' / 'imag' for that half
    of the scalars (units are points then).  Returns `heldout_reduce`'s dict, lpd [G, units], the others [G, columns of the
    part]; every entry equals `host_heldout` on the downloaded draws bit for bit.  sigma_out='prior': the same for an outlier
    error model, with `heldout_mix_reduce` on the problem's `sigma_out_prior_table` (bdrt_sampler_heldout_mix)."""
    who = 'heldout'
    freq, A = _heldout_grid(sampler.problem, freq_test, A_test_blocks, who, sigma_out)
    H = len(freq)
    pair, col0, ncols = _heldout_part(unit, part, H, who)
    unit_lo, unit_hi, chains, G = _unit_groups(sampler, unit_lo, unit_hi, chains, who)
    z = np.atleast_2d(_lib.f64(z_test))
    if z.shape != (G, 2 * H):
        raise ValueError('%s: z_test must be [%d, %d] (real halves, then imaginary halves), not %s' % (who, G, 2 * H, z.shape))
    chunk = chunk_or_default(chunk_bytes)
    _sampler_draw_count(sampler, chains, who, max_draws)
    lpd = np.empty((G, ncols // 2 if pair else ncols))
    outs = [np.empty((G, ncols)) for _ in HELDOUT_FIELDS]
    front = (sampler.handle, unit_lo, unit_hi, chains, pair, col0, ncols, chunk, _lib.ptr(freq), H, _lib.ptr(A), _lib.ptr(z))
    if sigma_out is None:
        _lib.check(sampler._lib.bdrt_sampler_heldout(*front, _lib.ptr(lpd), *[_lib.ptr(o) for o in outs]), 'bdrt_sampler_heldout')
    else:
        y, w, ey2, shared = _mix_table(sigma_out_prior_table(sampler.problem), who)
        _lib.check(sampler._lib.bdrt_sampler_heldout_mix(*front, shared, _lib.ptr(y), _lib.ptr(w), len(y), ey2, _lib.ptr(lpd),
                                                         *[_lib.ptr(o) for o in outs]), 'bdrt_sampler_heldout_mix')
    return dict(zip(HELDOUT_FIELDS, outs), lpd=lpd)


def host_heldout(problem, draws, chains, freq_test, A_test_blocks, z_test, unit='frequency', part='both', sigma_out=None):
    """What `sampler_heldout` computes, on host-resident unconstrained draws [G, chains * n_draws, D] through the host-staged
    entry points (`Problem.transformed` for the constrained parameters, `heldout_transformed`, `heldout_reduce`): the yardstick
    of the device path.  sigma_out='prior': through `heldout_transformed(..., sigma_out='prior')` and `heldout_mix_reduce`."""
    who = 'heldout'
    freq, _ = _heldout_grid(problem, freq_test, A_test_blocks, who, sigma_out)
    H = len(freq)
    _, col0, ncols = _heldout_part(unit, part, H, who)
    draws, z = np.asarray(draws, dtype=float), np.atleast_2d(np.asarray(z_test, dtype=float))
    if draws.ndim != 3 or draws.shape[2] != problem.D or z.shape != (draws.shape[0], 2 * H):
        raise ValueError('%s: draws must be [G, S, %d] and z_test [G, %d]' % (who, problem.D, 2 * H))
    _draw_count(draws.shape[1], who, max_draws)
    cols = slice(col0, col0 + ncols)
    tr = [heldout_transformed(problem, problem.transformed(d)[0], freq, A_test_blocks, sigma_out) for d in draws]
    arrays = (np.ascontiguousarray(np.stack([t[0] for t in tr])[:, :, cols]),
              np.ascontiguousarray(np.stack([t[1] for t in tr])[:, :, cols]), np.ascontiguousarray(z[:, cols]))
    if sigma_out is None:
        return heldout_reduce(*arrays, unit)
    return heldout_mix_reduce(*arrays, sigma_out_prior_table(problem), unit)


def _host_arrays(problem, draws, z, part):
    """Z_hat, sigma_tot [G, S, columns] and z [G, columns] of host-resident unconstrained draws [G, S, D]: `transformed` per
    group, as `StanFit['Z_hat']` calls it, then the columns of the part."""
    draws, z = np.asarray(draws, dtype=float), np.atleast_2d(np.asarray(z, dtype=float))
    if draws.ndim != 3 or z.shape[0] != draws.shape[0]:
        raise ValueError('draws must be [G, S, D] and z [G, 2 Nf]')
    col0, ncols = part_columns(part, z.shape[1] // 2)
    cols = slice(col0, col0 + ncols)
    tr = [problem.transformed(d)[1:] for d in draws]
    return (np.ascontiguousarray(np.stack([t[0] for t in tr])[:, :, cols]),
            np.ascontiguousarray(np.stack([t[1] for t in tr])[:, :, cols]), np.ascontiguousarray(z[:, cols]))


def host_psis_loo(problem, draws, z, chains, unit='frequency', part='both', reff='auto'):
    """What `sampler_psis_loo` computes, on host-resident draws [G, chains * n_draws, D] against z [G, 2 Nf] through the host-
    staged entry points (`Problem.transformed`, `pointwise_log_lik`, `psis_loo`): the yardstick of the device path, and what
    `parallel.sample_sharded` runs when the chains of a spectrum are spread over ranks.  reff='auto' is
    `relative_efficiency`."""
    check_device_args(unit, part, reff, 'psis_loo')
    Zh, sg, zz = _host_arrays(problem, draws, z, part)
    ll = pointwise_log_lik(Zh, sg, zz, unit)
    r = np.broadcast_to(np.asarray(1.0 if reff is None else _reff_arg(reff, ll, int(chains)), dtype=float), ll[:, 0].shape)
    return dict(psis_loo(ll, r), reff=np.array(r))


def host_psis_predict(problem, draws, z, chains, unit='frequency', part='both', reff='auto'):
    """The same for `sampler_psis_predict` (`psis_predict`)."""
    pair, _ = check_device_args(unit, part, reff, 'psis_predict')
    Zh, sg, zz = _host_arrays(problem, draws, z, part)
    U = zz.shape[1] // 2 if pair else zz.shape[1]
    r = np.broadcast_to(np.asarray(1.0 if reff is None else _predict_reff(reff, Zh, sg, zz, pair, int(chains)), dtype=float),
                        (len(zz), U))
    return dict(psis_predict(Zh, sg, zz, unit, r), reff=np.array(r))


def relative_efficiency(ll, chains):
    """MCMC relative efficiency of the likelihood draws, n_eff(exp(ll - max ll)) / S per column (`column_diagnostics`), for the
    tail length of PSIS.  ll [S, N] or [G, S, N]; a column without a finite n_eff (constant, or too few draws) gets 1."""
    from .diagnostics import column_diagnostics
    ll = np.asarray(ll, dtype=float)
    S = ll.shape[-2]
    with np.errstate(invalid='ignore', over='ignore'):
        lik = np.exp(ll - ll.max(axis=-2, keepdims=True))
    n_eff = column_diagnostics(lik, chains)[2]
    r = n_eff / S
    return np.where(np.isfinite(r) & (r > 0), r, 1.0)


# ---------------------------------------------------------------------------------------------------- fits
def _fit_arrays(fit, z, columns):
    Zhat, sig = np.asarray(fit['Z_hat'], dtype=float), np.asarray(fit['sigma_tot'], dtype=float)
    z = np.asarray(z, dtype=float).reshape(-1)
    if Zhat.ndim != 2 or sig.shape != Zhat.shape or z.shape[0] != Zhat.shape[1]:
        raise ValueError('loo: Z_hat %s, sigma_tot %s and the data %s do not fit' % (Zhat.shape, sig.shape, z.shape))
    if columns is not None:
        Zhat, sig, z = Zhat[:, columns], sig[:, columns], z[columns]
    return np.ascontiguousarray(Zhat), np.ascontiguousarray(sig), np.ascontiguousarray(z)


def _reff_arg(reff, ll, chains):
    if isinstance(reff, str):
        if reff != 'auto':
            raise ValueError("reff must be 'auto', None, a number or an array")
        return relative_efficiency(ll, chains)
    return reff


def _result(p, n_scalar_per_unit, S, log_scale, frequencies=None, prefix=''):
    """Pointwise kernel outputs of one fit -> LooResult; logs the k-hat line."""
    shift = n_scalar_per_unit * float(log_scale)
    n = len(p['lpd'])
    elpd_i, lpd_i = p['elpd_loo'] - shift, p['lpd'] - shift
    waic_i = lpd_i - p['p_waic']
    with np.errstate(invalid='ignore'):
        bad = np.nonzero(p['pareto_k'] > K_THRESHOLD)[0]
    res = LooResult(
        elpd_loo=float(np.sum(p['elpd_loo']) - n * n_scalar_per_unit * float(log_scale)),
        se=float(np.sqrt(n * np.var(elpd_i))), p_loo=float(np.sum(p['p_loo'])),
        elpd_waic=float(np.sum(p['elpd_waic']) - n * n_scalar_per_unit * float(log_scale)),
        p_waic=float(np.sum(p['p_waic'])), se_waic=float(np.sqrt(n * np.var(waic_i))),
        n_units=n, n_draws=int(S), elpd_i=elpd_i, lpd_i=lpd_i, pareto_k=p['pareto_k'], p_waic_i=p['p_waic'],
        n_tail=p['n_tail'], n_bad_k=int(len(bad)))
    if len(bad):
        where = ''
        if frequencies is not None and len(frequencies) in (n, n // 2) and len(frequencies):
            where = ', f = %s Hz' % np.array2string(np.asarray(frequencies, dtype=float)[bad % len(frequencies)], precision=4)
        logger.warning('%s%d of %d observations have Pareto k > %.1f (indices %s%s): their LOO estimates are unreliable and the '
                       'posterior hinges on them', prefix, len(bad), n, K_THRESHOLD, bad.tolist(), where)
    else:
        logger.info('%sAll Pareto k estimates are below %.1f (largest %.3g)', prefix, K_THRESHOLD,
                    float(np.nanmax(p['pareto_k'][np.isfinite(p['pareto_k'])], initial=-np.inf)))
    return res


def loo(fit, z, chains=None, unit='frequency', reff='auto', log_scale=0.0, columns=None, frequencies=None):
    """PSIS-LOO and WAIC of a sampling fit (`StanFit` or `SavedFit`) against the data z [2 Nf] it was fitted to (the Stan data
    entry 'Z': real parts, then imaginary parts, on the fit's scale).

    chains: chains of the fit (default fit.chains), for reff='auto'.  reff: 'auto' (`relative_efficiency`), None (1), a
    number or one per observation.  log_scale: subtracted once per scalar observation -- with log(Z scale) the result is a
    log density of the impedance as supplied, comparable between fits scaled differently.  columns: the scalar observations
    that count (a slice or index array into the 2 Nf; then every one of them is a unit of its own).
    Returns a `LooResult`: elpd_loo, se, p_loo, elpd_waic, p_waic, se_waic, n_units, n_draws, the pointwise arrays elpd_i,
    lpd_i, pareto_k, p_waic_i, n_tail, and n_bad_k, the number of observations with k > 0.7."""
    pair = _pair(unit) if columns is None else 0
    Zhat, sig, z = _fit_arrays(fit, z, columns)
    ll = pointwise_log_lik(Zhat, sig, z, 'frequency' if pair else 'point')
    chains = int(chains if chains is not None else getattr(fit, 'chains', 1))
    p = psis_loo(ll, _reff_arg(reff, ll, chains))
    return _result(p, 2 if pair else 1, ll.shape[0], log_scale, frequencies)


def loo_many(fits, zs, chains=None, unit='frequency', reff='auto', log_scales=None, columns=None, frequencies=None,
             chunk_bytes=CHUNK_BYTES):
    """`loo` of many fits: fits with equal (draws, observations) go through one launch of each kernel per chunk, a chunk being
    as many fits as keep its stacked host arrays (Z_hat, sigma_tot, ll) below `chunk_bytes`.  Results in input order, each
    equal to the single-fit `loo` bit for bit (a column's result does not depend on what else is in the launch)."""
    n = len(fits)
    log_scales = [0.0] * n if log_scales is None else list(log_scales)
    frequencies = [None] * n if frequencies is None else list(frequencies)
    pair = _pair(unit) if columns is None else 0
    arrays = [_fit_arrays(f, z, columns) for f, z in zip(fits, zs)]
    ch = [int(chains if chains is not None else getattr(f, 'chains', 1)) for f in fits]
    groups = {}
    for i, a in enumerate(arrays):
        groups.setdefault((a[0].shape, ch[i]), []).append(i)
    out = [None] * n
    for (shape, m), idx in groups.items():
        per_fit = 3 * shape[0] * shape[1] * 8
        step = max(1, int(chunk_bytes // per_fit))
        for k0 in range(0, len(idx), step):
            sel = idx[k0:k0 + step]
            Zh, sg, zz = [np.stack([arrays[i][j] for i in sel]) for j in range(3)]
            ll = pointwise_log_lik(Zh, sg, zz, 'frequency' if pair else 'point')
            r = _reff_arg(reff, ll, m)
            if r is not None and np.ndim(r) == 1:
                r = np.broadcast_to(r, (ll.shape[2],))[None].repeat(len(sel), 0)
            p = psis_loo(ll, r)
            for g, i in enumerate(sel):
                out[i] = _result({k: v[g] for k, v in p.items()}, 2 if pair else 1, shape[0], log_scales[i], frequencies[i],
                                 'fit %d: ' % i)
    return out


def ks_uniform(p):
    """Kolmogorov-Smirnov distance of the finite values of p from U(0, 1) and its asymptotic p-value, the Kolmogorov series
    2 sum_{j >= 1} (-1)^(j - 1) exp(-2 j^2 n D^2).  (nan, nan) without a finite value."""
    p = np.asarray(p, dtype=float).reshape(-1)
    p = np.sort(p[np.isfinite(p)])
    n = len(p)
    if n == 0:
        return float('nan'), float('nan')
    i = np.arange(1, n + 1)
    D = float(max(np.max(i / n - p), np.max(p - (i - 1) / n)))
    t = n * D * D
    j = np.arange(1, 101)                            # t > 0.04: the terms beyond j = 23 are below 1e-18; below it 1 - Q < 1e-10
    q = 2.0 * float(np.sum((-1.0) ** (j - 1) * np.exp(-2.0 * j * j * t))) if t > 0.04 else 1.0
    return D, min(max(q, 0.0), 1.0)


def _predict_result(p, z, S, frequencies=None, prefix=''):
    """Kernel outputs of one fit -> LooPredictResult; logs the k-hat and residual line."""
    with np.errstate(invalid='ignore', divide='ignore'):
        resid, resid_post = (z - p['mean']) / p['sd'], (z - p['mean_post']) / p['sd_post']
        bad = np.nonzero(p['pareto_k'] > K_THRESHOLD)[0]
    ks, ks_p = ks_uniform(p['pit'])
    res = LooPredictResult(resid=resid, resid_post=resid_post, n_bad_k=int(len(bad)), n_draws=int(S), pit_ks=ks, pit_ks_p=ks_p,
                           **{k: p[k] for k in PREDICT_FIELDS + ('pareto_k', 'n_tail')})
    fin = np.abs(resid[np.isfinite(resid)])
    worst = int(np.nanargmax(np.abs(resid))) if len(fin) else -1
    where = ''
    if worst >= 0 and frequencies is not None and len(frequencies):
        where = ' (f = %.4g Hz)' % float(np.asarray(frequencies, dtype=float)[worst % len(frequencies)])
    logger.log(logging.WARNING if len(bad) else logging.INFO,
               '%sLOO predictive check: %d of %d units have Pareto k > %.1f; largest |LOO residual| %.3g at observation %d%s; '
               'LOO-PIT KS distance %.3g (p = %.3g)', prefix, len(bad), len(p['pareto_k']), K_THRESHOLD,
               float(fin.max()) if len(fin) else float('nan'), worst, where, ks, ks_p)
    return res


def _predict_reff(reff, Zh, sg, zz, pair, chains):
    if isinstance(reff, str):
        if reff != 'auto':
            raise ValueError("reff must be 'auto', None, a number or an array")
        return relative_efficiency(pointwise_log_lik(Zh, sg, zz, 'frequency' if pair else 'point'), chains)
    return reff


def loo_predict(fit, z, chains=None, unit='frequency', reff='auto', columns=None, frequencies=None):
    """LOO predictive check of a sampling fit (`StanFit` or `SavedFit`) against the data z [2 Nf] it was fitted to, on the
    fit's scale; arguments as `loo`.  Returns a `LooPredictResult`: per scalar observation mean, sd and pit of its
    leave-one-out predictive distribution, resid = (z - mean) / sd, and mean_post, sd_post, pit_post, resid_post of the
    in-sample posterior predictive; per unit pareto_k and n_tail; n_bad_k (units with k > 0.7, whose LOO figures are
    unreliable), n_draws, and pit_ks, pit_ks_p: the Kolmogorov-Smirnov distance of the finite LOO-PIT values from U(0, 1) and
    its asymptotic p-value."""
    pair = _pair(unit) if columns is None else 0
    Zhat, sig, z = _fit_arrays(fit, z, columns)
    chains = int(chains if chains is not None else getattr(fit, 'chains', 1))
    p = psis_predict(Zhat, sig, z, 'frequency' if pair else 'point', _predict_reff(reff, Zhat, sig, z, pair, chains))
    return _predict_result(p, z, Zhat.shape[0], frequencies)


def loo_predict_many(fits, zs, chains=None, unit='frequency', reff='auto', columns=None, frequencies=None,
                     chunk_bytes=CHUNK_BYTES):
    """`loo_predict` of many fits, grouped and chunked as `loo_many`: results in input order, each equal to the single-fit
    `loo_predict` bit for bit."""
    n = len(fits)
    frequencies = [None] * n if frequencies is None else list(frequencies)
    pair = _pair(unit) if columns is None else 0
    arrays = [_fit_arrays(f, z, columns) for f, z in zip(fits, zs)]
    ch = [int(chains if chains is not None else getattr(f, 'chains', 1)) for f in fits]
    groups = {}
    for i, a in enumerate(arrays):
        groups.setdefault((a[0].shape, ch[i]), []).append(i)
    out = [None] * n
    for (shape, m), idx in groups.items():
        per_fit = 3 * shape[0] * shape[1] * 8
        step = max(1, int(chunk_bytes // per_fit))
        for k0 in range(0, len(idx), step):
            sel = idx[k0:k0 + step]
            Zh, sg, zz = [np.stack([arrays[i][j] for i in sel]) for j in range(3)]
            r = _predict_reff(reff, Zh, sg, zz, pair, m)
            if r is not None and np.ndim(r) == 1:
                r = np.broadcast_to(r, (shape[1] // 2 if pair else shape[1],))[None].repeat(len(sel), 0)
            p = psis_predict(Zh, sg, zz, 'frequency' if pair else 'point', r)
            for g, i in enumerate(sel):
                out[i] = _predict_result({k: v[g] for k, v in p.items()}, zz[g], shape[0], frequencies[i], 'fit %d: ' % i)
    return out

# ---------------------------------------------------------------------------------------------------- K-fold and exact refits
def heldout_result(p, z, frequencies, part, unit, S, z_scale, sigma_out=None):
    """One group's row of `heldout_reduce`'s dict (lpd [units], mean, sd, pit [columns of the part]) against the scaled held-out
    data z [columns of the part] -> LooResult in the units of the impedance as supplied: frequencies, elpd (the sum), elpd_i per
    unit (log(z_scale) subtracted once per scalar), Z_pred (complex), sigma_pred_re/_im, pit_re/_im, resid_re/_im, n_draws.
    part 'real' / 'imag': the other half is NaN and units are points.  sigma_out='prior' (p from `heldout_mix_reduce`) is
    recorded under that key; None adds no key."""
    pair, _ = check_device_args(unit, part, None, 'heldout')
    check_sigma_out(sigma_out, 'heldout_result')
    freq = np.array(frequencies, dtype=float).reshape(-1)
    H, sc = len(freq), float(z_scale)
    half = {'real': ('re',), 'imag': ('im',), 'both': ('re', 'im')}[part]
    z, lpd = np.asarray(z, dtype=float).reshape(-1), np.asarray(p['lpd'], dtype=float).reshape(-1)
    if len(z) != H * len(half) or len(lpd) != (H if pair else len(z)) or any(np.shape(p[k]) != z.shape for k in HELDOUT_FIELDS):
        raise ValueError('heldout_result: the arrays do not fit %d frequencies, part %r, unit %r' % (H, part, unit))
    nan = np.full(H, np.nan)

    def parts(v):
        v = np.asarray(v, dtype=float)
        return {'re': v[:H] if 're' in half else nan, 'im': v[H * (len(half) - 1):] if 'im' in half else nan}
    with np.errstate(invalid='ignore', divide='ignore'):
        resid = (z - p['mean']) / p['sd']
    elpd_i = lpd - (2 if pair else 1) * float(np.log(sc))
    m, sd, pit, rs = parts(p['mean']), parts(p['sd']), parts(p['pit']), parts(resid)
    out = LooResult(frequencies=freq, elpd=float(np.sum(elpd_i)), elpd_i=elpd_i, n_draws=int(S), unit=unit, part=part)
    out['Z_pred'] = np.empty(H, dtype=complex)                              # (a NaN half must not spread to the other)
    out['Z_pred'].real, out['Z_pred'].imag = m['re'] * sc, m['im'] * sc
    for h in ('re', 'im'):
        out['sigma_pred_' + h], out['pit_' + h], out['resid_' + h] = sd[h] * sc, pit[h], rs[h]
    if sigma_out is not None:
        out['sigma_out'] = sigma_out
    return out


def fold_labels(frequencies, folds=10):
    """The fold of every frequency, in the order given, without random numbers: with an integer `folds` the frequencies are
    sorted in descending order and sorted index i goes to fold i % folds, so every fold spans the whole range; or `folds` is an
    integer array with one label per frequency.  ValueError for fewer than two folds, for a fold that would be empty or leave no
    training data, and for a label array of the wrong length."""
    f = np.asarray(frequencies, dtype=float).reshape(-1)
    n = len(f)
    if np.ndim(folds) == 0:
        k = int(folds)
        if k != folds or k < 2:
            raise ValueError('kfold: folds must be an integer of at least 2 or an array of fold labels, not %r' % (folds,))
        if k > n:
            raise ValueError('kfold: %d folds for %d frequencies: a fold would be empty' % (k, n))
        labels = np.empty(n, dtype=int)
        labels[np.argsort(-f, kind='stable')] = np.arange(n) % k
        return labels
    lab = np.asarray(folds)
    if lab.ndim != 1 or len(lab) != n:
        raise ValueError('kfold: %d fold labels for %d frequencies' % (lab.size, n))
    if not np.issubdtype(lab.dtype, np.integer):
        if not np.all(np.isfinite(lab.astype(float))) or np.any(lab.astype(float) != np.round(lab.astype(float))):
            raise ValueError('kfold: fold labels must be integers')
    lab = lab.astype(int)
    if len(np.unique(lab)) < 2:
        raise ValueError('kfold: at least 2 folds are needed: one fold alone leaves no training data')
    return lab


def kfold_result(labels, fold_results, unit='frequency', part='both'):
    """The `heldout_result`s of the folds of ONE spectrum -> its K-fold LooResult, in the order of the supplied grid.
    labels [n]: `fold_labels`; fold_results {label: heldout_result of the frequencies with that label, in grid order}.
    Carries what `compare` reads -- elpd_loo (the sum of the folds' elpd_i), se, elpd_i, n_units; p_loo NaN, pareto_k all NaN,
    n_bad_k 0 --, method='kfold', the `fold` of every unit and the predictive arrays of `heldout_result`; and `sigma_out` when
    the folds carry it (all of them, or none)."""
    pair, _ = check_device_args(unit, part, None, 'kfold')
    labels = np.asarray(labels, dtype=int)
    n = len(labels)
    both_points = part == 'both' and not pair
    n_units = 2 * n if both_points else n
    elpd_i = np.full(n_units, np.nan)
    filled = np.zeros(n, dtype=int)
    arrays = {k: np.full(n, np.nan, dtype=complex if k == 'Z_pred' else float)
              for k in ('Z_pred', 'sigma_pred_re', 'sigma_pred_im', 'pit_re', 'pit_im', 'resid_re', 'resid_im')}
    freq = np.full(n, np.nan)
    n_draws = None
    if set(fold_results) != set(np.unique(labels).tolist()):
        raise ValueError('kfold_result: folds %s, labels %s' % (sorted(fold_results), np.unique(labels).tolist()))
    for lab, r in fold_results.items():
        idx = np.nonzero(labels == lab)[0]
        e = np.asarray(r['elpd_i'])
        if len(e) != (2 * len(idx) if both_points else len(idx)):
            raise ValueError('kfold_result: fold %r has %d units for %d frequencies' % (lab, len(e), len(idx)))
        filled[idx] += 1
        if both_points:
            elpd_i[idx], elpd_i[n + idx] = e[:len(idx)], e[len(idx):]
        else:
            elpd_i[idx] = e
        for k in arrays:
            arrays[k][idx] = r[k]
        freq[idx] = r['frequencies']
        n_draws = int(r['n_draws']) if n_draws is None else min(n_draws, int(r['n_draws']))
    if not np.all(filled == 1):
        raise ValueError('kfold_result: every frequency must be held out exactly once')
    modes = {r.get('sigma_out') for r in fold_results.values()}
    if len(modes) > 1:
        raise ValueError('kfold_result: the folds differ in sigma_out (%s)' % sorted(map(repr, modes)))
    if modes != {None}:
        arrays = dict(arrays, sigma_out=modes.pop())
    return LooResult(elpd_loo=float(np.sum(elpd_i)), se=float(np.sqrt(n_units * np.var(elpd_i))), p_loo=float('nan'),
                     n_units=int(n_units), n_draws=n_draws, elpd_i=elpd_i, pareto_k=np.full(n_units, np.nan), n_bad_k=0,
                     method='kfold', fold=np.concatenate([labels, labels]) if both_points else labels.copy(), frequencies=freq,
                     unit=unit, part=part, **arrays)


def reloo_candidates(loo_result, k_threshold=K_THRESHOLD, max_refits=8):
    """Indices of the units of a `LooResult` whose Pareto k exceeds k_threshold: those an exact refit repairs.  ValueError when
    there are more than max_refits (None: no cap)."""
    with np.errstate(invalid='ignore'):
        cand = np.nonzero(np.asarray(loo_result['pareto_k'], dtype=float) > k_threshold)[0]
    if max_refits is not None and len(cand) > int(max_refits):
        raise ValueError('reloo: %d observations have Pareto k > %g, more than max_refits = %d exact refits: raise max_refits '
                         '(None lifts the cap), or use kfold, the cheaper route when so many are flagged'
                         % (len(cand), k_threshold, int(max_refits)))
    return cand


def reloo_result(loo_result, exact):
    """`LooResult` of `loo` with elpd_i replaced by exact values at refit units: exact {unit index: elpd_i of a fit without that
    unit}.  elpd_loo, se, p_loo (the sum of lpd_i - elpd_i) and n_bad_k (units still above 0.7 and not refit) are recomputed;
    lpd_i, pareto_k, the WAIC entries and every other elpd_i keep their bits.  Adds the boolean `refit` [n_units] and
    method='psis+refit'."""
    res = LooResult(loo_result)
    elpd_i = np.array(loo_result['elpd_i'], dtype=float)
    n = len(elpd_i)
    refit = np.zeros(n, dtype=bool)
    for i, v in exact.items():
        if not 0 <= int(i) < n:
            raise ValueError('reloo_result: unit %r of %d' % (i, n))
        elpd_i[int(i)] = float(v)
        refit[int(i)] = True
    with np.errstate(invalid='ignore'):
        bad = (np.asarray(loo_result['pareto_k'], dtype=float) > K_THRESHOLD) & ~refit
    res.update(elpd_i=elpd_i, elpd_loo=float(np.sum(elpd_i)), se=float(np.sqrt(n * np.var(elpd_i))),
               p_loo=float(np.sum(np.asarray(loo_result['lpd_i'], dtype=float) - elpd_i)), n_bad_k=int(np.sum(bad)), refit=refit,
               method='psis+refit')
    return res


def compare(results):
    """Rank fits of ONE data set: {name: LooResult} -> list of rows (dicts: name, elpd_loo, se, elpd_diff, dse, p_loo, n_bad_k),
    best first.  elpd_diff is the difference to the best fit and dse the standard error of the pointwise differences,
    sqrt(n var(elpd_i - elpd_i of the best)).  Raises ValueError when the results do not cover the same number of units."""
    if not results:
        return []
    names = list(results)
    n = {int(results[k]['n_units']) for k in names}
    if len(n) != 1:
        raise ValueError('compare: the results cover different numbers of observations (%s): not fits of one data set with '
                         'one unit' % sorted(n))
    n = n.pop()
    order = sorted(names, key=lambda k: -float(results[k]['elpd_loo']))
    best = results[order[0]]
    rows = []
    for k in order:
        r = results[k]
        d = np.asarray(r['elpd_i']) - np.asarray(best['elpd_i'])
        rows.append({'name': k, 'elpd_loo': float(r['elpd_loo']), 'se': float(r['se']),
                     'elpd_diff': float(r['elpd_loo']) - float(best['elpd_loo']), 'dse': float(np.sqrt(n * np.var(d))),
                     'p_loo': float(r['p_loo']), 'n_bad_k': int(r['n_bad_k'])})
    return rows
