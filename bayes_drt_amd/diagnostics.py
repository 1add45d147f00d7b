"""HMC diagnostics of a sampling fit: pystan's `summary`, `stansummary`, `check_hmc_diagnostics`, and the rank-normalised
`rank_diagnostics`, `sampler_rank_diagnostics`, `rank_summary`.

The reference's users read these after every `fit(mode='sample')`: pystan 2.19's `sampling()` checked every run itself and
logged the result (`WARNING:pystan:Rhat above 1.1 ...`), and its `fit.summary()` reported n_eff and Rhat.  Here the reductions
run on the GPU (bdrt_diag.hip: `bdrt_diagnostics` on host draws, `bdrt_sampler_diagnostics` on a sampler's device draws);
the definitions are Stan 2.19's, written out in tests/diag_numpy.py.  Messages go to logging.getLogger('bayes_drt_amd').

Columns: every flat element of the model's `parameters`, `transformed parameters` and `generated quantities`, on the
constrained scale, in declaration order, then lp__ -- as far as the fit can provide them.  A live fit of the Series and
Parallel families provides all of them; a Series-Parallel / Series-2Parallel fit leaves out the intermediate transformed
parameters of its parallel blocks (Y_hat*, Z_hat_p*, x_sum*) and its generated quantities; a fit restored from a file
(`SavedFit`) has the arrays it stored, plus Z_hat_re / Z_hat_im / dups, which follow from them (not q: that needs the
differentiation matrices).

Rank-normalised diagnostics (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; bdrt_rank.hip, definitions written out in
tests/rank_numpy.py): `rank_diagnostics` on host draws, `sampler_rank_diagnostics` / `Sampler.rank_diagnostics` on a sampler's
device draws, `rank_summary` (also `StanFit.rank_summary`, `SavedFit.rank_summary`) for the columns of a fit, and the checks
'rank_Rhat', 'ess_bulk', 'ess_tail' (`RANK_CHECKS`) of `check_hmc_diagnostics`, which run only when asked for: the automatic
check after `fit` / `fit_many` is pystan's, unchanged.  The convention (everything on split chains) is that of Stan's
`posterior` package and of arviz; neither was available to compare against, so no bit-parity with them is claimed.

Comparing fits (PSIS-LOO, WAIC, the Pareto k-hat of every observation) is in bayes_drt_amd.loo; its relative efficiency
comes from `column_diagnostics` here.

Out of scope: pystan's E-BFMI check ('energy').  It needs the Hamiltonian of every draw, and no sampler kernel records it;
`checks=['energy']` raises NotImplementedError.  Of the rank-normalised family: the MCSE of sd and of quantiles, rank plots,
and making these checks the default of `fit` / `fit_many` (`parallel.sample_sharded(..., rank_diagnostics=True)` reduces them
per rank on the sampler's device draws).
"""
import ctypes as C
import logging

import numpy as np

from . import _lib

logger = logging.getLogger('bayes_drt_amd')

MAX_FLAT = 1000                                  # pystan's sampling(): above this many flat names, n_eff / Rhat are skipped
DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
CHECKS = ('n_eff', 'Rhat', 'divergence', 'treedepth')
RANK_CHECKS = ('rank_Rhat', 'ess_bulk', 'ess_tail')    # on request only: check_hmc_diagnostics(fit, checks=[...])
RANK_PROBS = (0.05, 0.5, 0.95)
TAIL_PROBS = (0.05, 0.95)
RANK_RHAT_MAX = 1.01                             # thresholds of Vehtari et al. 2021
ESS_PER_CHAIN_MIN = 100.0


# ---------------------------------------------------------------------------------------------------- declarations
def _family(model_name):
    base = model_name.replace('_StanModel.pkl', '')
    return base.split('_')[0], base.endswith('_outliers')


def declared_columns(model_name, N, N_tilde, Ks):
    """[(name, size, block)] of the model text's parameters, transformed parameters and generated quantities, in declaration
    order (reference bayes_drt/stan_model_files/<model>_modelcode.txt).  N: the data size N of the Stan data (2 Nf; Nf for the
    Series outlier models), N_tilde: prediction size, Ks: basis sizes per block (series block first)."""
    fam, outl = _family(model_name)
    P, T, G = 'parameters', 'transformed parameters', 'generated quantities'
    err = ['sigma_res', 'alpha_prop', 'alpha_re', 'alpha_im']
    d = []
    if fam in ('Series', 'Parallel'):
        K = Ks[0]
        Nz = 2 * N if (fam == 'Series' and outl) else N                 # the Series outlier models take N = Nf
        d += [('Rinf_raw', 1, P), ('induc_raw', 1, P), ('x', K, P)] + [(e + '_raw', 1, P) for e in err]
        if outl:
            d += [('sigma_out_raw', N, P)] + ([('sigma_out_scale', N, P)] if fam == 'Series' else [])
        d += [('ups_raw', K, P)] + [('d%d_strength' % i, 1, P) for i in range(3)]
        d += [('Rinf', 1, T), ('induc', 1, T), ('q', K, T)] + [(e, 1, T) for e in err]
        if outl:
            d += [('sigma_out', N, T)]
        if fam == 'Parallel':
            d += [('Y_hat', N, T), ('Y_hat_re', N // 2, T), ('Y_hat_im', N // 2, T), ('Z_hat_p', N, T)]
        d += [('Z_hat', Nz, T), ('Z_hat_re', Nz, T), ('Z_hat_im', Nz, T), ('sigma_tot', Nz, T), ('ups', K, T), ('dups', K - 2, T)]
        if fam == 'Series' and not outl:
            d += [('Z_hat_tilde', N_tilde, G)]
        elif fam == 'Parallel' and not outl:
            d += [('Y_hat_tilde', N, G), ('Y_hat_re_tilde', N // 2, G), ('Y_hat_im_tilde', N // 2, G), ('Z_hat_p_tilde', N, G),
                  ('Z_hat_tilde', N, G)]
        return d
    if fam == 'Series-Parallel':
        sfx = ['s', 'p']
    elif fam == 'Series-2Parallel':
        sfx = ['s', 'p1', 'p2']
    else:
        raise ValueError('No model %s' % model_name)
    par = sfx[1:]
    kk = dict(zip(sfx, Ks))
    d += [('Rinf_raw', 1, P), ('induc_raw', 1, P), ('xs', kk['s'], P)] + [('x%s_raw' % s, kk[s], P) for s in par]
    d += [(e + '_raw', 1, P) for e in err]
    if outl:
        d += [('sigma_out_raw', N, P)]
    d += [('ups_%s_raw' % s, kk[s], P) for s in sfx]
    d += [('d%d%s_strength' % (i, s), 1, P) for s in sfx for i in range(3)]
    d += [('Rinf', 1, T), ('induc', 1, T)] + [('x%s' % s, kk[s], T) for s in par] + [('q%s' % s, kk[s], T) for s in sfx]
    d += [('x_sum_raw', 1, T), ('x_sum', 1, T)] + [(e, 1, T) for e in err]
    if outl:
        d += [('sigma_out', N, T)]
    if len(par) == 1:
        d += [('Y_hat', N, T), ('Y_hat_re', N // 2, T), ('Y_hat_im', N // 2, T), ('Z_hat_p', N, T)]
    else:
        for i in (1, 2):
            d += [('Y_hat%d' % i, N, T), ('Y_hat_re%d' % i, N // 2, T), ('Y_hat_im%d' % i, N // 2, T), ('Z_hat_p%d' % i, N, T)]
    d += [('Z_hat', N, T), ('Z_hat_re', N, T), ('Z_hat_im', N, T), ('sigma_tot', N, T)]
    d += [('ups_%s' % s, kk[s], T) for s in sfx] + [('dups_%s' % s, kk[s] - 2, T) for s in sfx]
    if len(par) == 1:
        d += [('Y_hat_tilde', N_tilde, G), ('Y_hat_re_tilde', N_tilde // 2, G), ('Y_hat_im_tilde', N_tilde // 2, G),
              ('Z_hat_p_tilde', N_tilde, G), ('Z_hat_tilde', N_tilde, G)]
    else:
        for i in (1, 2):
            d += [('Y_hat%d_tilde' % i, N, G), ('Y_hat_re%d_tilde' % i, N // 2, G), ('Y_hat_im%d_tilde' % i, N // 2, G),
                  ('Z_hat_p%d_tilde' % i, N, G)]
        d += [('Z_hat_tilde', N_tilde, G)]
    return d


def _dims_from_dat(model_name, dat):
    fam, _ = _family(model_name)
    if fam in ('Series', 'Parallel'):
        Ks = [np.shape(dat['A'])[1]]
    elif fam == 'Series-Parallel':
        Ks = [np.shape(dat['As'])[1], np.shape(dat['Ap'])[1]]
    else:
        Ks = [np.shape(dat['As'])[1], np.shape(dat['Ap1'])[1], np.shape(dat['Ap2'])[1]]
    N = int(dat['N']) if 'N' in dat else 2 * len(dat['freq'])
    return N, int(dat.get('N_tilde', 0)), Ks


def flat_parameter_count(model_name, dat):
    """Number of flat names pystan's `sampling()` compared with 1000 (`fit.sim['fnames_oi']`): every element of the declared
    parameters, transformed parameters and generated quantities, plus lp__.  For Series / Series_pos with the Stan data of
    `Inverter.fit` (N = 2 Nf, N_tilde = 2 Nf) that is 5 K + 13 + 8 Nf (parameters and transformed parameters) + N_tilde + 1."""
    N, N_tilde, Ks = _dims_from_dat(model_name, dat)
    return sum(s for _, s, _ in declared_columns(model_name, N, N_tilde, Ks)) + 1


def flatnames(name, size, scalar):
    return [name] if scalar else ['%s[%d]' % (name, i) for i in range(size)]


# ---------------------------------------------------------------------------------------------------- columns of a fit
def _saved_family(fit):
    if 'xp1' in fit:
        fam = 'Series-2Parallel'
    elif 'xs' in fit:
        fam = 'Series-Parallel'
    else:
        fam = 'Series'
    return fam + ('_outliers' if 'sigma_out_raw' in fit else '') + '_StanModel.pkl'


def fit_columns(fit):
    """(names, blocks) of the columns a fit provides: [(name, [draws x size] array, scalar)] in declaration order, lp__ last."""
    model = getattr(fit, '_model', None)
    if model is not None:
        P = model.problem
        N, N_tilde = model._N, model._N_tilde
        decl = declared_columns(model.model_name, N, N_tilde, P.Ks)
        scalars = {nm for nm, s, _ in decl if s == 1}
        get = fit.__getitem__
        has = model._can_extract
    else:
        decl = declared_columns(_saved_family(fit), 0, 0, [3, 3, 3])   # order only: sizes come from the arrays
        scalars = None
        derived = {'Z_hat_re', 'Z_hat_im'} if 'Z_hat' in fit else set()
        for nm in list(fit.keys()):
            if nm.startswith('ups') and not nm.endswith('_raw'):
                derived.add('d' + nm)
        get = lambda nm: fit[nm] if nm in fit else _derive_saved(fit, nm)    # noqa: E731
        has = lambda nm: nm in fit or nm in derived                          # noqa: E731
    cols = []
    for nm, _, _ in decl:
        if not has(nm):
            continue
        a = np.asarray(get(nm), dtype=np.float64)
        rows = a.shape[0]
        cols.append((nm, a.reshape(rows, -1), (a.ndim == 1) if scalars is None else (nm in scalars)))
    cols.append(('lp__', np.asarray(fit['lp__'], dtype=np.float64).reshape(-1, 1), True))
    return cols


def _derive_saved(fit, nm):
    if nm in ('Z_hat_re', 'Z_hat_im'):
        Zh = np.asarray(fit['Z_hat'])
        h = Zh.shape[1] // 2
        part = Zh[:, :h] if nm == 'Z_hat_re' else Zh[:, h:]
        return np.concatenate([part, part], axis=1)
    if nm.startswith('dups'):
        u = np.asarray(fit[nm[1:]])
        return 0.5 * (u[:, 1:-1] - 0.5 * (u[:, :-2] + u[:, 2:])) / u[:, 1:-1]
    raise KeyError(nm)


# ---------------------------------------------------------------------------------------------------- device reductions
def _host_draws(X, chains, is_pos, who):
    """(X as contiguous float64 [G, rows, C], whether it came as [rows, C], chains, is_pos as uint8 [C] or None) for the entry
    points that take host draws.  ValueError before the library is touched: the C side reads rows * C doubles and C flags."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64))
    one = X.ndim == 2
    if one:
        X = X[None]
    if X.ndim != 3:
        raise ValueError('%s: X must be [G, chains * draws, C] or [chains * draws, C]' % who)
    rows, Cn = X.shape[1:]
    chains = int(chains)
    if chains < 1 or rows % chains:
        raise ValueError('%s: %d draws do not split into %d chains' % (who, rows, chains))
    mask = None
    if is_pos is not None:
        mask = np.ascontiguousarray(np.asarray(is_pos, dtype=np.uint8))
        if mask.shape != (Cn,):
            raise ValueError('%s: is_pos must have one flag per column' % who)
    return X, one, chains, mask


def column_diagnostics(X, chains, is_pos=None):
    """mean, sd, n_eff, Rhat [G x C] of X [G groups, chains * draws, C columns] (or [chains * draws, C]: G = 1) on the GPU."""
    X, one, chains, mask = _host_draws(X, chains, is_pos, 'column_diagnostics')
    G, rows, Cn = X.shape
    lib = _lib.require_gpu()
    out = [np.empty((G, Cn)) for _ in range(4)]
    _lib.check(lib.bdrt_diagnostics(_lib.ptr(X), G, chains, rows // chains, Cn, Cn, _lib.ptr(mask),
                                    *[_lib.ptr(o) for o in out]), 'bdrt_diagnostics')
    return tuple(o[0] for o in out) if one else tuple(out)


def sampler_diagnostics(sampler, unit_lo, unit_hi, chains):
    """mean, sd, n_eff, Rhat [G x D] of the constrained parameters over the draws a sampler holds in HBM (units [unit_lo,
    unit_hi), `chains` consecutive units per group): one launch, no copy of the draws."""
    G = (unit_hi - unit_lo) // chains
    D = sampler.problem.D
    out = [np.empty((G, D)) for _ in range(4)]
    _lib.check(sampler._lib.bdrt_sampler_diagnostics(sampler.handle, int(unit_lo), int(unit_hi), int(chains),
                                                     *[_lib.ptr(o) for o in out]), 'bdrt_sampler_diagnostics')
    return tuple(out)


def _tail_probs(tail_probs, who):
    try:
        p_lo, p_hi = (float(p) for p in tail_probs)
    except (TypeError, ValueError):
        raise ValueError('%s: tail_probs must be two probabilities (p_lo, p_hi)' % who)
    if not (0.0 < p_lo < 1.0 and 0.0 < p_hi < 1.0) or not p_lo < p_hi:
        raise ValueError('%s: tail_probs need 0 < p_lo < p_hi < 1, got (%g, %g)' % (who, p_lo, p_hi))
    return p_lo, p_hi


def _rank_shape(who, chains, draws):
    """Checks that need no GPU: the split draws 2 * chains * (draws // 2) of one column must fit the kernel's LDS."""
    if chains < 1 or chains > 64:
        raise ValueError('%s: %d chains (1 ... 64)' % (who, chains))
    if draws < 2:
        raise ValueError('%s: %d draws per chain, the split chains need at least 2' % (who, draws))
    limit = _lib.load_library().bdrt_rank_max_draws()
    if 2 * chains * (draws // 2) > limit:
        raise ValueError('%s: %d split draws per column, the kernel holds at most %d' % (who, 2 * chains * (draws // 2), limit))


def _rank_dict(rhat, bulk, tail, essm, sd):
    with np.errstate(divide='ignore', invalid='ignore'):
        mcse = sd / np.sqrt(essm)
    return {'rhat': rhat, 'ess_bulk': bulk, 'ess_tail': tail, 'ess_mean': essm, 'mcse_mean': mcse, 'sd': sd}


def rank_diagnostics(X, chains, is_pos=None, tail_probs=TAIL_PROBS):
    """Rank-normalised diagnostics of X [G groups, chains * draws, C columns] (or [chains * draws, C]: G = 1) on the GPU: dict of
    'rhat' (rank-normalised, folded split R-hat), 'ess_bulk', 'ess_tail' (the smaller ESS of the indicators of the two
    `tail_probs` quantiles), 'ess_mean', 'mcse_mean', 'sd', each [G, C] (or [C]).  Definitions: tests/rank_numpy.py.  All on
    the split chains: an odd number of draws per chain drops the middle draw, of 'sd' too.  ValueError when the draws do not
    split into the chains, for tail probabilities outside 0 < p_lo < p_hi < 1, and when one column has more split draws than
    the kernel holds in LDS (bdrt_rank_max_draws(): 8192, i.e. 8 chains x 1000 or 4 x 2000)."""
    X, one, chains, mask = _host_draws(X, chains, is_pos, 'rank_diagnostics')
    G, rows, Cn = X.shape
    p_lo, p_hi = _tail_probs(tail_probs, 'rank_diagnostics')
    _rank_shape('rank_diagnostics', chains, rows // chains)
    lib = _lib.require_gpu()
    out = [np.empty((G, Cn)) for _ in range(5)]
    if G and Cn:
        _lib.check(lib.bdrt_rank_diagnostics(_lib.ptr(X), G, chains, rows // chains, Cn, Cn, _lib.ptr(mask), p_lo, p_hi,
                                             *[_lib.ptr(o) for o in out]), 'bdrt_rank_diagnostics')
    return _rank_dict(*[(o[0] if one else o) for o in out])


def sampler_rank_diagnostics(sampler, unit_lo, unit_hi, chains, tail_probs=TAIL_PROBS):
    """`rank_diagnostics` [G x D] of the constrained parameters over the draws a sampler holds in HBM (units [unit_lo, unit_hi),
    `chains` consecutive units per group): one launch, no copy of the draws."""
    chains = int(chains)
    if chains < 1 or unit_hi <= unit_lo or (unit_hi - unit_lo) % chains:
        raise ValueError('sampler_rank_diagnostics: units [%d, %d) do not split into groups of %d chains' % (unit_lo, unit_hi, chains))
    p_lo, p_hi = _tail_probs(tail_probs, 'sampler_rank_diagnostics')
    _rank_shape('sampler_rank_diagnostics', chains, int(sampler.n_draws))
    G = (unit_hi - unit_lo) // chains
    D = sampler.problem.D
    out = [np.empty((G, D)) for _ in range(5)]
    _lib.check(sampler._lib.bdrt_sampler_rank_diagnostics(sampler.handle, int(unit_lo), int(unit_hi), chains, p_lo, p_hi,
                                                          *[_lib.ptr(o) for o in out]), 'bdrt_sampler_rank_diagnostics')
    return _rank_dict(*out)


# ---------------------------------------------------------------------------------------------------- summary
def _quantile_names(probs):
    return ['{:g}%'.format(100 * p) for p in probs]


def _stacked_columns(fit, pars, who):
    """(flat names, X [chains * draws, n_flat]) of the columns of a fit, or of the parameters `pars` among them."""
    cols = fit_columns(fit)
    if pars is not None:
        want = [pars] if isinstance(pars, str) else list(pars)
        unknown = [p for p in want if p not in {c[0] for c in cols}]
        if unknown:
            raise ValueError('%s: unknown parameter(s) %s' % (who, unknown))
        cols = [c for c in cols if c[0] in want]
    names = [n for nm, a, sc in cols for n in flatnames(nm, a.shape[1], sc)]
    return names, np.hstack([a for _, a, _ in cols])


def summary(fit, pars=None, probs=DEFAULT_PROBS):
    """pystan's `fit.summary()`: dict with 'summary' [n_flat x (5 + len(probs))] (mean, se_mean, sd, quantiles, n_eff, Rhat),
    'summary_rownames', 'summary_colnames', and per chain 'c_summary' [n_flat x (2 + len(probs)) x chains] (mean, sd,
    quantiles), 'c_summary_rownames', 'c_summary_colnames'.  Quantiles: numpy's 'linear' rule (bdrt_percentiles)."""
    from . import post
    probs = tuple(float(p) for p in probs)
    names, X = _stacked_columns(fit, pars, 'summary')
    M, N = fit.chains, fit.n_draws
    mean, sd, n_eff, rhat = column_diagnostics(X, M)
    q = np.asarray(probs) * 100.0
    pct = post.percentile(X, q, axis=0).reshape(len(probs), X.shape[1])
    with np.errstate(divide='ignore', invalid='ignore'):
        se = sd / np.sqrt(n_eff)
    S = np.column_stack([mean, se, sd, pct.T, n_eff, rhat])
    Xc = X.reshape(M, N, -1)
    cs = np.empty((X.shape[1], 2 + len(probs), M))
    for m in range(M):
        cs[:, 0, m] = Xc[m].mean(axis=0)
        cs[:, 1, m] = Xc[m].std(axis=0, ddof=1) if N > 1 else np.nan
        cs[:, 2:, m] = np.percentile(Xc[m], q, axis=0).T
    qn = _quantile_names(probs)
    return {'summary': S, 'summary_rownames': np.array(names), 'summary_colnames': tuple(['mean', 'se_mean', 'sd'] + qn +
                                                                                          ['n_eff', 'Rhat']),
            'c_summary': cs, 'c_summary_rownames': np.array(names), 'c_summary_colnames': tuple(['mean', 'sd'] + qn)}


def rank_summary(fit, pars=None, probs=RANK_PROBS, tail_probs=TAIL_PROBS):
    """The table of `summary` with the diagnostics of Vehtari et al. 2021 in place of pystan's: dict with 'summary' [n_flat x
    (6 + len(probs))] (mean, mcse_mean, sd, quantiles, ess_bulk, ess_tail, Rhat), 'summary_rownames' (the rows of `summary`),
    'summary_colnames'.  Rhat is the rank-normalised, folded split R-hat (`rank_diagnostics`); mcse_mean = sd / sqrt(ess_mean);
    sd is that of the split chains.  Quantiles: numpy's 'linear' rule (bdrt_percentiles).  ess_tail is the ESS behind the
    `tail_probs` quantiles: tail_probs=(0.025, 0.975) gives the effective number of draws behind the package's own 95 % bands
    (`predict_distribution(percentile=)`, `coef_percentile`, `predict_Z(percentile=)`)."""
    from . import post
    probs = tuple(float(p) for p in probs)
    names, X = _stacked_columns(fit, pars, 'rank_summary')
    r = rank_diagnostics(X, fit.chains, tail_probs=tail_probs)
    mean = column_diagnostics(X, fit.chains)[0]
    pct = post.percentile(X, np.asarray(probs) * 100.0, axis=0).reshape(len(probs), X.shape[1])
    S = np.column_stack([mean, r['mcse_mean'], r['sd'], pct.T, r['ess_bulk'], r['ess_tail'], r['rhat']])
    return {'summary': S, 'summary_rownames': np.array(names),
            'summary_colnames': tuple(['mean', 'mcse_mean', 'sd'] + _quantile_names(probs) + ['ess_bulk', 'ess_tail', 'Rhat'])}


def stansummary(fit, pars=None, probs=DEFAULT_PROBS, digits_summary=2):
    """pystan's printed table (`print(fit)` / `fit.stansummary()`) as a string."""
    s = summary(fit, pars, probs)
    S, rn, cn = s['summary'], s['summary_rownames'], s['summary_colnames']
    head = 'Inference for the GPU model: {} chains, each with iter={}; warmup={}; thin=1;\npost-warmup draws per chain={}, ' \
           'total post-warmup draws={}.\n\n'.format(fit.chains, getattr(fit, 'warmup', 0) + fit.n_draws,
                                                   getattr(fit, 'warmup', 0), fit.n_draws, fit.chains * fit.n_draws)
    w = max([len(r) for r in rn] + [4]) + 2
    lines = [' ' * w + ''.join('{:>9}'.format(c) for c in cn)]
    for r, row in zip(rn, S):
        cells = []
        for j, (c, v) in enumerate(zip(cn, row)):
            if c == 'n_eff':
                cells.append('{:>9}'.format('nan' if not np.isfinite(v) else '%d' % int(round(v))))
            elif c == 'Rhat':
                cells.append('{:>9}'.format('%.2f' % v))
            else:
                cells.append('{:>9}'.format('%.*f' % (digits_summary, v)))
        lines.append('{:<{w}}'.format(r, w=w) + ''.join(cells))
    tail = '\n\nSamples were drawn using NUTS at the GPU sampler.\nFor each parameter, n_eff is a crude measure of effective ' \
           'sample size,\nand Rhat is the potential scale reduction factor on split chains (at \nconvergence, Rhat=1).'
    return head + '\n'.join(lines) + tail


# ---------------------------------------------------------------------------------------------------- checks and wording
def divergence_message(n_div, n_total, adapt_delta=0.9):
    return ['{} of {} iterations ended with a divergence ({:.3g} %).'.format(n_div, n_total, 100.0 * n_div / n_total),
            'Try running with adapt_delta larger than {} to remove the divergences.'.format(adapt_delta)]


def treedepth_message(n_max, n_total, max_treedepth=10):
    return ['{} of {} iterations saturated the maximum tree depth of {} ({:.3g} %)'.format(n_max, n_total, max_treedepth,
                                                                                           100.0 * n_max / n_total),
            'Run again with max_treedepth larger than {} to avoid saturation'.format(max_treedepth)]


RHAT_MESSAGE = 'Rhat above 1.1 or below 0.9 indicates that the chains very likely have not mixed'
NEFF_MESSAGE = 'n_eff / iter below 0.001 indicates that the effective sample size has likely been overestimated'
RANK_RHAT_MESSAGE = 'Rank-normalised Rhat above 1.01 indicates that the chains have not mixed'
ESS_BULK_MESSAGE = 'Bulk ESS below 100 per chain indicates that posterior means and medians may be unreliable'
ESS_TAIL_MESSAGE = 'Tail ESS below 100 per chain indicates that posterior variances and tail quantiles may be unreliable'
SKIP_MESSAGE = ('Maximum (flat) parameter count ({}) exceeded: skipping diagnostic tests for n_eff and Rhat.\n'
                'To run all diagnostics call bayes_drt_amd.diagnostics.check_hmc_diagnostics(fit)').format(MAX_FLAT)


def _control(fit):
    c = getattr(fit, 'control', None) or {}
    return float(c.get('adapt_delta', 0.9)), int(c.get('max_treedepth', 10))


def _checks_arg(checks):
    if checks is None:
        return list(CHECKS)
    checks = [checks] if isinstance(checks, str) else list(checks)
    if 'energy' in checks:
        raise NotImplementedError("the E-BFMI check ('energy') needs the Hamiltonian of every draw, which no sampler kernel "
                                  "records; the other checks are %s" % (CHECKS,))
    bad = [c for c in checks if c not in CHECKS + RANK_CHECKS]
    if bad:
        raise ValueError('unknown check(s) %s' % bad)
    return checks


def report(n_eff, rhat, total_draws, chain_div, chain_treedepth, adapt_delta=0.9, max_treedepth=10, checks=None, verbose=True,
           per_chain=False, prefix='', rank_rhat=None, ess_bulk=None, ess_tail=None):
    """Log pystan's lines for precomputed values and return {check: passed}.  n_eff / rhat: flat arrays (may be None when the
    check is not requested); chain_div / chain_treedepth: per-chain counts.  rank_rhat / ess_bulk / ess_tail: flat arrays for
    the checks of RANK_CHECKS, which run only when `checks` names them: 'rank_Rhat' fails when a value is > 1.01 or NaN, the
    ESS checks when a value is below 100 x chains or NaN."""
    checks = _checks_arg(checks)
    out = {}
    n_chains = len(chain_div)
    per = total_draws // max(1, n_chains)
    if 'n_eff' in checks:
        ratio = np.asarray(n_eff, dtype=float) / float(total_draws)
        ok = not bool(np.any(ratio < 0.001))
        if not ok:
            logger.warning(prefix + NEFF_MESSAGE)
        elif verbose:
            logger.info(prefix + 'n_eff / iter looks reasonable for all parameters')
        out['n_eff'] = ok
    if 'Rhat' in checks:
        r = np.asarray(rhat, dtype=float)
        ok = not bool(np.any(~np.isfinite(r) | (r > 1.1) | (r < 0.9)))
        if not ok:
            logger.warning(prefix + RHAT_MESSAGE)
        elif verbose:
            logger.info(prefix + 'Rhat looks reasonable for all parameters')
        out['Rhat'] = ok
    if 'divergence' in checks:
        n = int(np.sum(chain_div))
        if per_chain:
            for i, k in enumerate(chain_div):
                if k:
                    logger.warning(prefix + 'Chain {}: '.format(i + 1) + divergence_message(int(k), per, adapt_delta)[0])
        if n:
            for line in divergence_message(n, total_draws, adapt_delta):
                logger.warning(prefix + line)
        elif verbose:
            logger.info(prefix + 'No divergent transitions found.')
        out['divergence'] = n == 0
    if 'treedepth' in checks:
        n = int(np.sum(chain_treedepth))
        if per_chain:
            for i, k in enumerate(chain_treedepth):
                if k:
                    logger.warning(prefix + 'Chain {}: '.format(i + 1) + treedepth_message(int(k), per, max_treedepth)[0])
        if n:
            for line in treedepth_message(n, total_draws, max_treedepth):
                logger.warning(prefix + line)
        elif verbose:
            logger.info(prefix + 'No iterations saturated the maximum tree depth of {}.'.format(max_treedepth))
        out['treedepth'] = n == 0
    if 'rank_Rhat' in checks:
        r = np.asarray(rank_rhat, dtype=float)
        ok = not bool(np.any(np.isnan(r) | (r > RANK_RHAT_MAX)))
        if not ok:
            logger.warning(prefix + RANK_RHAT_MESSAGE)
        elif verbose:
            logger.info(prefix + 'Rank-normalised Rhat looks reasonable for all parameters')
        out['rank_Rhat'] = ok
    for name, vals, msg in (('ess_bulk', ess_bulk, ESS_BULK_MESSAGE), ('ess_tail', ess_tail, ESS_TAIL_MESSAGE)):
        if name in checks:
            e = np.asarray(vals, dtype=float)
            ok = not bool(np.any(np.isnan(e) | (e < ESS_PER_CHAIN_MIN * n_chains)))
            if not ok:
                logger.warning(prefix + msg)
            elif verbose:
                logger.info(prefix + '%s ESS looks reasonable for all parameters' % ('Bulk' if name == 'ess_bulk' else 'Tail'))
            out[name] = ok
    return out


def check_hmc_diagnostics(fit, pars=None, verbose=True, per_chain=False, checks=None):
    """pystan.check_hmc_diagnostics: {'n_eff', 'Rhat', 'divergence', 'treedepth'} -> bool, pystan's wording logged at WARNING
    to logging.getLogger('bayes_drt_amd') (verbose: the all-clear lines at INFO).  n_eff fails when n_eff / total draws <
    0.001 for some column; Rhat when some Rhat is > 1.1, < 0.9, NaN or inf.  Divergence and tree-depth counts are the
    sampler's per-chain counters.  The E-BFMI check ('energy') is not available (module docstring).
    `checks` may also name 'rank_Rhat', 'ess_bulk' and 'ess_tail' (RANK_CHECKS; never part of the default): the thresholds of
    Vehtari et al. 2021 on the values of `rank_summary` -- rank-normalised Rhat > 1.01 or NaN fails, bulk / tail ESS below
    100 x chains or NaN fails."""
    checks = _checks_arg(checks)
    n_eff = rhat = None
    if 'n_eff' in checks or 'Rhat' in checks:
        s = summary(fit, pars)
        n_eff, rhat = s['summary'][:, -2], s['summary'][:, -1]
    rank = {}
    if any(c in RANK_CHECKS for c in checks):
        rs = rank_summary(fit, pars)['summary']
        rank = dict(rank_rhat=rs[:, -1], ess_bulk=rs[:, -3], ess_tail=rs[:, -2])
    diag = fit.diagnostics
    ad, td = _control(fit)
    return report(n_eff, rhat, fit.chains * fit.n_draws, [d['n_divergent'] for d in diag], [d['n_max_treedepth'] for d in diag],
                  ad, td, checks, verbose, per_chain, **rank)


def auto_check(fit, flat_count, prefix='', n_eff=None, rhat=None):
    """What pystan's `sampling()` ran after every fit: all checks, or divergence and tree depth alone (with pystan's message)
    when the model has more than 1000 flat names.  n_eff / rhat: precomputed values (fit_many), else reduced here."""
    checks = list(CHECKS)
    if flat_count > MAX_FLAT:
        logger.warning(prefix + SKIP_MESSAGE)
        checks = ['divergence', 'treedepth']
    elif n_eff is None:
        s = summary(fit)
        n_eff, rhat = s['summary'][:, -2], s['summary'][:, -1]
    diag = fit.diagnostics
    ad, td = _control(fit)
    out = report(n_eff, rhat, fit.chains * fit.n_draws, [d['n_divergent'] for d in diag], [d['n_max_treedepth'] for d in diag],
                 ad, td, checks, True, False, prefix)
    fit.hmc_check = dict(out, n_eff_values=n_eff, Rhat_values=rhat)     # what the check saw (None where skipped)
    return out


def batch_check(fits, flat_count, param_stats=None, index=None):
    """`auto_check` of the fits of one `fit_many` batch (same model, same chains and draws).  n_eff / Rhat of all fits are
    reduced in one launch of `bdrt_diagnostics` over the columns after the parameters block; param_stats = (mean, sd, n_eff,
    Rhat) [n_fits x D] of the parameters block, reduced on the sampler's device draws (`Sampler.diagnostics`), or None (then
    the parameters go through the same launch).  index: the spectra's positions in the caller's list (the 'spectrum i: '
    prefix of the logged lines); default 0, 1, ..."""
    index = list(range(len(fits))) if index is None else list(index)
    if not fits:
        return []
    if flat_count > MAX_FLAT:
        return [auto_check(f, flat_count, 'spectrum %d: ' % i) for i, f in zip(index, fits)]
    skip = set()
    if param_stats is not None:
        m = fits[0]._model
        skip = {nm for nm, _, blk in declared_columns(m.model_name, m._N, m._N_tilde, m.problem.Ks) if blk == 'parameters'}
    X = np.stack([np.hstack([a for nm, a, _ in fit_columns(f) if nm not in skip]) for f in fits])
    _, _, ne, rh = column_diagnostics(X, fits[0].chains)
    if param_stats is not None:
        ne = np.hstack([param_stats[2], ne])
        rh = np.hstack([param_stats[3], rh])
    return [auto_check(f, flat_count, 'spectrum %d: ' % index[k], ne[k], rh[k]) for k, f in enumerate(fits)]
