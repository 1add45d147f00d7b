"""Power-scaling sensitivity on the GPU: the kernels of bdrt_powerscale.hip against the numpy statement
(tests/powerscale_numpy.py, tests/psis_numpy.psislw) on identical input, batch independence, the prior component against two
data sets, and the surface (`Inverter.powerscale`, `fit(..., powerscale=True)`, `Sampler.powerscale`, `powerscale_many`).

Tolerances.  NaN / inf patterns and n_tail: equal exactly.  cjs2 lies in [0, 1] and is compared by absolute difference; the log
weights and pareto_k follow the rule tests/test_gpu_loo.py states for elpd_loo and pareto_k: 100 x the largest deviation measured
on these inputs on the MI355X (profiles/powerscale/parity.txt), so that another fixed summation order in a later kernel does not
break the test; never looser than 1e-10 (cjs2) and 1e-8 (log weights, pareto_k) absolute, which are conditions on the kernels
and not measurements."""
import copy
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests import powerscale_numpy as pw
from tests import psis_numpy as pn
from tests.helpers import load

pytestmark = pytest.mark.gpu

# measured on the MI355X (profiles/powerscale/parity.txt): largest |kernel - numpy statement| over all inputs below
MEASURED_CJS, MEASURED_LW, MEASURED_K = 1.1e-12, 2.5e-14, 5.1e-14
TOL_CJS = min(100 * MEASURED_CJS, 1e-10)
TOL_LW = min(100 * MEASURED_LW, 1e-8)
TOL_K = min(100 * MEASURED_K, 1e-8)

SIZES = [37, 513, 1000, 8192]                        # a partial wave, no multiple of 512, a round count, the LDS limit
LO, HI = pw.LOWER_ALPHA, pw.UPPER_ALPHA


def _same_pattern(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and \
        np.array_equal(np.isneginf(got), np.isneginf(ref))


# ---------------------------------------------------------------------------------------------------- the distance kernel
@functools.lru_cache(maxsize=None)
def _cjs_case(S):
    """X [5, S], w [4, S] and the numpy statement's cjs2 [5, 4].  Columns: Gaussian; Student-t rounded to one decimal (tie
    runs); constant; log-normal; Gaussian on a grid of 7 values (long tie runs).  Weights: psislw of Gaussian log ratios at
    alpha = 0.99 and 1.01, of heavier ones at 1.01, and one dominant draw (Q jumps by 0.9 there)."""
    rng = np.random.default_rng(S)
    X = np.stack([rng.standard_normal(S), np.round(rng.standard_t(4, S), 1), np.full(S, -1.25), np.exp(1.5 * rng.standard_normal(S)),
                  np.round(rng.standard_normal(S))])
    L = 40.0 * rng.standard_normal(S) - 300.0
    w = np.stack([np.exp(pn.psislw((LO - 1.0) * L)[0]), np.exp(pn.psislw((HI - 1.0) * L)[0]),
                  np.exp(pn.psislw((HI - 1.0) * 400.0 * rng.standard_t(5, S))[0]), np.full(S, 0.1 / (S - 1))])
    w[3, S // 3] = 0.9
    ref = np.array([[pw.cjs2(x, wk) for wk in w] for x in X])
    for a in (X, w, ref):
        a.setflags(write=False)
    return X, w, ref


@pytest.mark.parametrize('Cn', [1, 5])
@pytest.mark.parametrize('S', SIZES)
def test_distance_kernel_matches_numpy_statement(S, Cn):
    from bayes_drt_amd.powerscale import debug_cjs
    X, w, ref = _cjs_case(S)
    got = debug_cjs(X[:Cn], w)
    dev = np.abs(got - ref[:Cn])
    print('cjs2 (S, C) = %s: values %.3g ... %.3g, largest deviation %.3g' % ((S, Cn), ref[:Cn].min(), ref[:Cn].max(), dev.max()))
    assert got.shape == (Cn, 4) and np.all(np.isfinite(got)) and np.all((got >= 0) & (got <= 1))
    assert dev.max() <= TOL_CJS
    if Cn == 5:
        assert np.all(got[2] == 0.0)                                        # the constant column: 0, not NaN
        assert np.all(ref[[0, 1, 3, 4]] > 0)


def test_distance_kernel_special_inputs():
    from bayes_drt_amd.powerscale import debug_cjs
    X, w, ref = _cjs_case(513)
    S = 513
    uni = np.full((4, S), 1.0 / S)
    got = debug_cjs(X, uni)
    print('uniform weights: largest cjs2 %.3g' % got.max())
    assert np.all((got >= 0) & (got <= 1e-12))
    # affine maps of the columns, also decreasing ones
    for a, b in ((2.5, -1.0), (-0.75, 3.0)):
        g2 = debug_cjs(a * X + b, w)
        assert np.abs(g2 - debug_cjs(X, w)).max() <= 1e-12
    # non-finite values: that column, or that weight vector, only
    Xn = np.array(X)
    Xn[1, 7] = np.nan
    Xn[3, 9] = np.inf
    wn = np.array(w)
    wn[2, 100] = np.nan
    got = debug_cjs(Xn, wn)
    bad = np.zeros((5, 4), dtype=bool)
    bad[[1, 3]] = True
    bad[:, 2] = True
    assert np.array_equal(np.isnan(got), bad)
    assert np.array_equal(got[~bad], debug_cjs(X, w)[~bad])


# ---------------------------------------------------------------------------------------------------- the weights kernel
@functools.lru_cache(maxsize=None)
def _weights_case(S):
    """L [3, 2, S] and the numpy statement's (lw [3, 4, S], k [3, 4], n_tail [3, 4]).  Fit 1 has an all-equal prior component,
    fit 2 a NaN in its likelihood component."""
    rng = np.random.default_rng(S + 1)
    L = np.stack([np.stack([30.0 * rng.standard_normal(S) - 200.0, 80.0 * rng.standard_t(6, S) + 1500.0]) for _ in range(3)])
    L[1, 0] = -123.5
    L[2, 1, S // 2] = np.nan
    lw, k, nt = np.empty((3, 4, S)), np.empty((3, 4)), np.empty((3, 4), dtype=np.int32)
    for g in range(3):
        for c in range(2):
            for a, alpha in enumerate((LO, HI)):
                lw[g, 2 * c + a], k[g, 2 * c + a], nt[g, 2 * c + a] = pw.weights(L[g, c], alpha)
    for a in (L, lw, k, nt):
        a.setflags(write=False)
    return L, lw, k, nt


@pytest.mark.parametrize('S', [20] + SIZES)
def test_weights_kernel_matches_psislw(S):
    from bayes_drt_amd.powerscale import debug_weights
    L, lw, k, nt = _weights_case(S)
    got = debug_weights(L, LO, HI)
    assert np.array_equal(got['n_tail'], nt), (got['n_tail'], nt)
    assert _same_pattern(got['pareto_k'], k) and _same_pattern(got['lw'], lw) and _same_pattern(got['w'], np.exp(lw))
    f, fk = np.isfinite(lw), np.isfinite(k)
    d_lw = np.abs(got['lw'][f] - lw[f]).max()
    d_k = np.abs(got['pareto_k'][fk] - k[fk]).max() if fk.any() else 0.0
    print('weights S = %d: n_tail %s, k %s; largest deviation lw %.3g, k %.3g' % (
        S, sorted(set(nt.reshape(-1).tolist())), np.array2string(k[fk], precision=2), d_lw, d_k))
    assert d_lw <= TOL_LW and d_k <= TOL_K
    assert np.all(np.abs(got['w'][f] - np.exp(lw[f])) <= 1e-12 * np.exp(lw[f]) + TOL_LW * np.exp(lw[f]))
    # the all-equal component: raw equal weights, k = inf; the NaN component: NaN, n_tail 0
    assert np.all(got['pareto_k'][1, :2] == np.inf) and np.all(got['n_tail'][1, :2] == 0)
    assert np.all(got['w'][1, :2] == got['w'][1, 0, 0]) and abs(got['w'][1, 0, 0] * S - 1.0) <= 1e-14
    assert np.all(np.isnan(got['pareto_k'][2, 2:])) and np.all(got['n_tail'][2, 2:] == 0) and np.all(np.isnan(got['w'][2, 2:]))
    assert np.all(np.isfinite(got['w'][2, :2]))
    if S == 20:                                                             # at most 4 tail values: raw weights, k = inf
        assert np.all(nt <= 4) and np.all(np.isinf(got['pareto_k']) | np.isnan(got['pareto_k']))
    else:
        assert np.all(np.isfinite(got['pareto_k'][0]))


# ---------------------------------------------------------------------------------------------------- batch independence
def test_a_column_and_a_fit_do_not_depend_on_the_launch():
    from bayes_drt_amd.powerscale import debug_cjs, debug_weights
    X, w, _ = _cjs_case(1000)
    all5 = debug_cjs(X, w)
    for c in range(5):
        assert np.array_equal(debug_cjs(X[c], w)[0], all5[c]), c
    assert np.array_equal(debug_cjs(X[::-1], w), all5[::-1])
    L, _, _, _ = _weights_case(1000)
    all3 = debug_weights(L, LO, HI)
    for g in range(3):
        one = debug_weights(L[g], LO, HI)
        for key in all3:
            assert np.array_equal(one[key], all3[key][g], equal_nan=True), (g, key)


def test_draw_limit_is_named():
    from bayes_drt_amd import powerscale as PS
    assert PS.max_draws() == 8192
    S = PS.max_draws() + 1
    with pytest.raises(ValueError, match='8192'):
        PS.debug_cjs(np.zeros((1, S)), np.full((4, S), 1.0 / S))
    with pytest.raises(ValueError, match='8192'):
        PS.debug_weights(np.zeros((2, S)))
    from bayes_drt_amd import _lib
    lib = _lib.require_gpu()
    out = np.empty(4)
    assert lib.bdrt_debug_powerscale_cjs(_lib.ptr(np.zeros(S)), _lib.ptr(np.zeros(4 * S)), 1, S, _lib.ptr(out)) == -2
    assert b'at most 8192' in lib.bdrt_last_error()


# ---------------------------------------------------------------------------------------------------- the pipeline on a problem
NF_SMALL = 21


@functools.lru_cache(maxsize=None)
def _small():
    """A Series problem of 21 frequencies (every third of the fixture's grid) with three spectra, one sampler run of 3 x 2 chains
    of 60 draws on it, kept open: (sampler, problem, Z [3, 42], downloaded draws [3, 120, D])."""
    from bayes_drt_amd import _lib
    from bayes_drt_amd import parallel as par
    from bayes_drt_amd.engine import Sampler
    from bayes_drt_amd.model import Problem
    d = load('dat_sample_2ZARC_uniform_0.25_K81')
    nf = len(d['freq'])
    sel = np.arange(0, nf, 3)[:NF_SMALL]
    rows = np.concatenate([sel, nf + sel])
    blk = dict(A=np.ascontiguousarray(d['A'][rows]), L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=True)
    rs = np.random.RandomState(2)
    z0 = np.asarray(d['Z'], dtype=float)[rows]
    Z = np.stack([z0 * (1 + 0.01 * k) + 0.002 * rs.standard_normal(z0.shape) for k in range(3)])
    prob = Problem([blk], Z, np.asarray(d['freq'], dtype=float)[sel], sigma_min=float(d['sigma_min']), ups_alpha=1.0, ups_beta=0.1)
    assert prob.nf == len(sel) <= NF_SMALL
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    chains, n_draws = 2, 60
    spec, chain = par.make_units(3, chains)
    smp = Sampler(prob, 3 * chains, 30, n_draws, 21, ctrl, spec=spec, chain_ids=chain)
    smp.run()
    draws = smp.results()[0].reshape(3, chains * n_draws, prob.D)
    return smp, prob, Z, draws


def test_prior_component_does_not_see_the_data():
    """L_pri = lp0 - L_lik of the same random draws against two data sets: equal to 1e-9 relative, while L_lik moves.  A wrong
    column slice between the evaluator's likelihood and the pointwise one would leave a data term in the difference."""
    from bayes_drt_amd.powerscale import host_powerscale
    _, prob, Z, _ = _small()
    rs = np.random.RandomState(9)
    theta = rs.uniform(-2, 2, (1, 64, prob.D))
    a = host_powerscale(prob, theta, 1, spec=[0], components=True)['L'][0]
    b = host_powerscale(prob, theta, 1, spec=[2], components=True)['L'][0]
    Z2 = Z[::-1] * 1.3 + 0.05
    prob.set_Z(Z2)
    try:
        c = host_powerscale(prob, theta, 1, spec=[1], components=True)['L'][0]
    finally:
        prob.set_Z(Z)
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(np.isfinite(c))
    rel = max(np.abs(b[0] - a[0]).max() / np.abs(a[0]).max(), np.abs(c[0] - a[0]).max() / np.abs(a[0]).max())
    print('prior component: |L_pri| up to %.3g, |L_lik| up to %.3g, largest relative change of L_pri %.3g, of L_lik %.3g' % (
        np.abs(a[0]).max(), np.abs(a[1]).max(), rel, np.abs(c[1] - a[1]).max() / np.abs(a[1]).max()))
    assert np.all(np.abs(b[0] - a[0]) <= 1e-9 * np.abs(a[0])) and np.all(np.abs(c[0] - a[0]) <= 1e-9 * np.abs(a[0]))
    assert np.abs(c[1] - a[1]).max() > 1e-3 * np.abs(a[1]).max()
    # the components are what the host entry points give: lp0 without the Jacobian term, the numpy log-likelihood
    lp0 = prob.logp_grad(theta[0], jacobian=False, want_grad=False)[0]
    _, Zh, sg = prob.transformed(theta[0])
    L_pri, L_lik = pw.components(lp0, pn.pointwise_log_lik(Zh, sg, Z[0]))
    tol = 1e-11 * (np.abs(lp0) + np.abs(L_lik))                             # (both are sums in another order, and L_pri a difference)
    assert np.all(np.abs(a[1] - L_lik) <= tol) and np.all(np.abs(a[0] - L_pri) <= tol)


def _statement(prob, theta, z, cols=slice(None), spec=0):
    """The numpy statement on what the host entry points give for the draws theta [S, D] against spectrum `spec` (= z)."""
    lp0 = prob.logp_grad(theta, jacobian=False, spec=np.full(len(theta), spec), want_grad=False)[0]
    par, Zh, sg = prob.transformed(theta)
    return pw.powerscale(lp0, pn.pointwise_log_lik(Zh, sg, z)[:, cols], par)


def _assert_statement(got_cjs2, got_k, got_nt, ref, what):
    cj = np.asarray(got_cjs2).reshape(-1, 2, 2)
    d_c = np.abs(cj - ref['cjs2']).max()
    d_k = np.abs(np.asarray(got_k).reshape(2, 2) - ref['pareto_k']).max()
    print('%s: cjs2 up to %.3g, k %s, n_tail %s; largest deviation cjs2 %.3g, k %.3g' % (
        what, ref['cjs2'].max(), np.array2string(ref['pareto_k'].reshape(-1), precision=2), ref['n_tail'].reshape(-1).tolist(), d_c, d_k))
    assert np.array_equal(np.asarray(got_nt).reshape(2, 2), ref['n_tail'])
    assert d_c <= TOL_CJS and d_k <= TOL_K


@pytest.mark.parametrize('part', ['both', 'real', 'imag'])
def test_sampler_path_equals_host_path_and_the_statement(part):
    """`Sampler.powerscale` against `host_powerscale` on the downloaded draws, bit for bit, alone, in a batch of three and in
    chunks of one group; and against the numpy statement on the host entry points' output."""
    from bayes_drt_amd.powerscale import host_powerscale
    smp, prob, Z, draws = _small()
    dev = smp.powerscale(0, smp.n_units, 2, part=part)
    host = host_powerscale(prob, draws, 2, spec=[0, 1, 2], part=part)
    chunked = smp.powerscale(0, smp.n_units, 2, part=part, chunk_bytes=1)
    alone = host_powerscale(prob, draws[1:2], 2, spec=[1], part=part)
    pair = smp.powerscale(2, 6, 2, part=part)
    for k in ('cjs2', 'pareto_k', 'n_tail'):
        assert dev[k].shape == host[k].shape and dev[k].dtype == host[k].dtype
        assert np.array_equal(dev[k], host[k], equal_nan=True), k
        assert np.array_equal(dev[k], chunked[k], equal_nan=True), k
        assert np.array_equal(dev[k][1], alone[k][0], equal_nan=True), k
        assert np.array_equal(dev[k][1:], pair[k], equal_nan=True), k
    assert dev['cjs2'].shape == (3, prob.D, 4) and np.all(np.isfinite(dev['cjs2'])) and np.all((dev['cjs2'] >= 0) & (dev['cjs2'] <= 1))
    cols = {'both': slice(None), 'real': slice(0, prob.nf), 'imag': slice(prob.nf, 2 * prob.nf)}[part]
    for g in (0, 2):
        _assert_statement(dev['cjs2'][g], dev['pareto_k'][g], dev['n_tail'][g], _statement(prob, draws[g], Z[g], cols, g),
                          'sampler, part %s, spectrum %d' % (part, g))


def test_sampler_entry_refuses_bad_arguments():
    from bayes_drt_amd import _lib
    smp, prob, _, _ = _small()
    lib = prob._lib
    out = (_lib.ptr(np.empty((3, prob.D, 4))), _lib.ptr(np.empty((3, 4))), _lib.ptr(np.empty((3, 4), dtype=np.int32)))
    n2 = 2 * prob.nf
    assert lib.bdrt_sampler_powerscale(smp.handle, 0, 3, 2, 0, n2, LO, HI, 0, *out) == -1
    assert b'bdrt_sampler_powerscale: bad unit range' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_powerscale(smp.handle, 0, 6, 2, prob.nf, prob.nf + 1, LO, HI, 0, *out) == -1
    assert b'bad column range' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_powerscale(smp.handle, 0, 6, 2, 0, n2, HI, LO, 0, *out) == -1
    assert b'alpha_lo' in lib.bdrt_last_error()
    with pytest.raises(ValueError, match='do not split into groups of 4'):
        smp.powerscale(0, 6, 4)
    with pytest.raises(ValueError, match='lower_alpha'):
        smp.powerscale(0, 6, 2, lower_alpha=1.2)


# ---------------------------------------------------------------------------------------------------- Inverter surface
BASIS = np.logspace(6, -2, 81)
NAMES = ['trunc_uniform_0.25', 'trunc_Orazem_1.0']


def _spectrum(name):
    d = load('kat_' + name)
    return np.array(d['data_freq'], dtype=float), np.array(d['data_Z'])


def _equal_results(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=(np.asarray(a[k]).dtype.kind == 'f')), k


def test_inverter_powerscale_end_to_end(tmp_path):
    from bayes_drt_amd import powerscale as PS
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', warmup=60, samples=100, chains=2, random_seed=3, check_diagnostics=False, powerscale=True)
    stored = inv.powerscale_result
    fit = inv._sample_result
    prob = fit._model.problem
    res = inv.powerscale()
    assert res is inv.powerscale_result and res is not stored
    _equal_results(res, stored)                                             # reduced while the sampler held the draws: same bits
    D = prob.D
    assert len(res.names) == D == len(set(res.names)) and res.names[0] == 'Rinf_raw' and 'x[80]' in res.names
    assert res.prior.shape == res.likelihood.shape == (D,) and len(res.diagnosis) == D and res.cjs2.shape == (D, 2, 2)
    assert res.pareto_k.shape == res.n_tail.shape == (2, 2) and res.n_draws == 200 and res.alphas == (0.99, 1.01)
    assert np.all(np.isfinite(res.prior)) and np.all(np.isfinite(res.likelihood)) and np.all(res.prior >= 0)
    # the numpy statement on the host draws
    z = np.asarray(inv._stan_input['Z'], dtype=float)
    ref = _statement(prob, fit.theta, z)
    _assert_statement(res.cjs2, res.pareto_k, res.n_tail, ref, 'Inverter.powerscale, 2 x 100 draws')
    assert np.allclose(res.prior, ref['prior'], rtol=0, atol=np.sqrt(TOL_CJS) / np.log2(1.01))
    assert set(res.flagged()) == {n for n, d in zip(res.names, res.diagnosis) if d != '-'} | \
        {n for n, l in zip(res.names, res.likelihood) if l >= res.threshold}
    print('\n'.join(str(res).split('\n')[:4] + ['...', str(res).split('\n')[-1]]))
    # one half of the observations as the likelihood; another threshold and other powers
    re_ = inv.powerscale(part='real')
    assert re_.cjs2.shape == (D, 2, 2) and np.all(np.isfinite(re_.cjs2)) and re_.part == 'real'
    _assert_statement(re_.cjs2, re_.pareto_k, re_.n_tail, _statement(prob, fit.theta, z, slice(0, len(f))), 'part real')
    assert not np.array_equal(re_.cjs2, res.cjs2)
    wide = inv.powerscale(lower_alpha=0.98, upper_alpha=1.02, threshold=0.01)
    assert wide.alphas == (0.98, 1.02) and wide.threshold == 0.01 and np.all(np.isfinite(wide.cjs2))    # save -> load carries the result; a restored fit has no model to evaluate
    inv.powerscale()
    fn = str(tmp_path / 'fit.pkl')
    inv.save_fit_data(fn)
    inv2 = Inverter(basis_freq=BASIS)
    inv2.load_fit_data(fn)
    _equal_results(inv2.powerscale_result, res)
    assert isinstance(inv2.powerscale_result, PS.PowerscaleResult)
    with pytest.raises(ValueError, match='live sampling fit'):
        inv2.powerscale()
    # a MAP fit has no draws to reweight
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='optimize')
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.powerscale()


def test_fit_many_stores_what_powerscale_many_would():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    rs = np.random.RandomState(4)
    zs = [Z, Z * (1 + 0.01 * rs.standard_normal(len(Z))), Z + 0.005 * np.abs(Z).max() * rs.standard_normal(len(Z))]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = Inverter(basis_freq=BASIS).fit_many(f, zs, mode='sample', warmup=60, samples=100, chains=2, random_seed=8,
                                                    check_outliers=False, check_diagnostics=False, powerscale=True,
                                                    powerscale_kw=dict(threshold=0.03))
    cp = [copy.copy(v) for v in views]
    many = Inverter.powerscale_many(cp, threshold=0.03)
    chunked = Inverter.powerscale_many([copy.copy(v) for v in views], threshold=0.03, chunk_bytes=1)
    for i, (v, c, m, ch) in enumerate(zip(views, cp, many, chunked)):
        assert v.powerscale_result is not m and c.powerscale_result is m and m.threshold == 0.03 and m.n_draws == 200
        _equal_results(v.powerscale_result, m)
        _equal_results(m, ch)
        _equal_results(m, copy.copy(v).powerscale(threshold=0.03))
    assert not np.array_equal(many[0].cjs2, many[1].cjs2)
    fit = views[1]._sample_result
    z = np.asarray(views[1]._stan_input['Z'], dtype=float)
    prob = fit._model.problem
    lp0 = prob.logp_grad(fit.theta, jacobian=False, spec=np.full(len(fit.theta), 1), want_grad=False)[0]
    par, Zh, sg = prob.transformed(fit.theta)
    ref = pw.powerscale(lp0, pn.pointwise_log_lik(Zh, sg, z), par, threshold=0.03)
    _assert_statement(many[1].cjs2, many[1].pareto_k, many[1].n_tail, ref, 'fit_many view 1')
    assert many[1].diagnosis == ref['diagnosis']


def test_outlier_model_fit_comes_back_finite():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', outliers=True, warmup=60, samples=100, chains=2, random_seed=3, check_diagnostics=False,
                powerscale=True)
    res = inv.powerscale_result
    D = inv._sample_result._model.problem.D
    assert D == 2 + 81 + 4 + 2 * len(f) + 81 + 3
    assert len(res.names) == D and 'sigma_out_raw[0]' in res.names and 'sigma_out_scale[%d]' % (len(f) - 1) in res.names
    assert res.cjs2.shape == (D, 2, 2) and np.all(np.isfinite(res.cjs2)) and np.all(np.isfinite(res.prior))
    assert np.all(np.isfinite(res.pareto_k)) and np.all(res.n_tail == 40)
    _equal_results(res, inv.powerscale())
