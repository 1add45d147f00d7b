"""Rank-normalised diagnostics on the GPU: bdrt_rank.hip against the numpy statement (tests/rank_numpy.py), the device Phi^-1
against scipy's, batch independence, the two entry points against each other, and the surface of Inverter fits
(rank_summary, the RANK_CHECKS of check_hmc_diagnostics)."""
import logging
import os
import pickle
import warnings

import numpy as np
import pytest

from tests import diag_numpy as dn
from tests import rank_numpy as rk
from tests.helpers import load

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RTOL = 1e-9
# Largest relative deviation of the kernel's z (HIP's normcdfinv) from scipy.special.ndtri((r - 3/8) / (S + 1/4)), measured on an
# MI355X over all ranks of S = 8 (2.6e-16) and S = 8000 (7.545e-16; p from 7.8e-5 to 1 - 7.8e-5), plain and folded
# (profiles/rank_diag/README.md).  The tolerance is four times that; it may never be looser than 1e-12.
Z_MEASURED = 7.6e-16
Z_TOL = 4 * Z_MEASURED
assert Z_TOL <= 1e-12


def _series(rng, M, N, C):
    X = np.empty((M, N, C))
    phis = rng.choice([0.0, 0.3, 0.7, 0.95, -0.4], size=C)
    for c in range(C):
        X[:, :, c] = dn.ar1(rng, phis[c], M, N, burn=50) * rng.uniform(0.1, 10) + rng.normal(0, 3)
    return X


# (M, N, C): smallest n with a finite ESS; odd N; n = 2 (ESS NaN, R-hat finite); sort lengths that are no power of two; 8000
# split draws next to the limit; two chains with 8192 split draws, exactly the limit
SHAPES = [(1, 8, 5), (2, 9, 6), (4, 4, 6), (3, 101, 17), (2, 64, 12), (4, 1000, 9), (8, 1000, 3), (2, 4097, 2)]
G = 2


def _inputs(M, N, C):
    rng = np.random.default_rng(M * 10007 + N * 31 + C)
    X = np.stack([_series(rng, M, N, C) for _ in range(G)])                 # [G, M, N, C]
    X[0, :, :, 0] = 2.5                                                     # constant column
    X[1, 0, 1, 1] = np.nan                                                  # non-finite draw
    X[0, :, :, 1] = rng.integers(0, 3, (M, N))                              # integers 0 ... 2: ties
    X[1, :, :, 0] = rng.standard_cauchy((M, N))                             # Cauchy
    if C > 2:
        X[1, :, :, C - 1] = np.arange(M)[:, None] * 1.0                     # constant chains at different values
    return X


def _same_kind(got, ref):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.array_equal(np.isneginf(got), np.isneginf(ref)), (got, ref)


def _assert_close(got, ref, what, tol=RTOL):
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, what
    _same_kind(got, ref)
    f = np.isfinite(ref)
    dev = np.abs(got[f] - ref[f]) / np.maximum(1e-300, np.abs(ref[f]))
    print('%s: largest relative deviation %.3g over %d values' % (what, dev.max() if dev.size else 0.0, int(f.sum())))
    assert np.all(dev <= tol), (what, float(dev.max()))


def _assert_matches_statement(got, X, probs=rk.PROBS):
    """got: dict of [G, C] arrays from the GPU; X [G, M, N, C].  The statement's Geyer sequences must not end within 1e-6 of a
    sign change (then another rounding of the lag sums could end them one pair earlier or later): asserted, not excused."""
    margin = np.array([[rk.min_margin(X[g, :, :, c], probs) for c in range(X.shape[3])] for g in range(X.shape[0])])
    print('smallest Geyer pair-sum margin: %.3g' % margin.min())
    assert margin.min() >= 1e-6
    ref = rk.diagnostics(X, probs)
    for k in rk.KEYS:
        _assert_close(got[k], ref[k], k)


@pytest.mark.parametrize('M,N,C', SHAPES)
def test_kernel_matches_numpy_statement(M, N, C):
    from bayes_drt_amd.diagnostics import rank_diagnostics
    X = _inputs(M, N, C)
    got = rank_diagnostics(X.reshape(G, M * N, C), M)
    assert set(got) == set(rk.KEYS) and all(v.shape == (G, C) for v in got.values())
    _assert_matches_statement(got, X)
    again = rank_diagnostics(X.reshape(G, M * N, C), M)
    for k in rk.KEYS:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    one = rank_diagnostics(X[1].reshape(M * N, C), M)                        # 2-D input: G = 1
    for k in rk.KEYS:
        assert one[k].shape == (C,) and np.array_equal(one[k], got[k][1], equal_nan=True), k


def _debug_z(y, what=0, is_pos=False):
    """what = 0: z of the split draws, 1: z of the folded split draws, 2: the split draws as the kernel stages them"""
    from bayes_drt_amd import _lib
    lib = _lib.require_gpu()
    y = np.ascontiguousarray(y, dtype=np.float64)
    M, N = y.shape
    z = np.empty((2 * M, N // 2))
    _lib.check(lib.bdrt_debug_rank_z(_lib.ptr(y), M, N, int(is_pos), int(what), _lib.ptr(z)), 'bdrt_debug_rank_z')
    return z


@pytest.mark.parametrize('M,N', [(1, 8), (4, 2000)])
def test_debug_z_matches_scipy_ndtri(M, N):
    y = np.random.default_rng(M + N).standard_normal((M, N))
    Y = rk.split(y)
    worst = 0.0
    for fold, ref in ((0, rk.zscale(Y)), (1, rk.zscale(np.abs(Y - np.median(Y))))):
        z = _debug_z(y, fold)
        assert z.shape == ref.shape
        dev = np.abs(z - ref) / np.abs(ref)                              # no rank of an even S maps to p = 1/2: ref != 0
        worst = max(worst, float(dev.max()))
    print('S = %d: largest relative deviation of z from scipy: %.3g' % (Y.size, worst))
    assert worst <= Z_TOL
    assert np.all(np.isnan(_debug_z(np.full((M, N), 1.5))))               # a constant column has no z
    assert np.array_equal(_debug_z(y, 2), Y)                              # the staged draws are the split chains


def test_ties_get_average_ranks():
    y = np.random.default_rng(11).integers(0, 3, (3, 40)).astype(float)
    Y = rk.split(y)
    assert np.abs(_debug_z(y, 0) - rk.zscale(Y)).max() <= Z_TOL * 4.0     # |z| < 4
    assert np.abs(_debug_z(y, 1) - rk.zscale(np.abs(Y - np.median(Y)))).max() <= Z_TOL * 4.0


def test_batch_independence():
    from bayes_drt_amd.diagnostics import rank_diagnostics
    M, N = 3, 101
    rng = np.random.default_rng(77)
    X = np.stack([_series(rng, M, N, 40) for _ in range(2)])               # [2, M, N, 40]
    col = X[0, :, :, 17]
    alone = rank_diagnostics(col.reshape(M * N, 1), M)
    batch = rank_diagnostics(X[0].reshape(M * N, 40), M)
    g0 = rank_diagnostics(X.reshape(2, M * N, 40), M)
    g1 = rank_diagnostics(X[::-1].reshape(2, M * N, 40), M)
    for k in rk.KEYS:
        assert np.isfinite(alone[k][0]), k
        assert alone[k][0] == batch[k][17] == g0[k][0, 17] == g1[k][1, 17], k


def test_tail_probabilities():
    from bayes_drt_amd.diagnostics import rank_diagnostics
    M, N, Cn = 4, 200, 6
    X = _series(np.random.default_rng(5), M, N, Cn)[None]
    probs = (0.025, 0.975)
    got = rank_diagnostics(X.reshape(1, M * N, Cn), M, tail_probs=probs)
    _assert_matches_statement(got, X, probs)
    default = rank_diagnostics(X.reshape(1, M * N, Cn), M)
    assert not np.array_equal(default['ess_tail'], got['ess_tail'])
    for k in ('rhat', 'ess_bulk', 'ess_mean', 'sd'):
        assert np.array_equal(default[k], got[k]), k


def _problem():
    from bayes_drt_amd.model import Problem
    d = np.load(os.path.join(GOLDEN, 'dat_sample_2ZARC_uniform_0.25_K81.npz'))
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=True)
    return Problem([blk], d['Z'], d['freq'], sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']),
                   ups_beta=float(d['ups_beta']))


def test_sampler_path_equals_host_path_bit_for_bit():
    from bayes_drt_amd.diagnostics import rank_diagnostics
    from bayes_drt_amd.engine import Sampler
    P = _problem()
    chains, n_draws = 3, 60
    with Sampler(P, 2 * chains, 40, n_draws, 5) as smp:
        smp.run()
        a = smp.rank_diagnostics(0, 2 * chains, chains)
        draws = smp.results()[0]
    b = rank_diagnostics(draws.reshape(2, chains * n_draws, P.D), chains, is_pos=P.is_pos)
    for k in rk.KEYS:
        assert a[k].shape == (2, P.D)
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    # The statement on the constrained draws.  The kernel ranks exp(theta) as the device computes it, which differs from
    # numpy's exp in the last bit of some draws.  That bit decides, in a few columns, whether the two middle draws tie after
    # folding about their mean (|a - med| = |b - med| up to rounding), i.e. whether the two smallest folded ranks are 1, 2 or
    # 1.5, 1.5 -- and with 30 draws per split chain that moves R-hat by up to 0.7 %.  So the statement gets the numbers the
    # kernel ranks (the debug entry returns the staged column), which numpy's are to the last bit.
    c = np.array(draws)
    for j in np.flatnonzero(P.is_pos):
        for g in range(2):
            y = draws[g * chains:(g + 1) * chains, :, j]
            c[g * chains:(g + 1) * chains, :, j] = _debug_z(y, 2, True).reshape(chains, n_draws)
    c_np = np.where(P.is_pos, np.exp(draws), draws)
    assert np.all(np.abs(c - c_np) <= 4.5e-16 * np.abs(c_np))              # both within one ulp of exp(theta)
    _assert_matches_statement(a, c.reshape(2, chains, n_draws, P.D))
    # and numpy's own constrained draws through the host path, no exp on the device
    d = rank_diagnostics(c_np.reshape(2, chains * n_draws, P.D), chains)
    _assert_matches_statement(d, c_np.reshape(2, chains, n_draws, P.D))


def _trunc():
    d = load('kat_trunc_uniform_0.25')
    return np.array(d['data_freq'], dtype=float), np.array(d['data_Z'])


BASIS = np.logspace(6, -2, 81)


def test_fit_surface(caplog):
    from bayes_drt_amd import diagnostics as dg, post
    from bayes_drt_amd.inversion import Inverter
    f, Z = _trunc()
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
            inv.fit(f, Z, mode='sample', warmup=60, samples=40, chains=2, random_seed=3)
    auto = [(r.levelno, r.getMessage()) for r in caplog.records if r.name == 'bayes_drt_amd']
    fit = inv._sample_result
    # the automatic check logged pystan's four lines from pystan's values, as before: nothing of the rank family
    hc = fit.hmc_check
    assert set(hc) == {'n_eff', 'Rhat', 'divergence', 'treedepth', 'n_eff_values', 'Rhat_values'}
    total = fit.chains * fit.n_draws
    want = [(logging.INFO, 'n_eff / iter looks reasonable for all parameters') if hc['n_eff'] else (logging.WARNING, dg.NEFF_MESSAGE),
            (logging.INFO, 'Rhat looks reasonable for all parameters') if hc['Rhat'] else (logging.WARNING, dg.RHAT_MESSAGE)]
    want += ([(logging.INFO, 'No divergent transitions found.')] if hc['divergence'] else
             [(logging.WARNING, m) for m in dg.divergence_message(fit.n_divergent, total, 0.9)])
    want += ([(logging.INFO, 'No iterations saturated the maximum tree depth of 10.')] if hc['treedepth'] else
             [(logging.WARNING, m) for m in dg.treedepth_message(fit.n_max_treedepth, total, 10)])
    assert auto == want
    s, r = fit.summary(), fit.rank_summary()
    assert list(r['summary_rownames']) == list(s['summary_rownames'])
    assert r['summary_colnames'] == ('mean', 'mcse_mean', 'sd', '5%', '50%', '95%', 'ess_bulk', 'ess_tail', 'Rhat')
    assert set(r) == {'summary', 'summary_rownames', 'summary_colnames'}
    T = r['summary']
    assert T.shape == (len(s['summary_rownames']), 9)
    names, X = dg._stacked_columns(fit, None, 'test')
    assert np.array_equal(T[:, 3:6], post.percentile(X, [5.0, 50.0, 95.0], axis=0).T)
    assert np.array_equal(T[:, 0], s['summary'][:, 0], equal_nan=True)
    Sp = 2 * fit.chains * (fit.n_draws // 2)
    for j in (6, 7):
        e = T[:, j]
        assert np.all(e[np.isfinite(e)] <= Sp * np.log10(Sp)) and np.isfinite(e).sum() > 0.9 * len(e)
    d = dg.rank_diagnostics(X, fit.chains)
    for j, k in ((1, 'mcse_mean'), (2, 'sd'), (6, 'ess_bulk'), (7, 'ess_tail'), (8, 'Rhat')):
        assert np.array_equal(T[:, j], d['rhat' if k == 'Rhat' else k], equal_nan=True), k
    few = fit.rank_summary(pars=['Rinf', 'x'], probs=(0.5,), tail_probs=(0.025, 0.975))
    assert few['summary'].shape == (82, 7) and few['summary_colnames'][3] == '50%'
    with pytest.raises(ValueError):
        fit.rank_summary(pars=['no_such_parameter'])
    # a fit restored from its stored arrays gives the same bits on the rows it covers
    saved = pickle.loads(pickle.dumps(fit.to_saved()))
    r2 = saved.rank_summary()
    live = dict(zip(r['summary_rownames'], T))
    rows = list(r2['summary_rownames'])
    assert rows[-1] == 'lp__' and 'x[0]' in rows and r2['summary_colnames'] == r['summary_colnames']
    assert np.array_equal(np.array([live[n] for n in rows]), r2['summary'], equal_nan=True)
    # the checks on request
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        res = dg.check_hmc_diagnostics(fit, checks=['rank_Rhat', 'ess_bulk', 'ess_tail'])
    assert list(res) == ['rank_Rhat', 'ess_bulk', 'ess_tail']
    rec = [(x.levelno, x.getMessage()) for x in caplog.records if x.name == 'bayes_drt_amd']
    assert len(rec) == 3
    assert res['rank_Rhat'] == (not np.any(np.isnan(T[:, 8]) | (T[:, 8] > 1.01)))
    assert res['ess_bulk'] == (not np.any(np.isnan(T[:, 6]) | (T[:, 6] < 200.0)))
    assert res['ess_tail'] == (not np.any(np.isnan(T[:, 7]) | (T[:, 7] < 200.0)))
    for ok, (lv, msg), bad in zip(res.values(), rec, (dg.RANK_RHAT_MESSAGE, dg.ESS_BULK_MESSAGE, dg.ESS_TAIL_MESSAGE)):
        assert (lv == logging.INFO) if ok else (lv, msg) == (logging.WARNING, bad)
    both = dg.check_hmc_diagnostics(fit, verbose=False, checks=['Rhat', 'rank_Rhat'])
    assert list(both) == ['Rhat', 'rank_Rhat'] and both['Rhat'] == hc['Rhat']
    assert set(dg.check_hmc_diagnostics(fit, verbose=False)) == {'n_eff', 'Rhat', 'divergence', 'treedepth'}
