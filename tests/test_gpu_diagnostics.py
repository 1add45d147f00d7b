"""HMC diagnostics on the GPU: bdrt_diag.hip against the numpy statement (tests/diag_numpy.py), the two entry points against
each other, and the pystan-style surface of Inverter fits (summary, automatic check after sampling)."""
import logging
import os
import warnings

import numpy as np
import pytest

from tests import diag_numpy as dn
from tests.helpers import load

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _series(rng, M, N, C):
    X = np.empty((M, N, C))
    phis = rng.choice([0.0, 0.3, 0.7, 0.95, -0.4], size=C)
    for c in range(C):
        X[:, :, c] = dn.ar1(rng, phis[c], M, N, burn=50) * rng.uniform(0.1, 10) + rng.normal(0, 3)
    return X


# (M, N, C): LDS-resident tiles of 8, 1 and several columns; streamed (M * N * 8 B > 64 KiB) sizes
SHAPES = [(1, 200, 900), (2, 5, 40), (4, 4, 30), (8, 1000, 24), (8, 4001, 6), (4, 4001, 10), (2, 1000, 300), (8, 200, 100)]


@pytest.mark.parametrize('M,N,C', SHAPES)
def test_kernel_matches_numpy_statement(M, N, C):
    from bayes_drt_amd.diagnostics import column_diagnostics
    rng = np.random.default_rng(M * 10007 + N * 31 + C)
    G = 2
    X = np.stack([_series(rng, M, N, C) for _ in range(G)])                 # [G, M, N, C]
    X[0, :, :, 0] = 2.5                                                     # constant column
    X[1, 0, 1, 1] = np.nan                                                  # non-finite draw
    if C > 2 and N >= 4:
        X[1, :, :, 2] = np.arange(M)[:, None] * 1.0                         # constant chains at different values
    mean, sd, ne, rh = column_diagnostics(X.reshape(G, M * N, C), M)
    rm, rs, rn, rr = dn.diagnostics(X)
    for got, ref, tol in ((mean, rm, 1e-12), (sd, rs, 1e-12), (rh, rr, 1e-9)):
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.isinf(got), np.isinf(ref))
        f = np.isfinite(ref)
        assert np.all(np.abs(got[f] - ref[f]) <= tol * np.maximum(1e-300, np.abs(ref[f]))), np.max(np.abs(got[f] / ref[f] - 1))
    assert np.array_equal(np.isnan(ne), np.isnan(rn))
    f = np.isfinite(rn)
    off = f & ~(np.abs(ne - rn) <= 1e-9 * np.abs(rn))
    # the one exception: a Geyer pair sum within 1e-10 var_plus of 0 may end the sequence one pair earlier or later
    margin = np.array([[dn.ess_and_margin(X[g, :, :, c])[1] for c in range(C)] for g in range(G)])
    print('n_eff columns truncated differently: %d of %d (pair sum near 0 in %d)'
          % (int(off.sum()), int(f.sum()), int((f & (margin < 1e-10)).sum())))
    assert np.all(margin[off] < 1e-10), (ne[off], rn[off], margin[off])
    again = column_diagnostics(X.reshape(G, M * N, C), M)
    for a, b in zip(again, (mean, sd, ne, rh)):
        assert np.array_equal(a, b, equal_nan=True)


def _problem():
    from bayes_drt_amd.model import Problem
    d = np.load(os.path.join(GOLDEN, 'dat_sample_2ZARC_uniform_0.25_K81.npz'))
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=True)
    return Problem([blk], d['Z'], d['freq'], sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']),
                   ups_beta=float(d['ups_beta']))


def test_sampler_path_equals_host_path_bit_for_bit():
    from bayes_drt_amd.diagnostics import column_diagnostics
    from bayes_drt_amd.engine import Sampler
    P = _problem()
    chains, n_draws = 3, 60
    with Sampler(P, 2 * chains, 40, n_draws, 5) as smp:
        smp.run()
        a = smp.diagnostics(0, 2 * chains, chains)
        a2 = smp.diagnostics(0, 2 * chains, chains)
        draws = smp.results()[0]
    b = column_diagnostics(draws.reshape(2, chains * n_draws, P.D), chains, is_pos=P.is_pos)
    for x, y, z in zip(a, a2, b):
        assert x.shape == (2, P.D)
        assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x, z, equal_nan=True)
    c = np.exp(draws) * P.is_pos + draws * ~P.is_pos
    ref = dn.diagnostics(c.reshape(2, chains, n_draws, P.D))
    assert np.allclose(b[3], ref[3], rtol=1e-9, equal_nan=True)


def _trunc():
    d = load('kat_trunc_uniform_0.25')
    return np.array(d['data_freq'], dtype=float), np.array(d['data_Z'])


BASIS = np.logspace(6, -2, 81)


def test_fit_summary_and_automatic_check(caplog, tmp_path):
    from bayes_drt_amd import diagnostics as dg, post
    from bayes_drt_amd.inversion import Inverter
    f, Z = _trunc()
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
            inv.fit(f, Z, mode='sample', warmup=60, samples=40, chains=2, random_seed=3)
    fit = inv._sample_result
    s = fit.summary()
    flat = dg.flat_parameter_count(inv.stan_model_name, inv._stan_input)
    assert flat <= dg.MAX_FLAT
    assert s['summary'].shape == (flat, 10) and len(s['summary_rownames']) == flat
    assert s['summary_colnames'] == ('mean', 'se_mean', 'sd', '2.5%', '25%', '50%', '75%', '97.5%', 'n_eff', 'Rhat')
    assert s['c_summary'].shape == (flat, 7, 2)
    rn = list(s['summary_rownames'])
    assert rn[:3] == ['Rinf_raw', 'induc_raw', 'x[0]'] and rn[-1] == 'lp__'
    ix = [rn.index('x[%d]' % i) for i in range(81)]
    assert np.array_equal(s['summary'][ix, 7], post.percentile(fit['x'], 97.5, axis=0))
    assert np.array_equal(inv._rescale_coef(s['summary'][ix, 7], 'series'), inv.coef_percentile('DRT', 97.5))
    assert np.allclose(s['summary'][ix, 0], np.mean(fit['x'], axis=0), rtol=1e-12, atol=0)
    iz = [rn.index('Z_hat[%d]' % i) for i in range(2 * len(f))]
    assert np.array_equal(s['summary'][iz, 3], post.percentile(fit['Z_hat'], 2.5, axis=0))
    # the automatic check ran the same reduction and logged from it
    assert np.array_equal(fit.hmc_check['Rhat_values'], s['summary'][:, -1], equal_nan=True)
    warn = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and r.name == 'bayes_drt_amd']
    assert (dg.RHAT_MESSAGE in warn) == (not fit.hmc_check['Rhat'])
    assert isinstance(fit.stansummary(pars=['Rinf', 'x']), str)
    # save -> load -> summary: the stored arrays give the same numbers on the rows they cover
    fn = str(tmp_path / 'fit.pkl')
    inv.save_fit_data(fn)
    inv2 = Inverter(basis_freq=BASIS)
    inv2.load_fit_data(fn)
    s2 = inv2._sample_result.summary()
    rows = list(s2['summary_rownames'])
    assert 'q[0]' not in rows and 'dups[0]' in rows and 'Z_hat_im[0]' in rows and rows[-1] == 'lp__'
    live = dict(zip(rn, s['summary']))
    assert np.array_equal(np.array([live[r] for r in rows]), s2['summary'], equal_nan=True)


def test_treedepth_line_and_switch(caplog):
    from bayes_drt_amd import diagnostics as dg
    from bayes_drt_amd.inversion import Inverter
    f, Z = _trunc()
    inv = Inverter(basis_freq=BASIS)
    inv._NUTS_CONTROL = dict(adapt_delta=0.9, adapt_t0=10, max_treedepth=2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        with caplog.at_level(logging.DEBUG, logger='bayes_drt_amd'):
            inv.fit(f, Z, mode='sample', warmup=40, samples=50, chains=2, random_seed=4)
        fit = inv._sample_result
        warn = [r.getMessage() for r in caplog.records if r.levelno >= logging.WARNING and r.name == 'bayes_drt_amd']
        assert fit.n_max_treedepth > 0
        for line in dg.treedepth_message(fit.n_max_treedepth, 100, 2):
            assert line in warn
        caplog.clear()
        with caplog.at_level(logging.DEBUG, logger='bayes_drt_amd'):
            inv.fit(f, Z, mode='sample', warmup=40, samples=50, chains=2, random_seed=4, check_diagnostics=False)
        assert [r for r in caplog.records if r.name == 'bayes_drt_amd'] == []
    with pytest.raises(NotImplementedError):
        dg.check_hmc_diagnostics(fit, checks=['energy'])
    res = dg.check_hmc_diagnostics(fit, verbose=False)
    assert set(res) == {'n_eff', 'Rhat', 'divergence', 'treedepth'} and res['treedepth'] is False


def test_fit_many_diagnostics_equal_separate_fits():
    from bayes_drt_amd.inversion import Inverter
    names = ['trunc_uniform_0.25', 'trunc_Orazem_1.0', 'trunc_Macdonald_2.5']
    fs, zs = [], []
    for n in names:
        d = load('kat_' + n)
        fs.append(np.array(d['data_freq'], dtype=float)); zs.append(np.array(d['data_Z']))
    kw = dict(mode='sample', warmup=40, samples=30, chains=2, random_seed=8)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = Inverter(basis_freq=BASIS).fit_many(fs[0], zs, **kw)
        for Z, v in zip(zs, views):
            one = Inverter(basis_freq=BASIS)
            one.fit(fs[0], Z, **kw)
            a, b = v._sample_result.hmc_check, one._sample_result.hmc_check
            assert {k: a[k] for k in ('n_eff', 'Rhat', 'divergence', 'treedepth')} == \
                {k: b[k] for k in ('n_eff', 'Rhat', 'divergence', 'treedepth')}
            # parameters: exp on the device (sampler path) against numpy's exp (host path): last-bit differences only
            assert np.allclose(a['n_eff_values'], b['n_eff_values'], rtol=1e-9, equal_nan=True)
            assert np.allclose(a['Rhat_values'], b['Rhat_values'], rtol=1e-9, equal_nan=True)
