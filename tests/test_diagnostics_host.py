"""HMC diagnostics without a GPU: the numpy statement (tests/diag_numpy.py) against known answers, pystan's wording, and the
flat parameter count that decides whether n_eff / Rhat are checked after sampling."""
import logging
import os

import numpy as np
import pytest

from bayes_drt_amd import diagnostics as dg
from tests import diag_numpy as dn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_iid_normal(seed):
    y = np.random.default_rng(seed).standard_normal((4, 1000))
    assert 0.85 <= dn.ess(y) / 4000 <= 1.15
    assert abs(dn.split_rhat(y) - 1) <= 0.01


@pytest.mark.parametrize('phi', [0.5, 0.9])
def test_ar1_ess(phi):
    y = dn.ar1(np.random.default_rng(7), phi, 4, 4000)
    want = y.size * (1 - phi) / (1 + phi)
    assert abs(dn.ess(y) / want - 1) <= 0.15


def test_shifted_chains_rhat():
    y = np.random.default_rng(3).standard_normal((4, 500))
    y[1] += 3.0
    assert dn.split_rhat(y) > 1.1


def test_edge_cases():
    rng = np.random.default_rng(5)
    y = rng.standard_normal((3, 201))                          # odd N: the middle draw is in no half
    n = 100
    halves = np.concatenate([y[:, :n], y[:, 101:]])
    B = n * np.var(halves.mean(axis=1), ddof=1)
    W = np.mean(np.var(halves, axis=1, ddof=1))
    assert dn.split_rhat(y) == np.sqrt((B / W + n - 1) / n)
    one = rng.standard_normal((1, 300))
    assert np.isfinite(dn.ess(one)) and np.isfinite(dn.split_rhat(one))
    assert np.isnan(dn.ess(np.full((2, 50), 1.5))) and np.isnan(dn.split_rhat(np.full((2, 50), 1.5)))
    bad = rng.standard_normal((2, 50)); bad[1, 3] = np.inf
    assert np.isnan(dn.ess(bad)) and np.isnan(dn.split_rhat(bad))
    bad[1, 3] = np.nan
    assert np.isnan(dn.ess(bad)) and np.isnan(dn.split_rhat(bad))
    assert np.isnan(dn.ess(rng.standard_normal((2, 3))))
    assert np.isfinite(dn.ess(rng.standard_normal((2, 4))))
    const = np.vstack([np.full(40, 1.0), np.full(40, 2.0)])
    assert dn.split_rhat(const) == np.inf


def test_fft_autocovariance_equals_direct_sum():
    c = np.random.default_rng(9).standard_normal(777)
    c -= c.mean()
    a, b = dn.autocovariance_fft(c), dn.autocovariance_direct(c)
    assert np.max(np.abs(a - b)) <= 1e-12 * max(1.0, abs(b[0]))


@pytest.mark.parametrize('n,total,pct', [(29, 400, '7.25'), (2, 400, '0.5'), (11, 2000, '0.55')])
def test_divergence_wording(n, total, pct):
    assert dg.divergence_message(n, total) == [
        '%d of %d iterations ended with a divergence (%s %%).' % (n, total, pct),
        'Try running with adapt_delta larger than 0.9 to remove the divergences.']


@pytest.mark.parametrize('n,total,pct', [(183, 400, '45.8'), (1936, 2000, '96.8'), (332, 400, '83')])
def test_treedepth_wording(n, total, pct):
    assert dg.treedepth_message(n, total) == [
        '%d of %d iterations saturated the maximum tree depth of 10 (%s %%)' % (n, total, pct),
        'Run again with max_treedepth larger than 10 to avoid saturation']


def test_report_logs_pystan_lines(caplog):
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        out = dg.report(np.array([500.0, 900.0]), np.array([1.0, 1.2]), 400, [20, 9], [100, 83])
    assert out == {'n_eff': True, 'Rhat': False, 'divergence': False, 'treedepth': False}
    warn = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING]
    assert warn == [dg.RHAT_MESSAGE] + dg.divergence_message(29, 400) + dg.treedepth_message(183, 400)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        out = dg.report(np.array([0.1, 900.0]), np.array([np.nan, 1.0]), 400, [0, 0], [0, 0])
    assert out == {'n_eff': False, 'Rhat': False, 'divergence': True, 'treedepth': True}
    with pytest.raises(NotImplementedError, match='Hamiltonian'):
        dg.report(None, None, 400, [0], [0], checks=['energy'])


def _dat(Nf, K, Kname='A'):
    return {Kname: np.empty((2 * Nf, K)), 'N': 2 * Nf, 'N_tilde': 2 * Nf, 'freq': np.empty(Nf)}


def test_flat_parameter_count_follows_the_model_texts():
    for K, Nf in ((81, 81), (81, 53), (41, 41), (91, 81)):
        for m in ('Series_StanModel.pkl', 'Series_pos_StanModel.pkl'):
            # parameters 2K + 9, transformed parameters 3K + 4 + 8 Nf, generated quantity Z_hat_tilde [N_tilde], lp__
            assert dg.flat_parameter_count(m, _dat(Nf, K)) == 5 * K + 13 + 8 * Nf + 2 * Nf + 1
        # Parallel: 14 Nf of transformed parameters and 8 Nf of generated quantities instead
        assert dg.flat_parameter_count('Parallel_StanModel.pkl', _dat(Nf, K)) == 5 * K + 13 + 22 * Nf + 1


def test_flat_count_lands_where_pystan_did():
    suite = np.load(os.path.join(GOLDEN, 'hmc_suite.npz'))
    nf = suite['Z'].shape[1]                                   # the 60 spectra: 81 frequencies, notebook basis K = 81
    assert dg.flat_parameter_count('Series_StanModel.pkl', _dat(nf, 81)) > dg.MAX_FLAT
    trunc = np.load(os.path.join(GOLDEN, 'kat_trunc_uniform_0.25.npz'))
    nf = len(trunc['data_freq'])                               # truncated spectra: 53 frequencies on the basis of 81
    assert nf == 53 and dg.flat_parameter_count('Series_StanModel.pkl', _dat(nf, 81)) <= dg.MAX_FLAT
    rc = np.load(os.path.join(GOLDEN, 'csv_RC-ZARC_uniform_0.25.npz'))
    nf = rc['Z'].shape[0]                                      # tutorial 0: basis_freq = freq, so K = Nf
    assert dg.flat_parameter_count('Series_pos_StanModel.pkl', _dat(nf, nf)) <= dg.MAX_FLAT
    ddt = np.load(os.path.join(GOLDEN, 'csv_BimodalTP-DDT_uniform_0.25.npz'))
    nf = ddt['Z'].shape[0]                                     # tutorial 0's DDT fit: Parallel model, K = 91
    assert dg.flat_parameter_count('Parallel_StanModel.pkl', _dat(nf, 91)) > dg.MAX_FLAT


def test_declared_order_and_saved_family():
    d = dg.declared_columns('Series_outliers_StanModel.pkl', 10, 0, [5])
    names = [n for n, _, _ in d]
    assert names[:9] == ['Rinf_raw', 'induc_raw', 'x', 'sigma_res_raw', 'alpha_prop_raw', 'alpha_re_raw', 'alpha_im_raw',
                         'sigma_out_raw', 'sigma_out_scale']
    assert dict((n, s) for n, s, _ in d)['Z_hat'] == 20
    assert dg._saved_family({'xs': 0, 'xp': 0}) == 'Series-Parallel_StanModel.pkl'


def test_column_diagnostics_checks_its_arrays_before_the_library():
    X = np.zeros((8, 3))
    with pytest.raises(ValueError, match='is_pos must have one flag per column'):
        dg.column_diagnostics(X, 2, is_pos=[1, 0])                     # the C side would read 3 flags
    with pytest.raises(ValueError, match='X must be'):
        dg.column_diagnostics(np.zeros(8), 2)
