"""Rank-normalised diagnostics without a GPU: properties of the numpy statement (tests/rank_numpy.py), the argument checks of
`rank_diagnostics` (they come before the device is asked for) and the RANK_CHECKS handling of `report`."""
import logging

import numpy as np
import pytest

from tests import diag_numpy as dn
from tests import rank_numpy as rk

SEEDS = range(20)


def _ar(seed, M=4, N=200):
    return dn.ar1(np.random.default_rng(seed), 0.3, M, N)


def test_scale_difference_is_seen_by_rank_rhat_only():
    """chain 3 with 3x the scale, 4 x 200, AR(1) 0.3, seeds 0...19: rank R-hat min 1.11, classic split R-hat max 1.03"""
    for seed in SEEDS:
        y = _ar(seed)
        y[3] *= 3.0
        assert rk.column_stats(y)['rhat'] > 1.05, seed
        assert dn.split_rhat(y) < 1.05, seed


def test_shifted_cauchy_chain_is_seen_by_rank_rhat_only():
    """standard Cauchy, chain 3 shifted by 2: rank R-hat min 1.047 (fails the 1.01 check), classic passes pystan's 1.1"""
    for seed in SEEDS:
        y = np.random.default_rng(seed).standard_cauchy((4, 200))
        y[3] += 2.0
        assert rk.column_stats(y)['rhat'] > 1.01, seed
        assert dn.split_rhat(y) < 1.1, seed


def test_rhat_and_bulk_ess_are_invariant_under_exp():
    for seed in range(5):
        y = _ar(seed)                                   # |y| < 20: exp neither overflows nor collapses two draws
        e = np.exp(y)
        assert len(np.unique(e)) == len(np.unique(y)) == y.size
        a, b = rk.column_stats(y), rk.column_stats(e)
        assert a['ess_bulk'] == b['ess_bulk']
        # the folded part ranks |Y - median|, which exp does not preserve: the unfolded R-hat is what is invariant
        assert rk.rhat_plain(rk.zscale(rk.split(y))) == rk.rhat_plain(rk.zscale(rk.split(e)))
        assert np.array_equal(rk.zscale(rk.split(y)), rk.zscale(rk.split(e)))


def test_odd_length_drops_the_middle_draw():
    y = np.arange(14.0).reshape(2, 7)
    Y = rk.split(y)
    assert Y.shape == (4, 3)
    assert np.array_equal(Y, [[0, 1, 2], [4, 5, 6], [7, 8, 9], [11, 12, 13]])
    y2 = _ar(1, 3, 101)
    z = y2.copy()
    z[:, 50] = 1e6                                      # the middle draw is never looked at
    assert rk.column_stats(y2) == rk.column_stats(z)
    y3 = np.arange(16.0).reshape(2, 8)
    assert np.array_equal(rk.split(y3), [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [12, 13, 14, 15]])


def test_nan_rules():
    y = _ar(2)
    const = np.full((4, 200), 2.5)
    assert all(np.isnan(v) for v in rk.column_stats(const).values())
    bad = y.copy()
    bad[1, 7] = np.nan
    assert all(np.isnan(v) for v in rk.column_stats(bad).values())
    bad[1, 7] = np.inf
    assert all(np.isnan(v) for v in rk.column_stats(bad).values())
    # three values, the largest in more than 5 % of the draws: q_hi is that value, 1[Y <= q_hi] is constant, ess_tail NaN
    three = np.random.default_rng(3).integers(0, 3, (4, 200)).astype(float)
    s = rk.column_stats(three)
    assert np.isnan(s['ess_tail'])
    for k in ('rhat', 'ess_bulk', 'ess_mean', 'mcse_mean', 'sd'):
        assert np.isfinite(s[k]), k
    # n = 2: ESS is NaN (fewer than 4 draws per split chain), R-hat is finite
    s = rk.column_stats(_ar(4, 4, 4))
    assert np.isfinite(s['rhat']) and np.isfinite(s['sd'])
    assert np.isnan(s['ess_bulk']) and np.isnan(s['ess_tail']) and np.isnan(s['ess_mean']) and np.isnan(s['mcse_mean'])
    assert np.isnan(rk.nan_max(np.nan, 1.0)) and np.isnan(rk.nan_min(1.0, np.nan))


def test_ess_is_capped():
    y = dn.ar1(np.random.default_rng(5), -0.6, 4, 200)          # antithetic: Geyer's estimate is several times the draws
    S = 800
    assert dn.ess(rk.split(y)) > S * np.log10(S)
    assert rk.column_stats(y)['ess_mean'] == S * np.log10(S)


def test_rank_diagnostics_argument_errors():
    from bayes_drt_amd import _lib
    from bayes_drt_amd.diagnostics import rank_diagnostics
    X = np.zeros((30, 4))
    with pytest.raises(ValueError, match='do not split'):
        rank_diagnostics(X, 4)
    for tp in ((0.0, 0.95), (0.05, 1.0), (0.5, 0.5), (0.9, 0.1), (-0.1, 0.5), (0.05,), 0.05):
        with pytest.raises(ValueError, match='tail_probs'):
            rank_diagnostics(X, 3, tail_probs=tp)
    limit = _lib.load_library().bdrt_rank_max_draws()
    assert limit >= 8192
    with pytest.raises(ValueError, match='at most %d' % limit):
        rank_diagnostics(np.zeros((2 * (limit // 2 + 2), 1)), 2)
    with pytest.raises(ValueError, match='at least 2'):
        rank_diagnostics(np.zeros((3, 2)), 3)
    with pytest.raises(ValueError, match='one flag per column'):
        rank_diagnostics(X, 3, is_pos=[1, 0])


def _report(caplog, checks, verbose=True, **kw):
    from bayes_drt_amd import diagnostics as dg
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        out = dg.report(None, None, 800, [0, 0, 0, 0], [0, 0, 0, 0], checks=checks, verbose=verbose, **kw)
    rec = [(r.levelno, r.getMessage()) for r in caplog.records if r.name == 'bayes_drt_amd']
    return out, rec


def test_report_handles_rank_checks(caplog):
    from bayes_drt_amd import diagnostics as dg
    assert dg.RANK_CHECKS == ('rank_Rhat', 'ess_bulk', 'ess_tail')
    assert dg.CHECKS == ('n_eff', 'Rhat', 'divergence', 'treedepth')
    good = dict(rank_rhat=np.array([1.0, 1.009]), ess_bulk=np.array([400.0, 900.0]), ess_tail=np.array([401.0, 2000.0]))
    out, rec = _report(caplog, list(dg.RANK_CHECKS), **good)
    assert out == {'rank_Rhat': True, 'ess_bulk': True, 'ess_tail': True}
    assert len(rec) == 3 and all(lv == logging.INFO for lv, _ in rec)
    out, rec = _report(caplog, list(dg.RANK_CHECKS), verbose=False, **good)
    assert rec == [] and all(out.values())
    # 4 chains: the ESS threshold is 400
    bad = dict(rank_rhat=np.array([1.0, 1.011]), ess_bulk=np.array([399.0, 900.0]), ess_tail=np.array([401.0, np.nan]))
    out, rec = _report(caplog, list(dg.RANK_CHECKS), **bad)
    assert out == {'rank_Rhat': False, 'ess_bulk': False, 'ess_tail': False}
    assert rec == [(logging.WARNING, dg.RANK_RHAT_MESSAGE), (logging.WARNING, dg.ESS_BULK_MESSAGE),
                   (logging.WARNING, dg.ESS_TAIL_MESSAGE)]
    out, rec = _report(caplog, ['rank_Rhat'], rank_rhat=np.array([np.nan]))
    assert out == {'rank_Rhat': False}
    out, rec = _report(caplog, ['rank_Rhat'], rank_rhat=np.array([np.inf]))
    assert out == {'rank_Rhat': False}
    out, rec = _report(caplog, ['ess_tail', 'divergence'], ess_tail=np.array([500.0]), prefix='spectrum 2: ')
    assert out == {'divergence': True, 'ess_tail': True} and all(m.startswith('spectrum 2: ') for _, m in rec)


def test_default_checks_are_what_they_were(caplog):
    from bayes_drt_amd import diagnostics as dg
    assert dg._checks_arg(None) == ['n_eff', 'Rhat', 'divergence', 'treedepth']
    with pytest.raises(NotImplementedError):
        dg._checks_arg(['rank_Rhat', 'energy'])
    with pytest.raises(ValueError):
        dg._checks_arg(['rank_rhat'])
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        out = dg.report(np.array([500.0]), np.array([1.0]), 800, [0, 0], [0, 0])
    assert list(out) == ['n_eff', 'Rhat', 'divergence', 'treedepth'] and all(out.values())
    assert [r.getMessage() for r in caplog.records] == [
        'n_eff / iter looks reasonable for all parameters', 'Rhat looks reasonable for all parameters',
        'No divergent transitions found.', 'No iterations saturated the maximum tree depth of 10.']
