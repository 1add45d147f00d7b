"""PSIS-LOO without a GPU: the numpy statement (tests/psis_numpy.py) against facts it did not produce -- the shape of known
generalised-Pareto samples and the exact leave-one-out density of a conjugate model --, and the host side of
bayes_drt_amd.loo (`compare`, units, the log-scale shift, the logged line, the ValueError paths)."""
import logging

import numpy as np
import pytest

from bayes_drt_amd import loo as L
from tests import psis_numpy as pn


def test_generalised_pareto_shape_is_recovered():
    """20 samples of 4000 genpareto draws per shape, RandomState(0) drawn in sequence; the mean k-hat of `psislw(log r)` lies
    within 0.1 of the truth.  Observed mean k-hat: -0.143, 0.106, 0.328, 0.594, 0.855 (largest miss 0.06, at k = -0.2)."""
    from scipy.stats import genpareto
    rs = np.random.RandomState(0)
    for k in (-0.2, 0.1, 0.3, 0.6, 0.9):
        est = []
        for _ in range(20):
            r = genpareto.rvs(k, size=4000, random_state=rs)
            est.append(pn.psislw(np.log(r))[1])
        print('k = %.1f: mean k-hat %.3f' % (k, np.mean(est)))
        assert abs(np.mean(est) - k) <= 0.1, (k, np.mean(est))


def _conjugate():
    """y_i ~ N(mu, 1), flat prior, n = 30, y[0] = 6 planted; S = 4000 draws of mu | y ~ N(mean y, 1 / n)."""
    from scipy.stats import genpareto
    rs = np.random.RandomState(0)
    for k in (-0.2, 0.1, 0.3, 0.6, 0.9):                                    # the generator of the test above, continued
        genpareto.rvs(k, size=20 * 4000, random_state=rs)
    n, S = 30, 4000
    y = rs.standard_normal(n)
    y[0] = 6.0
    mu = np.mean(y) + rs.standard_normal(S) / np.sqrt(n)
    ll = -0.5 * np.log(2 * np.pi) - 0.5 * (y[None, :] - mu[:, None]) ** 2
    loo_mean = (np.sum(y) - y) / (n - 1)
    v = 1.0 + 1.0 / (n - 1)
    exact = -0.5 * np.log(2 * np.pi * v) - 0.5 * (y - loo_mean) ** 2 / v
    return ll, exact


def test_exact_loo_of_a_conjugate_model():
    """elpd_i against log N(y_i | mean(y_-i), 1 + 1/(n-1)).  Observed: largest |elpd_i - exact| 0.0037 for i >= 1 and 0.024 at
    the planted point; sum p_loo 2.045 against sum p_waic 2.039; largest k 0.24, at the planted point."""
    ll, exact = _conjugate()
    r = pn.loo(ll)
    err = np.abs(r['elpd_loo'] - exact)
    print('max |elpd_i - exact|: %.4f (i >= 1), %.4f (planted); sum p_loo %.3f, sum p_waic %.3f; max k %.2f at %d'
          % (err[1:].max(), err[0], r['p_loo'].sum(), r['p_waic'].sum(), r['pareto_k'].max(), int(np.argmax(r['pareto_k']))))
    assert np.all(err[1:] <= 0.01)
    assert err[0] <= 0.05
    assert abs(r['p_loo'].sum() - r['p_waic'].sum()) <= 0.05
    assert np.all(r['pareto_k'] < 0.7)
    assert np.allclose(r['elpd_waic'], r['lpd'] - r['p_waic'], rtol=0, atol=0)


def test_statement_edge_cases():
    rng = np.random.default_rng(1)
    ll = rng.standard_normal((50, 4))
    ll[:, 0] = -1.25                                                        # constant column
    ll[3, 1] = np.nan
    ll[4, 2] = np.inf
    r = pn.loo(ll)
    assert r['pareto_k'][0] == np.inf and r['p_waic'][0] == 0.0 and r['n_tail'][0] == 0
    assert r['elpd_loo'][0] == -1.25 and r['lpd'][0] == -1.25
    for k in ('lpd', 'elpd_loo', 'pareto_k', 'p_waic'):
        assert np.isnan(r[k][1]) and np.isnan(r[k][2]) and np.isfinite(r[k][3])
    # at most 4 ratios above the cutoff: k = inf, raw weights, elpd_loo = the harmonic-mean identity
    r20 = pn.loo(rng.standard_normal((20, 2)))
    assert np.all(r20['n_tail'] <= 4) and np.all(np.isinf(r20['pareto_k']))
    col = rng.standard_normal(20)
    lw, k, nt = pn.psislw(-col)
    assert np.isinf(k) and abs(pn.logsumexp(lw)) <= 1e-14
    assert abs(pn.logsumexp(lw + col) - (np.log(20) - pn.logsumexp(-col))) <= 1e-13
    # tail length: S / 5 when the relative efficiency is small
    assert pn.tail_length(1000, 1.0) == 95 and pn.tail_length(1000, 0.05) == 200 and pn.tail_length(20) == 4
    # gpinv: the k -> 0 branch is the exponential quantile; NaN unless sigma > 0
    p = np.array([0.1, 0.5, 0.9])
    assert np.allclose(pn.gpinv(p, 0.0, 2.0), -2.0 * np.log1p(-p), rtol=1e-15)
    assert np.allclose(pn.gpinv(p, 1e-9, 2.0), -2.0 * np.log1p(-p), rtol=1e-8)
    assert np.all(np.isnan(pn.gpinv(p, 0.3, 0.0)))


def test_pointwise_log_lik_and_pairing():
    from scipy.stats import norm
    rng = np.random.default_rng(2)
    Zh, sg, z = rng.standard_normal((9, 6)), rng.uniform(0.5, 2, (9, 6)), rng.standard_normal(6)
    sg[2, 4] = 0.0
    sg[3, 1] = np.nan
    ll = pn.pointwise_log_lik(Zh, sg, z)
    ok = np.ones_like(ll, dtype=bool)
    ok[2, 4] = ok[3, 1] = False
    assert np.array_equal(np.isnan(ll), ~ok)
    assert np.allclose(ll[ok], norm.logpdf(z[None, :], Zh, np.where(ok, sg, 1.0))[ok], rtol=1e-13)
    pr = pn.pair_columns(ll)
    assert pr.shape == (9, 3) and np.array_equal(pr[0], ll[0, :3] + ll[0, 3:], equal_nan=True)


def _pointwise(elpd, lpd, k, pw):
    elpd, lpd, k, pw = [np.asarray(a, dtype=float) for a in (elpd, lpd, k, pw)]
    return {'lpd': lpd, 'elpd_loo': elpd, 'p_loo': lpd - elpd, 'pareto_k': k, 'p_waic': pw, 'elpd_waic': lpd - pw,
            'n_tail': np.full(len(k), 30, dtype=np.int32)}


def test_result_units_log_scale_and_logged_line(caplog):
    p = _pointwise([-1.0, -2.0, -4.0], [-0.9, -1.5, -3.0], [0.1, 0.75, np.inf], [0.1, 0.4, 0.9])
    f = np.array([100.0, 10.0, 1.0])
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        r0 = L._result(p, 2, 500, 0.0, f)
        r1 = L._result(p, 2, 500, np.log(3.0), f)
        rp = L._result(p, 1, 500, np.log(3.0), f)
    assert r0.elpd_loo == -7.0 and r0['n_units'] == 3 and r0.n_draws == 500 and r0.n_bad_k == 2
    assert r1.elpd_loo == r0.elpd_loo - 2 * 3 * np.log(3.0)                 # once per scalar observation, two per frequency
    assert rp.elpd_loo == r0.elpd_loo - 3 * np.log(3.0)
    assert np.array_equal(r1.elpd_i, p['elpd_loo'] - 2 * np.log(3.0)) and np.array_equal(r1.pareto_k, p['pareto_k'])
    assert r1.se == pytest.approx(r0.se, rel=1e-13) and r0.se == pytest.approx(np.sqrt(3 * np.var([-1.0, -2.0, -4.0])))
    assert r0.p_loo == pytest.approx(2.6 - 1.0) and r0.p_waic == pytest.approx(1.4)
    assert r0.elpd_waic == pytest.approx(-5.4 - 1.4)
    warn = [m.getMessage() for m in caplog.records if m.levelno == logging.WARNING and m.name == 'bayes_drt_amd']
    assert len(warn) == 3 and '2 of 3 observations have Pareto k > 0.7' in warn[0] and '10.' in warn[0] and '[1, 2]' in warn[0]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        L._result(_pointwise([-1.0, -2.0], [-0.9, -1.5], [0.1, 0.5], [0.1, 0.4]), 2, 500, 0.0, f[:2])
    assert [m.levelno for m in caplog.records if m.name == 'bayes_drt_amd'] == [logging.INFO]
    with pytest.raises(AttributeError):
        r0.no_such_entry


def test_compare_orders_and_differences():
    a = L._result(_pointwise([-1.0, -2.0, -3.0], [-0.9, -1.5, -2.5], [0.1, 0.2, 0.3], [0.1, 0.4, 0.4]), 2, 100, 0.0)
    b = L._result(_pointwise([-1.5, -1.0, -5.0], [-1.0, -0.5, -4.0], [0.1, 0.2, 0.9], [0.1, 0.4, 0.9]), 2, 100, 0.0)
    rows = L.compare({'b': b, 'a': a})
    assert [r['name'] for r in rows] == ['a', 'b']
    assert rows[0]['elpd_diff'] == 0.0 and rows[0]['dse'] == 0.0
    assert rows[1]['elpd_diff'] == pytest.approx(-1.5)
    assert rows[1]['dse'] == pytest.approx(np.sqrt(3 * np.var([-0.5, 1.0, -2.0])))
    assert rows[1]['n_bad_k'] == 1 and rows[0]['n_bad_k'] == 0 and rows[1]['p_loo'] == pytest.approx(2.0)
    c = L._result(_pointwise([-1.0, -2.0], [-0.9, -1.5], [0.1, 0.2], [0.1, 0.4]), 2, 100, 0.0)
    with pytest.raises(ValueError):
        L.compare({'a': a, 'c': c})
    assert L.compare({}) == []


def test_value_error_paths():
    from bayes_drt_amd.inversion import Inverter
    with pytest.raises(ValueError, match='unit'):
        L.pointwise_log_lik(np.zeros((4, 6)), np.ones((4, 6)), np.zeros(6), unit='declared')
    with pytest.raises(ValueError, match='do not fit'):
        L.pointwise_log_lik(np.zeros((4, 6)), np.ones((4, 5)), np.zeros(6))
    with pytest.raises(ValueError, match='even'):
        L.pointwise_log_lik(np.zeros((4, 5)), np.ones((4, 5)), np.zeros(5))
    limit = L.max_draws()
    assert limit >= 16384
    with pytest.raises(ValueError, match=str(limit)):
        L.psis_loo(np.zeros((limit + 1, 1)))
    with pytest.raises(ValueError, match='2 draws'):
        L.psis_loo(np.zeros((1, 3)))
    with pytest.raises(ValueError, match='reff'):
        L.psis_loo(np.zeros((10, 3)), reff=[1.0, 0.0, 1.0])
    with pytest.raises(ValueError, match='reff'):
        L._reff_arg('declared', None, 1)
    with pytest.raises(ValueError, match='do not fit'):
        L.loo({'Z_hat': np.zeros((8, 4)), 'sigma_tot': np.ones((8, 4))}, np.zeros(6))
    inv = Inverter()
    inv.fit_type = 'map'
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.loo()
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        Inverter.loo_many([inv])
