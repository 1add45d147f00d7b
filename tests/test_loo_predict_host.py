"""PSIS-LOO predictive checks without a GPU: the numpy statement (tests/loo_predict_numpy.py) against a case with a known
answer and its stated conventions, the Kolmogorov-Smirnov pair of bayes_drt_amd.loo against scipy, and the argument validation
of the Python layer, which raises before anything is launched."""
import numpy as np
import pytest
from scipy import stats
from scipy.special import erfc

from tests import loo_predict_numpy as lp


def test_statement_recovers_the_conjugate_leave_one_out_predictive():
    """y_i ~ normal(theta, 1) with a flat prior: theta | y ~ normal(ybar, 1 / n), and the LOO predictive of y_i is
    normal(ybar_-i, 1 + 1 / (n - 1)) exactly.  Bounds: about three times the spread of the PSIS estimate at S = 4000 over 20
    replications x 12 observations (worst: mean 0.034, sd 0.0083, pit 0.0040, k-hat at most 0.50)."""
    rng = np.random.default_rng(1)
    n, S = 12, 4000
    y = rng.standard_normal(n) + 0.3
    y[4] += 3.0
    th = y.mean() + rng.standard_normal(S) / np.sqrt(n)
    dev = np.zeros(3)
    for i in range(n):
        u = lp.predict_unit(th[:, None], np.ones((S, 1)), y[i:i + 1])
        m = np.delete(y, i).mean()
        s = np.sqrt(1.0 + 1.0 / (n - 1))
        pit = 0.5 * erfc((m - y[i]) / (s * np.sqrt(2.0)))
        d = np.abs([u['mean'][0] - m, u['sd'][0] - s, u['pit'][0] - pit])
        dev = np.maximum(dev, d)
        assert d[0] <= 0.1 and d[1] <= 0.03 and d[2] <= 0.02, (i, d, u['pareto_k'])
        assert u['pareto_k'] < 0.7
        # the in-sample predictive is normal(ybar, 1 + 1 / n): the outlier pulls it towards itself, the LOO one not
        assert abs(u['mean_post'][0] - y.mean()) <= 0.02 and abs(u['sd_post'][0] - np.sqrt(1 + 1 / n)) <= 0.01
    print('conjugate case: largest deviation mean %.3g, sd %.3g, pit %.3g' % tuple(dev))


def _ties():
    l = np.linspace(0.1, 2, 20)
    return np.concatenate((1 + l, 1 - l))


def test_statement_orders_ties_by_draw_index():
    """20 symmetric pairs of draws with equal log-likelihood and different mu: the stable order of the tail decides which
    of a pair gets the larger smoothed weight, so the result depends on the order of the draws."""
    mu = _ties()
    fwd = lp.predict_unit(mu[:, None], np.ones((40, 1)), [1.0])
    rev = lp.predict_unit(mu[::-1][:, None], np.ones((40, 1)), [1.0])
    assert fwd['mean'][0] == pytest.approx(0.97687, abs=1e-5) and fwd['pit'][0] == pytest.approx(0.50569, abs=1e-5)
    assert rev['mean'][0] == pytest.approx(1.01572, abs=1e-5) and rev['pit'][0] == pytest.approx(0.49606, abs=1e-5)
    for u in (fwd, rev):
        assert u['pareto_k'] == pytest.approx(-0.0350475, abs=1e-5) and u['n_tail'] == 8
    assert fwd['mean_post'][0] == pytest.approx(1.0, abs=1e-14) and fwd['pit_post'][0] == pytest.approx(0.5, abs=1e-14)


def test_statement_degenerate_units():
    S = 30
    rng = np.random.default_rng(2)
    sg = np.full((S, 2), 0.5)
    # all log-likelihoods equal, the draws not: equal weights, the LOO figures are the in-sample ones
    mu = np.stack((np.where(np.arange(S) % 2, 1.25, 0.75), np.full(S, 2.0)), axis=1)
    u = lp.predict_unit(mu, sg, [1.0, 2.5])
    assert u['pareto_k'] == np.inf and u['n_tail'] == 0
    for k in ('mean', 'sd', 'pit'):
        assert np.allclose(u[k], u[k + '_post'], rtol=1e-14, atol=0)
    assert u['mean'] == pytest.approx([1.0, 2.0], abs=1e-14)
    assert u['sd'] == pytest.approx([np.sqrt(0.25 + 0.0625), 0.5], abs=1e-14)
    # a non-finite log-likelihood anywhere: every output of the unit NaN, n_tail 0 -- both scalars of a pair
    mu = rng.standard_normal((S, 2))
    for bad in (0.0, -1.0, np.inf, np.nan):
        s2 = sg.copy()
        s2[7, 1] = bad
        u = lp.predict_unit(mu, s2, [0.1, 0.2])
        assert all(np.all(np.isnan(u[k])) and u[k].shape == (2,) for k in lp.FIELDS)
        assert np.isnan(u['pareto_k']) and u['n_tail'] == 0
    m2 = mu.copy()
    m2[3, 0] = np.nan
    assert np.all(np.isnan(lp.predict_unit(m2, sg, [0.1, 0.2])['mean']))
    # as points, only the scalar with the bad sigma is lost
    s2 = sg.copy()
    s2[7, 1] = 0.0
    p = lp.predict(mu, s2, np.array([0.1, 0.2]), unit='point')
    assert np.isfinite(p['mean'][0]) and np.isnan(p['mean'][1]) and p['n_tail'][1] == 0
    f = lp.predict(mu, s2, np.array([0.1, 0.2]), unit='frequency')
    assert np.all(np.isnan(f['mean'])) and f['pareto_k'].shape == (1,)


@pytest.mark.parametrize('n,kind', [(1, 'uniform'), (7, 'uniform'), (81, 'uniform'), (162, 'skewed'), (500, 'tight'), (40, 'nan')])
def test_ks_pair_matches_scipy(n, kind):
    from bayes_drt_amd import loo as L
    rng = np.random.default_rng(n)
    p = rng.uniform(size=n)
    if kind == 'skewed':
        p = p ** 1.3
    elif kind == 'tight':                                                    # an error model that is too wide: PIT piles up at 1/2
        p = 0.5 + 0.2 * (p - 0.5)
    fin = p.copy()
    if kind == 'nan':
        p[[3, 11]] = np.nan
        fin = p[np.isfinite(p)]
    D, pv = L.ks_uniform(p)
    ref = stats.kstest(fin, 'uniform', method='asymp')
    assert D == pytest.approx(ref.statistic, abs=1e-15)
    assert pv == pytest.approx(ref.pvalue, abs=1e-6)
    assert 0.0 <= pv <= 1.0


def test_ks_pair_without_a_finite_value():
    from bayes_drt_amd import loo as L
    D, pv = L.ks_uniform(np.array([np.nan, np.nan]))
    assert np.isnan(D) and np.isnan(pv)


def test_python_layer_validates_before_launching(monkeypatch):
    from bayes_drt_amd import loo as L
    S, Nf = 8, 3
    Zh, sg, z = np.zeros((S, 2 * Nf)), np.ones((S, 2 * Nf)), np.zeros(2 * Nf)
    with pytest.raises(ValueError, match='do not fit'):
        L.psis_predict(Zh, sg[:, :5], z)
    with pytest.raises(ValueError, match='do not fit'):
        L.psis_predict(Zh, sg, z[:5])
    with pytest.raises(ValueError, match='do not fit'):
        L.psis_predict(Zh[None], sg[None], z)                               # [G, S, N] needs z [G, N]
    with pytest.raises(ValueError, match='unit must be'):
        L.psis_predict(Zh, sg, z, unit='pair')
    with pytest.raises(ValueError, match='even number'):
        L.psis_predict(Zh[:, :5], sg[:, :5], z[:5])
    with pytest.raises(ValueError, match='at least 2 draws'):
        L.psis_predict(Zh[:1], sg[:1], z)
    for bad in (0.0, -0.5, np.nan, np.inf):
        with pytest.raises(ValueError, match='reff must be positive'):
            L.psis_predict(Zh, sg, z, reff=bad)
    with pytest.raises(ValueError):
        L.psis_predict(Zh, sg, z, reff=np.ones(Nf + 1))                     # does not broadcast to the units
    monkeypatch.setattr(L, 'predict_max_draws', lambda: 7)
    with pytest.raises(ValueError, match='at most 7'):
        L.psis_predict(Zh, sg, z)
    monkeypatch.undo()
    assert L.predict_max_draws() >= 8192                                    # (the library answers without a GPU)
    fit = {'Z_hat': Zh, 'sigma_tot': sg}
    with pytest.raises(ValueError, match='do not fit'):
        L.loo_predict(fit, z[:5])
    with pytest.raises(ValueError, match='unit must be'):
        L.loo_predict(fit, z, unit='pair')
    with pytest.raises(ValueError, match="reff must be 'auto'"):
        L.loo_predict(fit, z, reff='mcmc')
    with pytest.raises(ValueError, match='unit must be'):
        L.loo_predict_many([fit], [z], unit='pair')


def test_result_is_a_dict_with_attribute_access():
    from bayes_drt_amd import loo as L
    r = L.LooPredictResult(pit=np.array([0.5]), n_bad_k=0)
    assert r.pit is r['pit'] and r.n_bad_k == 0 and isinstance(r, dict)
    with pytest.raises(AttributeError):
        r.missing
