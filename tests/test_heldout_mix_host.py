"""Held-out prediction under the outlier error models (sigma_out integrated over its prior): what needs no GPU.

  * the integration rule `loo.sigma_out_table` / `loo.sigma_out_prior_table` against closed forms and the numpy statement
    (tests/heldout_mix_numpy.py): total mass, second moment, tail sums, and the Lomax form of mode 1 against a direct quadrature of
    the exponential / inverse-gamma mixture;
  * the mixture density on that rule against a rule of a quarter the step in np.longdouble (and against mpmath's quadrature);
  * the degenerate table (y = 0, w = 1) is the plain statement, tests/heldout_numpy.py;
  * every new ValueError, and every NotImplementedError that remains, fires before the library is loaded."""
import numpy as np
import pytest

from tests import heldout_cases as hc
from tests import heldout_mix_numpy as hm
from tests import heldout_numpy as hn

# (mode, so_lambda, so_alpha, so_beta): the defaults of the two families (sampling: alpha = 5, beta = 1, lambda = 10, i.e. a Lomax
# of scale 5e-4 and an exponential of rate 200) and one other set
HYPER = [(1, 10.0, 5.0, 1.0), (2, 10.0, 5.0, 1.0), (1, 4.0, 3.0, 2.0), (2, 4.0, 3.0, 2.0)]


class _Dat:
    def __init__(self, mode, lam, alpha, beta):
        self.outlier_mode, self.so_lambda, self.so_alpha, self.so_beta = mode, lam, alpha, beta


class _FakeProblem:
    def __init__(self, Ks=(5, 4), mode=0, lam=10.0, alpha=5.0, beta=1.0):
        self.Ks, self.nf = list(Ks), 9
        self.D = 2 + 2 * sum(Ks) + 4 + 3 * len(Ks) + (2 * self.nf if mode else 0)
        self.dat = _Dat(mode, lam, alpha, beta)


class _FakeSampler:
    def __init__(self, problem, n_units=6, n_draws=10):
        self.problem, self.n_units, self.n_draws, self.handle, self._lib = problem, n_units, n_draws, None, None


# ---------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('mode,lam,alpha,beta', HYPER)
def test_table_mass_moment_and_tails(mode, lam, alpha, beta):
    from scipy.optimize import brentq
    from bayes_drt_amd import loo
    y, w, ey2, shared = loo.sigma_out_prior_table(_FakeProblem(mode=mode, lam=lam, alpha=alpha, beta=beta))
    ys, ws, ey2s, shs = hm.table(mode, lam, alpha, beta)
    assert 1 < len(y) <= 512 and y.shape == w.shape == ys.shape and shared == shs == (mode == 1)
    assert np.all(np.diff(y) > 0) and np.all(w > 0) and np.all(y > 0)
    assert np.allclose(y, ys, rtol=1e-14, atol=0) and np.allclose(w, ws, rtol=1e-13, atol=0) and ey2 == ey2s
    assert ey2 == pytest.approx(hm.second_moment(mode, lam, alpha, beta), rel=1e-15)
    mass, mom = float(np.sum(w)), float(np.sum(w * y * y))
    print('table: mode %d lambda %g alpha %g beta %g: Q = %d, sum w - 1 = %.3g, sum w y^2 / E[y^2] - 1 = %.3g'
          % (mode, lam, alpha, beta, len(y), mass - 1, mom / ey2 - 1))
    assert abs(mass - 1) <= 1e-13
    assert abs(mom / ey2 - 1) <= 1e-10
    # Tail sums against the closed-form survival.  A trapezoid sum cut at t is a rule without its end correction: it differs from
    # the integral beyond t by up to step x (y p(y) at t), whatever the step's accuracy on the whole line.  So the bound of 1e-10 is
    # taken where it can hold and where it says something about the rule, its two cut-offs: five t with y p(y) = 1e-10, 1e-12
    # and 1e-14 in the lower tail (the survival is 1 minus the mass the lower cut-off leaves out) and 1e-10, 1e-13 in the upper.
    s = hm.scale(mode, lam, alpha, beta)

    def g(u, level):
        return np.log(np.exp(u) * s * hm.density(mode, np.exp(u) * s, lam, alpha, beta)) - np.log(level)
    ts = [brentq(g, -35.9, -1.0, args=(lv,)) for lv in (1e-10, 1e-12, 1e-14)] + \
         [brentq(g, 1.0, float(np.log(y[-1] / s)), args=(lv,)) for lv in (1e-10, 1e-13)]
    for u in ts:
        t = s * np.exp(u)
        tail, want = float(np.sum(w[y > t])), float(hm.survival(mode, t, lam, alpha, beta))
        print('table: mode %d: t / s = e^%.2f: tail sum %.15g, survival %.15g, difference %.3g' % (mode, u, tail, want, tail - want))
        assert abs(tail - want) <= 1e-10


def test_table_refuses_a_plain_problem_and_bad_hyperparameters():
    from bayes_drt_amd import loo
    with pytest.raises(ValueError, match='no outlier error model'):
        loo.sigma_out_prior_table(_FakeProblem())
    with pytest.raises(ValueError, match='no outlier error model'):
        loo.sigma_out_table(0, 10.0)
    for bad in ((1, 0.0, 5.0, 1.0), (1, 10.0, -1.0, 1.0), (2, np.inf, 5.0, 1.0)):
        with pytest.raises(ValueError, match='positive finite'):
            loo.sigma_out_table(*bad)
    assert loo.sigma_out_table(1, 10.0, 1.5, 1.0)[2] == np.inf and len(loo.sigma_out_table(1, 10.0, 0.5, 1.0)[0]) <= 512


@pytest.mark.parametrize('lam,alpha,beta', [(10.0, 5.0, 1.0), (4.0, 3.0, 2.0)])
def test_mode_1_is_the_lomax_distribution(lam, alpha, beta):
    """The density the table weights come from against the model as the Stan files state it: sigma_out = 0.05 raw scale.  With
    g = 1 / scale ~ gamma(alpha, rate beta), y given g is exponential of rate lam g / 0.05."""
    from scipy.integrate import quad
    from scipy.special import gammaln
    s = hm.scale(1, lam, alpha, beta)
    for y in s * np.array([0.01, 0.3, 1.0, 5.0, 50.0]):
        def f(g):
            rate = lam * g / 0.05
            return np.exp(alpha * np.log(beta) - gammaln(alpha) + (alpha - 1) * np.log(g) - beta * g + np.log(rate) - rate * y)
        peak = alpha / (beta + lam * y / 0.05)
        got = sum(quad(f, a, b, epsabs=0, epsrel=1e-13, limit=200)[0] for a, b in ((0, peak), (peak, 8 * peak), (8 * peak, np.inf)))
        want = float(hm.density(1, y, lam, alpha, beta))
        print('lomax: y / s = %5.2f: quadrature %.15g closed form %.15g' % (y / s, got, want))
        assert abs(got / want - 1) <= 1e-10
    # and the weights are step x y p(y) of that density, halved at the ends
    yt, wt = hm.table(1, lam, alpha, beta)[:2]
    assert np.allclose(wt[1:-1], 0.125 * yt[1:-1] * hm.density(1, yt[1:-1], lam, alpha, beta), rtol=1e-12, atol=0)
    assert np.allclose(wt[[0, -1]], 0.0625 * yt[[0, -1]] * hm.density(1, yt[[0, -1]], lam, alpha, beta), rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------------- the mixture density
S_B = (0.002, 0.01, 0.05)                            # sigma_min (the smallest base scale a draw can have) and two larger
RESIDUALS = ((0.0, 1e-10), (0.003, 1e-10), (0.03, 1e-10), (0.1, 1e-10), (0.5, 1e-6))


def _density_cases():
    mu = np.zeros((len(S_B) * len(RESIDUALS), 1))
    sb = np.repeat(S_B, len(RESIDUALS))[:, None]
    e = np.tile([r for r, _ in RESIDUALS], len(S_B))
    tol = np.tile([t for _, t in RESIDUALS], len(S_B))
    return mu, sb, e, tol


@pytest.mark.skipif(not hc.LONGDOUBLE, reason='np.longdouble is no wider than float64 here')
@pytest.mark.parametrize('mode,lam,alpha,beta', HYPER)
def test_mixture_density_against_a_quarter_of_the_step(mode, lam, alpha, beta):
    from bayes_drt_amd import loo
    y, w, _, shared = loo.sigma_out_table(mode, lam, alpha, beta)
    yr, wr = hm.table(mode, lam, alpha, beta, step=0.125 / 4, dtype=np.longdouble)[:2]
    mu, sb, e, tol = _density_cases()
    worst = {}
    for i in range(len(e)):
        z = np.array([e[i]])
        got = hm.log_density(mu[i:i + 1], sb[i:i + 1], z, y, w, shared)[0]
        ref = hm.log_density(mu[i:i + 1], sb[i:i + 1], z, yr, wr, shared, dtype=np.longdouble)[0]
        rel = abs(float(np.expm1(np.longdouble(got) - ref)))
        worst[e[i]] = max(worst.get(e[i], 0.0), rel)
        assert rel <= tol[i], (mode, sb[i, 0], e[i], rel)
        if shared:                                                           # a pair under one y: the real residual and half of it
            z2 = np.array([e[i], 0.5 * e[i]])
            m2, s2 = np.zeros((1, 2)), np.array([[sb[i, 0], 1.5 * sb[i, 0]]])
            got = hm.log_density(m2, s2, z2, y, w, True)[0]
            ref = hm.log_density(m2, s2, z2, yr, wr, True, dtype=np.longdouble)[0]
            assert abs(float(np.expm1(np.longdouble(got) - ref))) <= tol[i], (mode, sb[i, 0], e[i])
    print('mixture density, mode %d alpha %g: worst relative error per residual: %s'
          % (mode, alpha, ', '.join('%g: %.2g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('mode,lam,alpha,beta', HYPER[:2])
def test_mixture_density_against_mpmath(mode, lam, alpha, beta):
    mp = pytest.importorskip('mpmath')
    from bayes_drt_amd import loo
    mp.mp.dps = 40
    y, w, _, shared = loo.sigma_out_table(mode, lam, alpha, beta)
    s = mp.mpf(hm.scale(mode, lam, alpha, beta))
    for sb in S_B:
        for e, tol in RESIDUALS:
            def f(u):                                                        # in u = ln(y / s), as the table integrates it
                t = mp.e ** u
                v = mp.mpf(sb) ** 2 + (s * t) ** 2
                p = mp.mpf(alpha) * t * (1 + t) ** -(alpha + 1) if mode == 1 else t * mp.e ** -t
                return p * mp.e ** (-mp.mpf(e) ** 2 / (2 * v)) / mp.sqrt(2 * mp.pi * v)
            want = mp.quad(f, [-60, -30, -10, -5, 0, 3, 6, 12, 30, 80] if mode == 1 else [-60, -30, -10, -5, 0, 2, 4, 7])
            got = hm.log_density(np.zeros((1, 1)), np.array([[sb]]), np.array([e]), y, w, shared)[0]
            rel = abs(float(mp.e ** (mp.mpf(float(got)) - mp.log(want)) - 1))
            assert rel <= tol, (mode, sb, e, rel)


# ---------------------------------------------------------------------------------------------------- the degenerate table
@pytest.mark.parametrize('unit', ['frequency', 'point'])
@pytest.mark.parametrize('shared', [True, False])
def test_the_degenerate_table_is_the_plain_statement(unit, shared):
    rs = np.random.default_rng(3)
    S, N2 = 67, 6
    sig = 0.01 * np.exp(0.05 * rs.standard_normal((S, N2)))
    Zh = 1.0 + 0.01 * rs.standard_normal((S, N2))
    z = 1.0 + sig[0] * np.array([0.0, 3.0, 50.0, -1.0, 0.5, -50.0])
    got = hm.reduce(Zh, sig, z, (np.zeros(1), np.ones(1), 0.0, shared), unit)
    want = hn.reduce(Zh, sig, z, unit)
    for k in ('lpd',) + hm.FIELDS:
        ulp = np.max(np.abs(got[k] - want[k]) / np.spacing(np.maximum(np.abs(want[k]), np.finfo(float).tiny)))
        assert ulp <= 4, (k, ulp)
    assert np.all(np.isfinite(got['lpd'])) and got['lpd'].min() < -750          # (50 sigma: exp() of the term itself would be 0)
    bad = sig.copy()
    bad[5, 1] = np.inf
    nan = hm.reduce(Zh, bad, z, (np.zeros(1), np.ones(1), 0.0, shared), unit)
    hit = np.zeros(N2, dtype=bool)
    hit[[1, 4] if unit == 'frequency' else [1]] = True
    assert np.array_equal(np.isnan(nan['mean']), hit) and np.array_equal(nan['pit'][~hit], got['pit'][~hit])


def test_the_moments_gain_the_second_moment_of_the_prior():
    rs = np.random.default_rng(5)
    sig, Zh, z = 0.01 + 0.001 * rs.random((40, 2)), rs.standard_normal((40, 2)) * 0.01, np.array([0.0, 0.02])
    for mode in (1, 2):
        tab = hm.table(mode, 10.0)
        got, plain = hm.reduce(Zh, sig, z, tab), hn.reduce(Zh, sig, z)
        assert np.array_equal(got['mean'], plain['mean'])
        assert np.allclose(got['sd'] ** 2, plain['sd'] ** 2 + tab[2], rtol=1e-13)
        assert np.all(got['lpd'] < plain['lpd'] + 1) and np.all((got['pit'] > 0) & (got['pit'] < 1))
    assert np.all(np.isinf(hm.reduce(Zh, sig, z, hm.table(1, 10.0, 2.0, 1.0))['sd']))


# ---------------------------------------------------------------------------------------------------- refusals without the library
@pytest.fixture
def no_library(monkeypatch):
    from bayes_drt_amd import _lib

    def refuse(*a, **k):
        raise AssertionError('the library was asked for')
    monkeypatch.setattr(_lib, 'load_library', refuse)
    monkeypatch.setattr(_lib, 'require_gpu', refuse)
    monkeypatch.setattr(_lib, '_LIB', None)


def test_device_entry_points_refuse_before_the_library_loads(no_library):
    from bayes_drt_amd import loo
    from bayes_drt_amd.engine import Sampler, sample_units
    plain, outl, H = _FakeProblem(), _FakeProblem(mode=1), 3
    f = np.array([10.0, 1.0, 0.1])
    A = [np.zeros((2 * H, 5)), np.zeros((2 * H, 4))]
    zt = np.zeros((3, 2 * H))
    par, paro = np.ones((2, plain.D)), np.ones((2, outl.D))
    # 'prior' on a plain model, and anything that is neither None nor 'prior'
    for call in (lambda so: loo.heldout_transformed(plain, par, f, A, sigma_out=so),
                 lambda so: loo.sampler_heldout(_FakeSampler(plain), 0, 6, 2, f, A, zt, sigma_out=so),
                 lambda so: loo.host_heldout(plain, np.zeros((3, 20, plain.D)), 2, f, A, zt, sigma_out=so),
                 lambda so: Sampler.heldout(_FakeSampler(plain), 0, 6, 2, f, A, zt, sigma_out=so),
                 lambda so: sample_units(plain, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt, sigma_out=so))):
        with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
            call('prior')
        for so in ('posterior', True, 1):
            with pytest.raises(ValueError, match="sigma_out must be None or 'prior'"):
                call(so)
    with pytest.raises(ValueError, match="sigma_out must be None or 'prior'"):
        loo.heldout_transformed(outl, paro, f, A, sigma_out='Prior')
    # without the keyword the outlier models are refused as before, by the old text
    for call in (lambda: loo.heldout_transformed(outl, paro, f, A), lambda: loo.sampler_heldout(_FakeSampler(outl), 0, 6, 2, f, A, zt),
                 lambda: loo.host_heldout(outl, np.zeros((3, 20, outl.D)), 2, f, A, zt),
                 lambda: loo.sampler_heldout(_FakeSampler(outl), 0, 6, 2, f, A, zt, sigma_out=None),
                 lambda: sample_units(outl, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt))):
        with pytest.raises(NotImplementedError, match='every training point has its own sigma_out and a held-out point has none'):
            call()
    # with it, the remaining argument checks still come first
    with pytest.raises(ValueError, match=r'params must be \[B, 48\]'):
        loo.heldout_transformed(outl, par, f, A, sigma_out='prior')
    with pytest.raises(ValueError, match='do not split into groups of 4'):
        loo.sampler_heldout(_FakeSampler(outl), 0, 6, 4, f, A, zt, sigma_out='prior')
    with pytest.raises(ValueError, match='at least 2 draws'):
        loo.sampler_heldout(_FakeSampler(outl, n_draws=1), 0, 6, 1, f, A, np.zeros((6, 2 * H)), sigma_out='prior')
    with pytest.raises(ValueError, match="needs part='both'"):
        sample_units(outl, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt, part='imag', sigma_out='prior'))
    # heldout_mix_reduce
    Zh, z = np.ones((2, 5, 6)), np.zeros((2, 6))
    tab = loo.sigma_out_prior_table(outl)
    for args, msg in (((Zh, Zh[:, :4], z, tab), 'do not fit'), ((Zh[:, :, :5], Zh[:, :, :5], z[:, :5], tab), 'even number'),
                      ((Zh[:, :1], Zh[:, :1], z, tab), 'at least 2 draws'), ((Zh, Zh, z, tab[:3]), 'the table must be'),
                      ((Zh, Zh, z, (tab[0], tab[1][:-1], tab[2], tab[3])), 'the table needs'),
                      ((Zh, Zh, z, (-tab[0], tab[1], tab[2], tab[3])), 'the table needs'),
                      ((Zh, Zh, z, (tab[0], tab[1], np.nan, tab[3])), 'the table needs'),
                      ((Zh, Zh, z, (np.ones(513), np.ones(513), 1.0, True)), 'the kernel holds at most 512')):
        with pytest.raises(ValueError, match=msg):
            loo.heldout_mix_reduce(*args)
    with pytest.raises(ValueError, match="unit must be 'frequency' or 'point'"):
        loo.heldout_mix_reduce(Zh, Zh, z, tab, unit='scalar')


def test_draw_limit_is_refused_on_the_host():
    from bayes_drt_amd import loo
    S = loo.max_draws() + 1
    outl = _FakeProblem(mode=2)
    with pytest.raises(ValueError, match='the kernel holds at most'):
        loo.heldout_mix_reduce(np.ones((1, S, 2)), np.ones((1, S, 2)), np.zeros((1, 2)), loo.sigma_out_prior_table(outl))
    f, A = np.array([1.0]), [np.zeros((2, 5)), np.zeros((2, 4))]
    with pytest.raises(ValueError, match='the kernel holds at most'):
        loo.sampler_heldout(_FakeSampler(outl, n_units=2, n_draws=S), 0, 2, 1, f, A, np.zeros((2, 2)), sigma_out='prior')


def test_results_carry_the_keyword_and_nothing_else():
    from bayes_drt_amd import loo
    H = 3
    p = dict(lpd=np.array([-1.0, -2.0, -3.0]), mean=np.zeros(2 * H), sd=np.ones(2 * H), pit=np.full(2 * H, 0.5))
    args = (p, np.zeros(2 * H), [3.0, 2.0, 1.0], 'both', 'frequency', 10, 2.0)
    a, b = loo.heldout_result(*args), loo.heldout_result(*args, sigma_out='prior')
    assert 'sigma_out' not in a and b['sigma_out'] == 'prior' and set(b) - set(a) == {'sigma_out'}
    assert all(np.array_equal(a[k], b[k]) for k in a)
    with pytest.raises(ValueError, match="sigma_out must be None or 'prior'"):
        loo.heldout_result(*args, sigma_out='post')
    labels = np.array([0, 1, 0, 1, 0, 1])

    def folds(so):
        out = {}
        for lab in (0, 1):
            out[lab] = loo.heldout_result(p, np.zeros(2 * H), np.array([6.0, 5.0, 4.0, 3.0, 2.0, 1.0])[labels == lab], 'both', 'frequency',
                                          10, 2.0, **so[lab])
        return out
    ka = loo.kfold_result(labels, folds([{}, {}]))
    kb = loo.kfold_result(labels, folds([dict(sigma_out='prior')] * 2))
    assert 'sigma_out' not in ka and kb['sigma_out'] == 'prior' and set(kb) - set(ka) == {'sigma_out'}
    with pytest.raises(ValueError, match='the folds differ in sigma_out'):
        loo.kfold_result(labels, folds([{}, dict(sigma_out='prior')]))
    rows = loo.compare({'plain': ka, 'outliers': kb})
    assert len(rows) == 2


def test_inverter_refuses_before_the_library_loads(no_library):
    from bayes_drt_amd.inversion import Inverter
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + 1j * 2 * np.pi * f * 1e-3)
    inv = Inverter()
    held = (f[:2], Z[:2])
    old = 'every training point has its own sigma_out and a held-out point has none'
    for call in (lambda **k: inv.fit(f[2:], Z[2:], mode='sample', heldout=held, **k),
                 lambda **k: inv.fit_many(f[2:], [Z[2:], Z[2:]], mode='sample', heldout=held, **k)):
        with pytest.raises(NotImplementedError, match=old):
            call(outliers=True)
        with pytest.raises(NotImplementedError, match=old):
            call(outliers=True, heldout_sigma_out=None)
        with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
            call(heldout_sigma_out='prior')
        with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
            call(outliers=False, heldout_sigma_out='prior')
        with pytest.raises(ValueError, match="sigma_out must be None or 'prior'"):
            call(outliers=True, heldout_sigma_out='posterior')
    with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
        inv.fit_many(f[2:], [Z[2:], Z[2:]], mode='sample', outliers=[True, False], heldout=held, heldout_sigma_out='prior')
    with pytest.raises(ValueError, match='heldout is not set'):
        inv.fit(f, Z, mode='sample', outliers=True, heldout_sigma_out='prior')
    with pytest.raises(ValueError, match="heldout needs the draws of mode='sample'"):
        inv.fit(f[2:], Z[2:], outliers=True, heldout=held, heldout_sigma_out='prior')
    # K-fold and reloo
    for call in (lambda **k: inv.kfold_many(f, [Z], folds=3, **k), lambda **k: inv.kfold(f, Z, folds=3, **k)):
        with pytest.raises(NotImplementedError, match=old):
            call(outliers=True)
        with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
            call(sigma_out='prior')
        with pytest.raises(ValueError, match="sigma_out must be None or 'prior'"):
            call(outliers=True, sigma_out='post')
        with pytest.raises(ValueError, match='is set by kfold itself'):
            call(outliers=True, sigma_out='prior', heldout_sigma_out='prior')
        with pytest.raises(ValueError, match="needs mode='sample'"):
            call(outliers=True, sigma_out='prior', mode='optimize')
    k = np.zeros(21)
    k[[4, 9, 15]] = 0.9
    inv.loo_result = __import__('bayes_drt_amd.loo', fromlist=['LooResult']).LooResult(
        elpd_i=-np.ones(21), lpd_i=-0.5 * np.ones(21), pareto_k=k, n_units=21, n_draws=100, p_waic_i=np.zeros(21))
    inv._loo_unit_part = ('frequency', 'both')
    with pytest.raises(NotImplementedError, match=old):
        inv.reloo(f, Z, outliers=True)
    with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
        inv.reloo(f, Z, sigma_out='prior')
    with pytest.raises(ValueError, match='kfold'):
        inv.reloo(f, Z, outliers=True, sigma_out='prior', max_refits=2)
    assert not hasattr(inv, 'kfold_result') and not hasattr(inv, 'heldout_result')


def test_the_multi_rank_refusal_stays(no_library, monkeypatch):
    dist = pytest.importorskip('torch.distributed')
    from bayes_drt_amd.inversion import Inverter
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + 1j * 2 * np.pi * f * 1e-3)
    inv = Inverter()
    with pytest.raises(NotImplementedError, match='process group with more than one rank'):
        inv.fit_many(f[2:], [Z[2:]], mode='sample', outliers=True, heldout=(f[:2], Z[:2]), heldout_sigma_out='prior')
    with pytest.raises(NotImplementedError, match='process group with more than one rank'):
        inv.kfold_many(f, [Z], folds=3, outliers=True, sigma_out='prior')
