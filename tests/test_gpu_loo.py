"""PSIS-LOO on the GPU: bdrt_loo.hip against the numpy statement (tests/psis_numpy.py) on identical input, batch independence,
and the surface of Inverter fits (`loo`, `loo_many`, save / load).

Tolerances.  NaN / inf patterns and n_tail: equal exactly.  lpd, p_waic: relative 1e-12 (what test_gpu_diagnostics.py uses for
means and sd).  elpd_loo, pareto_k: 100 x the largest deviation measured on these inputs on the MI355X
(profiles/loo/parity.txt), so that another fixed summation order in a later kernel does not break the test; never looser than
1e-8 absolute, which is a condition on the kernel and not a measurement."""
import functools
import logging
import warnings

import numpy as np
import pytest

from tests import psis_numpy as pn
from tests.helpers import load

pytestmark = pytest.mark.gpu

# measured on the MI355X (profiles/loo/parity.txt): largest |kernel - numpy statement| over all shapes below
MEASURED_ELPD, MEASURED_K = 1.1e-14, 9.0e-15
TOL_ELPD = min(100 * MEASURED_ELPD, 1e-8)
TOL_K = min(100 * MEASURED_K, 1e-8)


# ---------------------------------------------------------------------------------------------------- pointwise log-likelihood
@pytest.mark.parametrize('unit', ['point', 'frequency'])
@pytest.mark.parametrize('G,S,Nf', [(1, 37, 7), (3, 1000, 21), (2, 513, 5)])
def test_pointwise_loglik_matches_numpy_statement(G, S, Nf, unit):
    """Relative tolerance 1e-13 was enough: the device log agrees with the host's to the last bit or two, and sigma is of the size
    of a scaled impedance error (1e-4 ... 1e-3), so no log-likelihood is a difference of nearly equal terms."""
    from bayes_drt_amd.loo import pointwise_log_lik
    rng = np.random.default_rng(S * 131 + Nf)
    N2 = 2 * Nf
    z = rng.standard_normal((G, N2))
    sig = np.exp(rng.uniform(np.log(1e-4), np.log(1e-3), (G, S, N2)))
    Zhat = z[:, None, :] + sig * rng.standard_normal((G, S, N2))
    g0, s0, c0 = G - 1, S // 3, Nf + 2
    sig[g0, s0, c0] = -0.3 if unit == 'point' else 0.0                      # non-positive sigma: NaN there only
    got = pointwise_log_lik(Zhat, sig, z, unit=unit)
    ref = np.stack([pn.pointwise_log_lik(Zhat[g], sig[g], z[g]) for g in range(G)])
    bad = np.zeros(ref.shape, dtype=bool)
    bad[g0, s0, c0] = True
    if unit == 'frequency':
        ref = ref[:, :, :Nf] + ref[:, :, Nf:]
        bad = bad[:, :, :Nf] | bad[:, :, Nf:]
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(ref), bad) and np.array_equal(np.isnan(got), bad)
    rel = np.abs(got[~bad] - ref[~bad]) / np.abs(ref[~bad])
    print('pointwise log-likelihood %s: largest relative deviation %.3g' % ((G, S, Nf, unit), rel.max()))
    assert rel.max() <= 1e-13
    one = pointwise_log_lik(Zhat[0], sig[0], z[0], unit=unit)               # 2-D input: G = 1
    assert np.array_equal(one, got[0], equal_nan=True)


# ---------------------------------------------------------------------------------------------------- PSIS-LOO columns
SHAPES = [(20, 3), (37, 5), (1000, 7), (4000, 4), (4097, 3), (16384, 2)]
SPECIAL = {(20, 3): ('const', 'nan', 'big', 'reff'), (37, 5): ('const', 'inf', 'big', 'low', 'reff'),
           (1000, 7): ('const', 'nan', 'big', 'low', 'reff'), (4000, 4): ('const', 'inf', 'big', 'low', 'reff'),
           (4097, 3): ('reff', 'low', 'big', 'nan'), (16384, 2): ('reff', 'big')}


@functools.lru_cache(maxsize=None)
def _case(S, N):
    """ll [2, S, N], reff [2, N], the numpy statement's results and where the special columns are.  Log ratios -ll are
    Student-t draws of 3 ... 30 degrees of freedom times 0.05 ... 2.5, so k-hat spans about -0.2 ... 1 and beyond."""
    rng = np.random.default_rng(S * 17 + N)
    G = 2
    ll = np.empty((G, S, N))
    for g in range(G):
        for i in range(N):
            ll[g, :, i] = -rng.uniform(0.05, 2.5) * rng.standard_t(rng.choice([3, 5, 10, 30]), S) + rng.uniform(2, 9)
    reff = np.ones((G, N))
    where = {}
    flat = [(g, i) for i in range(N) for g in range(G)]                     # specials alternate between the groups
    for kind, (g, i) in zip(SPECIAL[(S, N)], flat[1:]):
        where[kind] = (g, i)
        if kind == 'const':
            ll[g, :, i] = 3.75
        elif kind == 'nan':
            ll[g, S // 2, i] = np.nan
        elif kind == 'inf':
            ll[g, S // 2, i] = np.inf
        elif kind == 'big':                                                 # one ratio below log(DBL_MIN) after the shift
            ll[g, S // 3, i] = ll[g, :, i].min() + 800.0
        elif kind == 'low':                                                 # all but one below it: the cutoff is the floor
            ll[g, S // 3, i] = ll[g, :, i].min() - 800.0
        elif kind == 'reff':                                                # tail length S / 5 (where 3 sqrt(20 S) exceeds it)
            reff[g, i] = 0.05
    ref = [pn.loo(ll[g], reff[g]) for g in range(G)]
    ref = {k: np.stack([r[k] for r in ref]) for k in ref[0]}
    for a in (ll, reff) + tuple(ref.values()):
        a.setflags(write=False)
    return ll, reff, ref, where


def _same_pattern(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and \
        np.array_equal(np.isneginf(got), np.isneginf(ref))


@pytest.mark.parametrize('S,N', SHAPES)
def test_psis_loo_matches_numpy_statement(S, N):
    from bayes_drt_amd.loo import psis_loo
    ll, reff, ref, where = _case(S, N)
    got = psis_loo(ll, reff)
    fin = np.isfinite(ref['pareto_k'])
    print('(S, N) = %s: n_tail %d ... %d, k-hat %.2f ... %.2f, specials %s' % (
        (S, N), ref['n_tail'].min(), ref['n_tail'].max(), ref['pareto_k'][fin].min() if fin.any() else np.nan,
        ref['pareto_k'][fin].max() if fin.any() else np.nan, where))
    dev = {}
    for k in ('lpd', 'p_waic', 'elpd_loo', 'pareto_k'):
        assert _same_pattern(got[k], ref[k]), (k, got[k], ref[k])
        f = np.isfinite(ref[k])
        d = np.abs(got[k][f] - ref[k][f])
        dev[k] = (d.max(), (d / np.maximum(np.abs(ref[k][f]), 1e-300)).max()) if f.any() else (0.0, 0.0)
    print('  largest deviation abs (rel): ' + ', '.join('%s %.3g (%.3g)' % (k, v[0], v[1]) for k, v in dev.items()))
    assert np.array_equal(got['n_tail'], ref['n_tail']), (got['n_tail'], ref['n_tail'])
    for k in ('lpd', 'p_waic'):
        f = np.isfinite(ref[k])
        assert np.all(np.abs(got[k][f] - ref[k][f]) <= 1e-12 * np.abs(ref[k][f])), (k, dev[k])
    assert dev['elpd_loo'][0] <= TOL_ELPD and dev['pareto_k'][0] <= TOL_K, dev
    assert np.array_equal(got['p_loo'], got['lpd'] - got['elpd_loo'], equal_nan=True)
    assert np.array_equal(got['elpd_waic'], got['lpd'] - got['p_waic'], equal_nan=True)
    if 'const' in where:
        g, i = where['const']
        assert got['pareto_k'][g, i] == np.inf and got['p_waic'][g, i] == 0.0 and got['n_tail'][g, i] == 0
        assert got['elpd_loo'][g, i] == 3.75 and got['lpd'][g, i] == 3.75
    for kind in ('nan', 'inf'):
        if kind in where:
            g, i = where[kind]
            assert all(np.isnan(got[k][g, i]) for k in ('lpd', 'elpd_loo', 'pareto_k', 'p_waic')) and got['n_tail'][g, i] == 0
    if (S, N) == (20, 3):
        assert np.all(got['n_tail'] <= 4) and np.all(np.isinf(got['pareto_k']) | np.isnan(got['pareto_k']))
    if 'reff' in where and S <= 4500:
        g, i = where['reff']
        assert got['n_tail'][g, i] == -(-S // 5)


def test_a_column_does_not_depend_on_the_launch():
    from bayes_drt_amd.loo import psis_loo
    ll, reff, _, _ = _case(1000, 7)
    alone = psis_loo(ll[0], reff[0])
    again = psis_loo(ll[0], reff[0])
    rng = np.random.default_rng(5)
    big = rng.standard_normal((5, 1000, 7)) * 1.5 + 4.0
    big[3] = ll[0]
    r5 = np.ones((5, 7))
    r5[3] = reff[0]
    r5[1, 2] = 0.3
    batch = psis_loo(big, r5)
    for k, v in alone.items():
        assert np.array_equal(v, again[k], equal_nan=True), k
        assert np.array_equal(v, batch[k][3], equal_nan=True), k
    twice = psis_loo(big, r5)
    for k, v in batch.items():
        assert np.array_equal(v, twice[k], equal_nan=True), k


def test_draw_limit_is_named():
    from bayes_drt_amd import loo as L
    assert L.max_draws() == 16384
    with pytest.raises(ValueError, match='16384'):
        L.psis_loo(np.zeros((16385, 1)))


# ---------------------------------------------------------------------------------------------------- Inverter surface
BASIS = np.logspace(6, -2, 81)
NAMES = ['trunc_uniform_0.25', 'trunc_Orazem_1.0', 'trunc_Macdonald_2.5']


def _spectrum(name):
    d = load('kat_' + name)
    return np.array(d['data_freq'], dtype=float), np.array(d['data_Z'])


def _equal_results(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def test_inverter_loo_end_to_end(tmp_path, caplog):
    from bayes_drt_amd import loo as L
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', warmup=60, samples=60, chains=3, random_seed=3)
    fit = inv._sample_result
    nf = len(f)
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        res = inv.loo()
    assert res is inv.loo_result and res.n_units == nf and res.n_draws == 180
    lines = [r for r in caplog.records if r.name == 'bayes_drt_amd' and 'Pareto k' in r.getMessage()]
    assert len(lines) == 1 and (lines[0].levelno == logging.WARNING) == (res.n_bad_k > 0)
    # the numpy statement on the fit's arrays (the relative efficiency is the one `loo` reduced, from the same kernel)
    z = np.asarray(inv._stan_input['Z'], dtype=float)
    Zh, sg = fit['Z_hat'], fit['sigma_tot']
    reff = L.relative_efficiency(L.pointwise_log_lik(Zh, sg, z), 3)
    ref = pn.loo(pn.pair_columns(pn.pointwise_log_lik(Zh, sg, z)), reff)
    shift = 2 * np.log(inv._Z_scale)
    print('end to end: k-hat %.2f ... %.2f, n_tail %s; largest deviation elpd_i %.3g, k %.3g' % (
        res.pareto_k.min(), res.pareto_k.max(), sorted(set(res.n_tail.tolist())),
        np.abs(res.elpd_i + shift - ref['elpd_loo']).max(), np.abs(res.pareto_k - ref['pareto_k']).max()))
    assert np.array_equal(res.n_tail, ref['n_tail'])
    assert np.all(np.abs(res.elpd_i + shift - ref['elpd_loo']) <= TOL_ELPD)
    assert np.all(np.abs(res.pareto_k - ref['pareto_k']) <= TOL_K)
    assert np.allclose(res.lpd_i + shift, ref['lpd'], rtol=1e-12, atol=0)
    assert np.allclose(res.p_waic_i, ref['p_waic'], rtol=1e-12, atol=0)
    assert res.p_loo == pytest.approx(np.sum(ref['p_loo']), abs=nf * TOL_ELPD)
    assert res.se == pytest.approx(np.sqrt(nf * np.var(ref['elpd_loo'])), rel=1e-9)
    # log density of the impedance as supplied: exactly -2 Nf log(Z scale) against the scaled one
    raw = L.loo(fit, z, log_scale=0.0)
    assert res.elpd_loo == raw.elpd_loo - 2 * nf * np.log(inv._Z_scale)
    assert res.elpd_waic == raw.elpd_waic - 2 * nf * np.log(inv._Z_scale)
    assert np.array_equal(res.pareto_k, raw.pareto_k) and res.p_loo == raw.p_loo
    # units and parts
    pt = inv.loo(unit='point')
    re_ = inv.loo(part='real')
    assert pt.n_units == 2 * nf and re_.n_units == nf
    assert np.array_equal(re_.elpd_i, L.loo(fit, z, unit='point', log_scale=np.log(inv._Z_scale), columns=slice(0, nf)).elpd_i)
    assert np.allclose(pt.lpd_i[:nf], re_.lpd_i, rtol=1e-12, atol=0)
    rows = L.compare({'frequency': res, 'again': inv.loo()})
    assert rows[1]['elpd_diff'] == 0.0 and rows[1]['dse'] == 0.0
    with pytest.raises(ValueError):
        L.compare({'frequency': res, 'point': pt})
    # save -> load: same result from the stored arrays, with and without the stored Stan data
    fn = str(tmp_path / 'fit.pkl')
    inv.save_fit_data(fn)
    inv2 = Inverter(basis_freq=BASIS)
    inv2.load_fit_data(fn)
    _equal_results(inv2.loo(), res)
    inv3 = Inverter(basis_freq=BASIS)
    inv3.load_fit_data(inv.save_fit_data(which='core'))
    core = inv3.loo()
    assert np.allclose(core.elpd_i, res.elpd_i, rtol=0, atol=1e-9) and np.array_equal(core.n_tail, res.n_tail)
    # a MAP fit has no draws to reweight
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='optimize')
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.loo()


def test_loo_many_equals_single_fits_and_finds_the_planted_outlier():
    """The planted outlier (the impedance of one frequency of the second spectrum times 1.5) has the largest k-hat of its
    spectrum with 3 chains x 60 draws; no more draws were needed."""
    from bayes_drt_amd.inversion import Inverter
    fs, zs = zip(*[_spectrum(n) for n in NAMES])
    zs = [np.array(Z) for Z in zs]
    j0 = 25
    zs[1][j0] *= 1.5
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = Inverter(basis_freq=BASIS).fit_many(fs[0], zs, mode='sample', warmup=60, samples=60, chains=3, random_seed=8,
                                                    check_outliers=False)
    many = Inverter.loo_many(views)
    chunked = Inverter.loo_many(views, chunk_bytes=1)                       # one fit per chunk
    for v, m, c in zip(views, many, chunked):
        assert v.loo_result is c
        _equal_results(m, c)
        _equal_results(m, v.loo())
    k = many[1].pareto_k
    print('planted outlier at %d: k-hat %.3f, the others at most %.3f' % (j0, k[j0], np.delete(k, j0).max()))
    assert int(np.argmax(k)) == j0
