"""PSIS-LOO predictive checks on the GPU: bdrt_loo_predict.hip against the numpy statement (tests/loo_predict_numpy.py) on
identical input, against `psis_loo` for k-hat and n_tail (bit for bit: both kernels take their steps from bdrt_psis.h), batch
independence, and the surface of Inverter fits (`loo_predict`, `loo_predict_many`, `loo_outliers`, save / load).

Tolerances.  NaN / inf patterns and n_tail: equal exactly.  pareto_k, n_tail against `psis_loo(pointwise_log_lik(...))`: equal
bit for bit.  mean_post, sd_post, pit_post: relative 1e-12 of plain numpy means.  mean, sd (in units of the statement's sd)
and pit (absolute): 100 x the largest deviation measured on these inputs on the MI355X (profiles/loo_predict/parity.txt), so
that another fixed summation order in a later kernel does not break the test; never looser than 1e-8, which is a condition on
the kernel and not a measurement."""
import functools
import logging
import warnings

import numpy as np
import pytest

from tests import loo_predict_numpy as lp
from tests.helpers import load

pytestmark = pytest.mark.gpu

# measured on the MI355X (profiles/loo_predict/parity.txt): largest |kernel - numpy statement| over all shapes below
MEASURED_MEAN, MEASURED_SD, MEASURED_PIT = 5.0e-15, 7.6e-15, 3.2e-15
TOL_MEAN = min(100 * MEASURED_MEAN, 1e-8)
TOL_SD = min(100 * MEASURED_SD, 1e-8)
TOL_PIT = min(100 * MEASURED_PIT, 1e-8)

UNITS = ['frequency', 'point']


def _max_draws():
    from bayes_drt_amd import loo as L
    return L.predict_max_draws()


# (S, units per fit); 'max' stands for the draw limit.  (20, 3): n_tail <= 4, raw weights; 4097: no multiple of the 512 threads
SHAPES = [(20, 3), (37, 5), (1000, 7), (4097, 3), ('max', 2)]
SPECIAL = {(20, 3): ('const', 'nan', 'sig0', 'big', 'reff'), (37, 5): ('const', 'nan', 'sig0', 'big', 'low', 'reff', 'tie'),
           (1000, 7): ('const', 'nan', 'sig0', 'big', 'low', 'reff', 'tie'), (4097, 3): ('tie', 'low', 'big', 'reff', 'sig0'),
           ('max', 2): ('reff', 'big', 'tie')}


def _tie_scalar(S):
    """mu, sigma and z of a scalar whose draws come in symmetric pairs mu = z +- sigma l of equal log-likelihood: every
    operand is a short dyadic number, so the two log-likelihoods of a pair are equal to the bit (an odd S: one draw at z)"""
    l = np.round(np.linspace(0.1, 2, S // 2) * 2.0 ** 20) / 2.0 ** 20
    sg = 2.0 ** -11
    mu = np.full(S, 1.0)
    mu[:S // 2] += sg * l
    mu[S // 2:2 * (S // 2)] -= sg * l
    return mu, sg, 1.0


@functools.lru_cache(maxsize=None)
def _case(S, U, unit):
    """Zhat, sig [2, S, N2], z [2, N2], reff [2, U], the numpy statement's results and where the special units are.  The log
    ratios -ll of a scalar are Student-t draws of 3 ... 30 degrees of freedom times 0.05 ... 2.5 (as in test_gpu_loo._case),
    made by placing Z_hat at z + sigma_tot sqrt(2 ratio) with a random sign; sigma_tot is 1e-4 ... 1e-3 per scalar times a
    5 % log-normal factor per draw."""
    tag = S
    if S == 'max':
        S = _max_draws()
    rng = np.random.default_rng(S * 17 + U + (unit == 'point'))
    G, n = 2, 2 if unit == 'frequency' else 1
    N2 = U * n
    z = rng.standard_normal((G, N2))
    sig = np.exp(rng.uniform(np.log(1e-4), np.log(1e-3), (G, 1, N2))) * np.exp(0.05 * rng.standard_normal((G, S, N2)))
    ratio = np.empty((G, S, N2))
    for g in range(G):
        for c in range(N2):
            r = rng.uniform(0.05, 2.5) / n * rng.standard_t(rng.choice([3, 5, 10, 30]), S)
            ratio[g, :, c] = r - r.min()
    sign = np.where(rng.uniform(size=(G, S, N2)) < 0.5, -1.0, 1.0)
    reff = np.ones((G, U))
    where = {}
    flat = [(g, j) for j in range(U) for g in range(G)]                     # specials alternate between the fits
    for kind, (g, j) in zip(SPECIAL[(tag, U)], flat[1:]):
        where[kind] = (g, j)
        c = j + U * (n - 1)                                                 # the unit's last scalar (a pair: the imaginary part)
        if kind == 'big':                                                   # one ratio below log(DBL_MIN) after the shift
            ratio[g, :, c] += 800.0
            ratio[g, S // 3, c] = 0.0
        elif kind == 'low':                                                 # all but one below it: the cutoff is the floor
            ratio[g, S // 3, c] = ratio[g, :, c].max() + 800.0
        elif kind == 'reff':                                                # tail length S / 5 (where 3 sqrt(20 S) exceeds it)
            reff[g, j] = 0.05
    Zhat = z[:, None, :] + sig * (sign * np.sqrt(2.0 * ratio))
    for kind, (g, j) in where.items():
        cols = [j, j + U] if n == 2 else [j]
        c = cols[-1]
        if kind == 'const':                                                 # every draw the same likelihood
            sig[g][:, cols] = sig[g, 0, cols]
            Zhat[g][:, cols] = z[g, cols] + 0.5 * sig[g, 0, cols]
        elif kind == 'nan':
            Zhat[g, S // 2, c] = np.nan
        elif kind == 'sig0':                                                # no scale: in one half of a pair
            sig[g, S // 2, c] = 0.0 if unit == 'frequency' else -0.3
        elif kind == 'tie':
            Zhat[g, :, c], sig[g, :, c], z[g, c] = _tie_scalar(S)
            if n == 2:                                                      # the other half the same for every draw: the sums tie too
                sig[g, :, j] = sig[g, 0, j]
                Zhat[g, :, j] = z[g, j] + 0.25 * sig[g, 0, j]
    ref = [lp.predict(Zhat[g], sig[g], z[g], unit, reff[g]) for g in range(G)]
    ref = {k: np.stack([r[k] for r in ref]) for k in ref[0]}
    for a in (Zhat, sig, z, reff) + tuple(ref.values()):
        a.setflags(write=False)
    return Zhat, sig, z, reff, ref, where


def _same_pattern(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isposinf(got), np.isposinf(ref)) and \
        np.array_equal(np.isneginf(got), np.isneginf(ref))


def _deviations(got, ref):
    """largest deviation of mean and sd in units of the statement's sd, and of pit (absolute), over the finite entries"""
    f = np.isfinite(ref['sd']) & (ref['sd'] > 0)
    if not f.any():
        return 0.0, 0.0, 0.0
    return (float(np.max(np.abs(got['mean'][f] - ref['mean'][f]) / ref['sd'][f])),
            float(np.max(np.abs(got['sd'][f] - ref['sd'][f]) / ref['sd'][f])), float(np.max(np.abs(got['pit'][f] - ref['pit'][f]))))


def _equal(a, b):
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


@pytest.mark.parametrize('unit', UNITS)
@pytest.mark.parametrize('S,U', SHAPES)
def test_psis_predict_matches_numpy_statement(S, U, unit):
    from bayes_drt_amd.loo import pointwise_log_lik, psis_loo, psis_predict
    Zhat, sig, z, reff, ref, where = _case(S, U, unit)
    S = Zhat.shape[1]
    n = 2 if unit == 'frequency' else 1
    got = psis_predict(Zhat, sig, z, unit=unit, reff=reff)
    fin = np.isfinite(ref['pareto_k'])
    dev = _deviations(got, ref)
    print('(S, U, unit) = %s: n_tail %d ... %d, k-hat %.2f ... %.2f, specials %s' % (
        (S, U, unit), ref['n_tail'].min(), ref['n_tail'].max(), ref['pareto_k'][fin].min() if fin.any() else np.nan,
        ref['pareto_k'][fin].max() if fin.any() else np.nan, where))
    print('  largest deviation: mean %.3g sd, sd %.3g sd, pit %.3g' % dev)
    # patterns and n_tail: exactly
    for k in lp.FIELDS + ('pareto_k',):
        assert got[k].shape == ref[k].shape and _same_pattern(got[k], ref[k]), (k, got[k], ref[k])
    assert got['n_tail'].dtype == np.int32 and np.array_equal(got['n_tail'], ref['n_tail']), (got['n_tail'], ref['n_tail'])
    # k-hat and n_tail: those of the LOO kernel on the same input, to the bit
    loo = psis_loo(pointwise_log_lik(Zhat, sig, z, unit=unit), reff)
    assert np.array_equal(got['pareto_k'], loo['pareto_k'], equal_nan=True), np.abs(got['pareto_k'] - loo['pareto_k'])
    assert np.array_equal(got['n_tail'], loo['n_tail'])
    # equal weights: plain means
    for k in ('mean_post', 'sd_post', 'pit_post'):
        f = np.isfinite(ref[k])
        rel = np.abs(got[k][f] - ref[k][f]) / np.abs(ref[k][f])
        print('  %s: largest relative deviation %.3g' % (k, rel.max()))
        assert np.all(rel <= 1e-12), (k, rel.max())
    assert dev[0] <= TOL_MEAN and dev[1] <= TOL_SD and dev[2] <= TOL_PIT, dev
    # the planted units
    cols = lambda j: [j, j + U] if n == 2 else [j]                          # noqa: E731
    if 'const' in where:
        g, j = where['const']
        assert got['pareto_k'][g, j] == np.inf and got['n_tail'][g, j] == 0
        for k in ('mean', 'sd', 'pit'):
            assert np.array_equal(got[k][g, cols(j)], got[k + '_post'][g, cols(j)])
    for kind in ('nan', 'sig0'):
        if kind in where:
            g, j = where[kind]
            assert all(np.all(np.isnan(got[k][g, cols(j)])) for k in lp.FIELDS)       # both halves of a pair
            assert np.isnan(got['pareto_k'][g, j]) and got['n_tail'][g, j] == 0
    lost = sum(k in where for k in ('nan', 'sig0'))
    assert np.isnan(got['pareto_k']).sum() == lost and np.isnan(got['mean']).sum() == lost * n
    if (S, U) == (20, 3):
        assert np.all(got['n_tail'] <= 4) and np.all(np.isinf(got['pareto_k']) | np.isnan(got['pareto_k']))
    if 'reff' in where and S <= 4500:
        g, j = where['reff']
        assert got['n_tail'][g, j] == -(-S // 5)
    if 'tie' in where:
        # the statement's order of the tied draws, not the reversed one: reversing the draws reverses every tied pair
        g, j = where['tie']
        c = cols(j)
        rev = lp.predict_unit(Zhat[g][::-1][:, c], sig[g][::-1][:, c], z[g, c], reff[g, j])
        gap = abs(rev['mean'][-1] - ref['mean'][g, c[-1]]) / ref['sd'][g, c[-1]]
        mine = abs(got['mean'][g, c[-1]] - ref['mean'][g, c[-1]]) / ref['sd'][g, c[-1]]
        print('  tie unit: n_tail %d, reversed order differs by %.3g sd, the kernel by %.3g sd' % (got['n_tail'][g, j], gap, mine))
        assert rev['n_tail'] == ref['n_tail'][g, j] > 4 and gap > 1000 * TOL_MEAN     # (the inputs tell the two orders apart)
        assert mine <= TOL_MEAN
    one = psis_predict(Zhat[0], sig[0], z[0], unit=unit, reff=reff[0])      # 2-D input: G = 1
    _equal(one, {k: v[0] for k, v in got.items()})


@pytest.mark.parametrize('unit', UNITS)
def test_a_unit_does_not_depend_on_the_launch(unit):
    from bayes_drt_amd.loo import psis_predict
    Zhat, sig, z, reff, _, where = _case(1000, 7, unit)
    U, n = 7, 2 if unit == 'frequency' else 1
    alone = psis_predict(Zhat[0], sig[0], z[0], unit=unit, reff=reff[0])
    again = psis_predict(Zhat[0], sig[0], z[0], unit=unit, reff=reff[0])
    _equal(alone, again)
    rng = np.random.default_rng(5)
    zb = rng.standard_normal((5, U * n))
    sb = np.full((5, 1000, U * n), 3e-4)
    Zb = zb[:, None, :] + sb * rng.standard_normal((5, 1000, U * n)) * 1.5
    Zb[3], sb[3], zb[3] = Zhat[0], sig[0], z[0]
    r5 = np.ones((5, U))
    r5[3] = reff[0]
    r5[1, 2] = 0.3
    batch = psis_predict(Zb, sb, zb, unit=unit, reff=r5)
    _equal(alone, {k: v[3] for k, v in batch.items()})
    _equal(batch, psis_predict(Zb, sb, zb, unit=unit, reff=r5))
    # one unit as a fit of its own (the tie unit: its tail is sorted by value and draw index)
    g, j = where['tie']
    c = [j, j + U] if n == 2 else [j]
    solo = psis_predict(Zhat[g][:, c], sig[g][:, c], z[g, c], unit=unit, reff=reff[g, j])
    full = psis_predict(Zhat[g], sig[g], z[g], unit=unit, reff=reff[g])
    for k in lp.FIELDS:
        assert np.array_equal(solo[k], full[k][c]), k
    assert solo['pareto_k'][0] == full['pareto_k'][j] and solo['n_tail'][0] == full['n_tail'][j]


def test_draw_limit_is_named():
    from bayes_drt_amd import loo as L
    lim = L.predict_max_draws()
    assert lim >= 8192
    with pytest.raises(ValueError, match=str(lim)):
        L.psis_predict(np.zeros((lim + 1, 2)), np.ones((lim + 1, 2)), np.zeros(2))


# ---------------------------------------------------------------------------------------------------- Inverter surface
BASIS = np.logspace(6, -2, 81)
NAMES = ['trunc_uniform_0.25', 'trunc_Orazem_1.0', 'trunc_Macdonald_2.5']


def _spectrum(name):
    d = load('kat_' + name)
    return np.array(d['data_freq'], dtype=float), np.array(d['data_Z'])


def test_inverter_loo_predict_end_to_end(tmp_path, caplog):
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', warmup=60, samples=60, chains=3, random_seed=3)
    fit = inv._sample_result
    nf = len(f)
    with caplog.at_level(logging.INFO, logger='bayes_drt_amd'):
        res = inv.loo_predict()
    assert res is inv.loo_predict_result and res.n_draws == 180 and len(res.frequencies) == nf
    lines = [r for r in caplog.records if r.name == 'bayes_drt_amd' and 'LOO predictive check' in r.getMessage()]
    assert len(lines) == 1 and (lines[0].levelno == logging.WARNING) == (res.n_bad_k > 0)
    # k-hat and n_tail are `loo()`'s
    loo = inv.loo()
    assert np.array_equal(res.pareto_k, loo.pareto_k) and np.array_equal(res.n_tail, loo.n_tail) and res.n_bad_k == loo.n_bad_k
    # the numpy statement on the fit's arrays (the relative efficiency is the one `loo_predict` reduced, from the same kernel)
    from bayes_drt_amd import loo as L
    z = np.asarray(inv._stan_input['Z'], dtype=float)
    Zh, sg = fit['Z_hat'], fit['sigma_tot']
    reff = L.relative_efficiency(L.pointwise_log_lik(Zh, sg, z), 3)
    ref = lp.predict(Zh, sg, z, 'frequency', reff)
    sc = inv._Z_scale                                                       # means and sds: in the units of the impedance as supplied
    ref = {k: v * sc if k.startswith(('mean', 'sd')) else v for k, v in ref.items()}
    got = {'mean': np.concatenate((res.Z_loo.real, res.Z_loo.imag)), 'pit': np.concatenate((res.pit_re, res.pit_im)),
           'sd': np.concatenate((res.sigma_loo_re, res.sigma_loo_im))}
    dev = _deviations(got, ref)
    print('end to end: k-hat %.2f ... %.2f, |resid| up to %.2f, KS %.3f (p = %.3f); largest deviation mean %.3g sd, sd %.3g sd, '
          'pit %.3g' % ((res.pareto_k.min(), res.pareto_k.max(), max(np.abs(res.resid_re).max(), np.abs(res.resid_im).max()),
                         res.pit_ks, res.pit_ks_p) + dev))
    assert np.array_equal(res.n_tail, ref['n_tail'])
    assert dev[0] <= TOL_MEAN and dev[1] <= TOL_SD and dev[2] <= TOL_PIT, dev
    assert np.allclose(np.concatenate((res.Z_post.real, res.Z_post.imag)), ref['mean_post'], rtol=1e-12, atol=0)
    assert np.allclose(np.concatenate((res.sigma_post_re, res.sigma_post_im)), ref['sd_post'], rtol=1e-12, atol=0)
    assert np.allclose(np.concatenate((res.pit_post_re, res.pit_post_im)), ref['pit_post'], rtol=1e-12, atol=0)
    # residuals are scale-free: (Z - Z_loo) / sigma_loo in either units
    zs = np.asarray(inv.Z_train)
    assert np.allclose(res.resid_re, (zs.real - res.Z_loo.real) / res.sigma_loo_re, rtol=1e-9, atol=1e-9)
    assert np.allclose(res.resid_im, (zs.imag - res.Z_loo.imag) / res.sigma_loo_im, rtol=1e-9, atol=1e-9)
    assert (res.pit_ks, res.pit_ks_p) == L.ks_uniform(np.concatenate((res.pit_re, res.pit_im)))
    # units and parts: a point of the real part is the same unit either way
    pt = inv.loo_predict(unit='point')
    re_ = inv.loo_predict(part='real')
    im_ = inv.loo_predict(part='imag')
    assert pt.pareto_k.shape == (2 * nf,) and re_.pareto_k.shape == (nf,) and inv.loo_predict_result is im_
    assert np.all(np.isnan(re_.Z_loo.imag)) and np.all(np.isnan(re_.pit_im)) and np.all(np.isnan(im_.resid_re))
    assert np.array_equal(re_.n_tail, pt.n_tail[:nf]) and np.array_equal(im_.n_tail, pt.n_tail[nf:])
    assert np.allclose(re_.Z_loo.real, pt.Z_loo.real, rtol=1e-12, atol=0) and np.allclose(re_.pit_re, pt.pit_re, rtol=1e-12, atol=0)
    assert np.allclose(im_.sigma_loo_im, pt.sigma_loo_im, rtol=1e-12, atol=0)
    assert np.array_equal(re_.Z_post.real, res.Z_post.real)                  # equal weights: no unit in it
    # save -> load: same result from the stored arrays
    fn = str(tmp_path / 'fit.pkl')
    inv.save_fit_data(fn)
    inv2 = Inverter(basis_freq=BASIS)
    inv2.load_fit_data(fn)
    _equal(inv2.loo_predict(), res)
    assert np.array_equal(inv2.loo_outliers(), inv.loo_outliers())
    # a MAP fit has no draws to reweight
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='optimize')
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.loo_predict()
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.loo_outliers()


def test_loo_predict_many_equals_single_fits_and_finds_the_planted_outlier():
    """The planted outlier: the impedance of one frequency of the second spectrum times 1.5 (50 % of |Z| against noise of
    1 % of |Z|), 3 chains x 60 draws."""
    from bayes_drt_amd.inversion import Inverter
    fs, zs = zip(*[_spectrum(n) for n in NAMES])
    zs = [np.array(Z) for Z in zs]
    j0 = 25
    zs[1][j0] *= 1.5
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = Inverter(basis_freq=BASIS).fit_many(fs[0], zs, mode='sample', warmup=60, samples=60, chains=3, random_seed=8,
                                                    check_outliers=False)
    many = Inverter.loo_predict_many(views)
    chunked = Inverter.loo_predict_many(views, chunk_bytes=1)               # one fit per chunk
    for v, m, c in zip(views, many, chunked):
        assert v.loo_predict_result is c
        _equal(m, c)
        _equal(m, v.loo_predict())
    r = many[1]
    loo_z = np.sqrt((r.resid_re ** 2 + r.resid_im ** 2) / 2)
    in_z = np.sqrt((r.resid_post_re ** 2 + r.resid_post_im ** 2) / 2)
    print('planted outlier at %d: LOO residual %.3f (the others at most %.3f), in-sample z-score %.3f (the others at most %.3f), '
          'k-hat %.3f' % (j0, loo_z[j0], np.delete(loo_z, j0).max(), in_z[j0], np.delete(in_z, j0).max(), r.pareto_k[j0]))
    assert int(np.argmax(loo_z)) == j0
    assert j0 in views[1].loo_outliers(3.5)
