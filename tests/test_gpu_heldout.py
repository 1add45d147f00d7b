"""Prediction at held-out frequencies on the GPU (bdrt_heldout.hip): `heldout_transformed`, `heldout_reduce`, `Sampler.heldout`,
and `Inverter.fit_many(heldout=)`, `kfold_many`, `reloo` on top of them.

Tolerances of piece A are calibrated on the yardstick, never on the kernel: tests/heldout_numpy.py is evaluated in float64 and in
np.longdouble, e_ref is the largest deviation over a case's entries relative to the largest magnitude of that output, and the
kernel must lie within 16 x e_ref of the float64 statement -- it adds the K terms in another order and uses the device's
reciprocal and square root, both first order in the unit roundoff with the same condition number; a wrong term shows at 1e-3.
A case is a (family, H): its entries are those of all three batch sizes, the rows of B = 1 and B = 74 being the leading rows of
B = 5000 (over the two entries of one row at one frequency alone the statement's deviation came out at 3e-18 on the host, below
half a unit roundoff by chance, which no float64 result meets unless it is correctly rounded).  Where two independent float64
statements meet (the kernel against the batch evaluator) each is allowed 16, together 32.  Everything else is equality of bits."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests import heldout_cases as hc
from tests import heldout_numpy as hn
from tests.test_gpu_loo_device import BASIS, N_SPECTRA, NAMES, RUNS, UNIT_PART, _cols, _problem, _run, _spectrum

pytestmark = pytest.mark.gpu

FIELDS = ('lpd', 'mean', 'sd', 'pit')


@functools.lru_cache(maxsize=None)
def _family_problem(name):
    from bayes_drt_amd.model import Problem
    return Problem(**hc.family(name)['kw'])


class _closing:
    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        self.obj.close()


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


# ---------------------------------------------------------------------------------------------------- 1: against the yardstick
@pytest.mark.parametrize('H', hc.HS)
@pytest.mark.parametrize('name', sorted(hc.FAMILIES))
def test_heldout_transformed_against_the_yardstick(name, H):
    from bayes_drt_amd.loo import heldout_transformed
    prob = _family_problem(name)
    f, A = hc.grid(name, H)
    P = hc.rows(name, max(hc.BS))
    Zh, sg, eZ, eS, how = hc.calibrate(name, P, f, A)
    print('heldout parity: %-22s H = %2d  e_ref Z_hat %.3g  sigma_tot %.3g  (%s)' % (name, H, eZ, eS, how))
    assert 0 < eZ < 1e-13 and 0 < eS < 1e-13
    for B in hc.BS:
        gZ, gS = heldout_transformed(prob, P[:B], f, A)
        assert gZ.shape == gS.shape == (B, 2 * H)
        dZ = float(np.max(np.abs(gZ - Zh[:B])) / np.max(np.abs(Zh)))
        dS = float(np.max(np.abs(gS - sg[:B])) / np.max(np.abs(sg)))
        print('heldout parity: %-22s H = %2d  B = %4d  kernel Z_hat %.3g  sigma_tot %.3g' % (name, H, B, dZ, dS))
        assert dZ <= 16 * eZ and dS <= 16 * eS, (name, H, B, dZ, eZ, dS, eS)
    # (A_re, A_im) per block is the stacked form
    pairs = [(a[:H], a[H:]) for a in A]
    gZ2, gS2 = heldout_transformed(prob, P[:74], f, pairs)
    assert np.array_equal(gZ2, gZ[:74]) and np.array_equal(gS2, gS[:74])


# ---------------------------------------------------------------------------------------------------- 2: row independence
@pytest.mark.parametrize('name,H', [('Series-2Parallel_pos', 3), ('Series', 17), ('Parallel', 1)])
def test_a_row_does_not_depend_on_its_place_in_the_launch(name, H):
    from bayes_drt_amd.loo import heldout_transformed
    prob = _family_problem(name)
    f, A = hc.grid(name, H, seed=1)
    base = hc.rows(name, 74, seed=4)
    Z0, s0 = heldout_transformed(prob, base, f, A)
    for i in (0, 1, 31, 32, 63, 64, 73):
        Zi, si = heldout_transformed(prob, base[i:i + 1], f, A)
        assert np.array_equal(Zi[0], Z0[i]) and np.array_equal(si[0], s0[i]), i
    perm = np.random.default_rng(1).permutation(74)
    Zp, sp = heldout_transformed(prob, base[perm], f, A)
    assert np.array_equal(Zp, Z0[perm]) and np.array_equal(sp, s0[perm])
    for pre, B in ((5, 200), (37, 5000), (74, 20000)):
        big = hc.rows(name, B, seed=9)
        big[pre:pre + 74] = base
        Zb, sb = heldout_transformed(prob, big, f, A)
        assert np.array_equal(Zb[pre:pre + 74], Z0) and np.array_equal(sb[pre:pre + 74], s0), (pre, B)


# ---------------------------------------------------------------------------------------------------- 3: in-sample identity
@functools.lru_cache(maxsize=None)
def _draws(chains, n_draws):
    """(unconstrained draws [G, S, D], their constrained parameters [G, S, D]) of a run"""
    smp, prob = _run(chains, n_draws)[:2]
    d = smp.results()[0].reshape(N_SPECTRA, chains * n_draws, prob.D)
    return d, np.stack([prob.transformed(x)[0] for x in d])


@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_in_sample_transformed_agrees_with_the_evaluator(chains, n_draws):
    from bayes_drt_amd.loo import heldout_transformed
    from tests.diag_sharded_worker import problem_kwargs
    smp, prob, Zh, sg, z = _run(chains, n_draws)
    pk = problem_kwargs(N_SPECTRA)
    par = _draws(chains, n_draws)[1]
    A = [np.asarray(pk['blocks'][0]['A'], dtype=float)]
    for g in range(N_SPECTRA):
        yZ, yS, eZ, eS, _ = hc.statement_error(pk['blocks'], par[g], pk['freq'], A, pk['sigma_min'], 1.0)
        y64 = (yZ, yS)
        gZ, gS = heldout_transformed(prob, par[g], pk['freq'], A)
        print('heldout in-sample: S = %4d group %d  e_ref %.3g %.3g  kernel - evaluator %.3g %.3g  kernel - statement %.3g %.3g'
              % (chains * n_draws, g, eZ, eS, _rel(gZ, Zh[g]), _rel(gS, sg[g]), _rel(gZ, y64[0]), _rel(gS, y64[1])))
        assert _rel(gZ, Zh[g]) <= 32 * eZ and _rel(gS, sg[g]) <= 32 * eS
        assert _rel(gZ, y64[0]) <= 16 * eZ and _rel(gS, y64[1]) <= 16 * eS


@pytest.mark.parametrize('unit,part', UNIT_PART)
@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_reduce_equals_the_loo_kernels_bit_for_bit(chains, n_draws, unit, part):
    """Fed the evaluator's own arrays: lpd is `psis_loo`'s, mean, sd, pit are `psis_predict`'s *_post."""
    from bayes_drt_amd.loo import heldout_reduce, pointwise_log_lik, psis_loo, psis_predict
    prob, Zh, sg, z = _run(chains, n_draws)[1:]
    c = _cols(part, prob.nf)
    a = [np.ascontiguousarray(v) for v in (Zh[:, :, c], sg[:, :, c], z[:, c])]
    got = heldout_reduce(*a, unit=unit)
    ref_l = psis_loo(pointwise_log_lik(*a, unit=unit), None)
    ref_p = psis_predict(*a, unit=unit, reff=None)
    assert np.array_equal(got['lpd'], ref_l['lpd']) and np.all(np.isfinite(got['lpd']))
    for k in ('mean', 'sd', 'pit'):
        assert np.array_equal(got[k], ref_p[k + '_post']), k
    one = heldout_reduce(a[0][1], a[1][1], a[2][1], unit=unit)                # G = 1 without the leading axis
    for k in FIELDS:
        assert np.array_equal(one[k], got[k][1]), k
    y = hn.reduce(a[0][0], a[1][0], a[2][0], unit)                           # and the numpy statement, to rounding
    for k in FIELDS:
        assert np.allclose(got[k][0], y[k], rtol=1e-9, atol=1e-12), k


# ---------------------------------------------------------------------------------------------------- 4: device path = host path
def _test_grid(pk, H, seed):
    f = np.asarray(pk['freq'], dtype=float)
    nf = len(f)
    rs = np.random.default_rng(seed)
    i = np.sort(rs.choice(nf - 1, size=H, replace=False))
    Ab = np.asarray(pk['blocks'][0]['A'], dtype=float)
    A = [np.concatenate([0.5 * (Ab[i] + Ab[i + 1]), 0.5 * (Ab[nf + i] + Ab[nf + i + 1])])]
    Z = np.asarray(pk['Z'], dtype=float)
    z = np.concatenate([0.5 * (Z[:, i] + Z[:, i + 1]), 0.5 * (Z[:, nf + i] + Z[:, nf + i + 1])], axis=1)
    return np.sqrt(f[i] * f[i + 1]), A, z + 0.003 * rs.standard_normal(z.shape)


@pytest.mark.parametrize('unit,part', UNIT_PART)
@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_sampler_heldout_equals_the_host_path_bit_for_bit(chains, n_draws, unit, part):
    from bayes_drt_amd.loo import host_heldout
    from tests.diag_sharded_worker import problem_kwargs
    smp, prob = _run(chains, n_draws)[:2]
    H = 5
    f, A, zt = _test_grid(problem_kwargs(N_SPECTRA), H, 3)
    draws = _draws(chains, n_draws)[0]
    host = host_heldout(prob, draws, chains, f, A, zt, unit, part)
    ncols = 2 * H if part == 'both' else H
    assert host['lpd'].shape == (N_SPECTRA, H if unit == 'frequency' else ncols) and host['mean'].shape == (N_SPECTRA, ncols)
    assert all(np.all(np.isfinite(host[k])) for k in FIELDS)
    S = chains * n_draws
    per = (S * (prob.D + 1 + 4 * H + 2 * ncols) + 4 * ncols) * 8             # one group's scratch (bdrt_heldout.hip)
    for budget in (None, per, 2 * per + per // 2, 1):                        # all groups, one, two and a ragged chunk, one
        dev = smp.heldout(0, smp.n_units, chains, f, A, zt, unit=unit, part=part, chunk_bytes=budget)
        for k in FIELDS:
            assert dev[k].shape == host[k].shape and np.array_equal(dev[k], host[k]), (k, budget)
    mid = smp.heldout(chains, 2 * chains, chains, f, A, zt[1], unit=unit, part=part)       # a unit range that is not the whole sampler
    for k in FIELDS:
        assert np.array_equal(mid[k][0], host[k][1]), k
    y = hn.reduce(*[v[2][:, _cols(part, H)] for v in _host_arrays(prob, draws, f, A)], zt[2][_cols(part, H)], unit)
    for k in FIELDS:
        assert np.allclose(host[k][2], y[k], rtol=1e-9, atol=1e-12), k


def _host_arrays(prob, draws, f, A):
    from bayes_drt_amd.loo import heldout_transformed
    tr = [heldout_transformed(prob, prob.transformed(d)[0], f, A) for d in draws]
    return np.stack([t[0] for t in tr]), np.stack([t[1] for t in tr])


def test_sample_units_appends_the_heldout_reduction():
    from bayes_drt_amd import _lib
    from bayes_drt_amd import parallel as par
    from bayes_drt_amd.engine import sample_units
    from tests.diag_sharded_worker import problem_kwargs
    chains, n_draws = RUNS[0]
    smp, prob = _run(chains, n_draws)[:2]
    f, A, zt = _test_grid(problem_kwargs(N_SPECTRA), 2, 5)
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    spec, chain = par.make_units(N_SPECTRA, chains)
    res = sample_units(prob, N_SPECTRA * chains, 30, n_draws, 21, ctrl, spec=spec, chain_ids=chain, diagnostics_chains=chains,
                       loo=dict(chains=chains, reff=None),
                       heldout=dict(chains=chains, freq_test=f, A_test_blocks=A, z_test=zt, unit='point'))
    assert len(res) == 3 and set(res.loo) == {'loo'} and set(res.heldout) == set(FIELDS)
    assert np.array_equal(res[0], smp.results()[0])
    ref = smp.heldout(0, smp.n_units, chains, f, A, zt, unit='point')
    for k in FIELDS:
        assert np.array_equal(res.heldout[k], ref[k]), k
    want = smp.diagnostics(0, smp.n_units, chains)                           # all three extras of one call, each by its name
    assert len(res.diagnostics) == len(want) == 4
    for got, exp in zip(res.diagnostics, want):
        assert np.array_equal(got, exp, equal_nan=True)


# ---------------------------------------------------------------------------------------------------- 5: refusals on the device
def test_refusals_on_the_device():
    from bayes_drt_amd import _lib, loo
    from bayes_drt_amd.engine import Sampler
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    pk = problem_kwargs(1)
    f, A, zt = _test_grid(pk, 2, 1)
    lib = _lib.require_gpu()
    with _closing(Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'], outlier_mode=1)) as outl:
        par = np.ones((3, outl.D))
        with pytest.raises(NotImplementedError, match='outlier error models'):
            loo.heldout_transformed(outl, par, f, A)
        out = np.empty((3, 4))
        Ap = np.ascontiguousarray(A[0].reshape(-1))
        assert lib.bdrt_heldout_transformed(outl.handle, _lib.ptr(par), 3, _lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(out), _lib.ptr(out)) == -2
        assert b'outlier error models are refused' in lib.bdrt_last_error()
        with Sampler(outl, 2, 5, 4, 3, spec=[0, 0]) as smp:                  # (refused before the draws are looked at)
            with pytest.raises(NotImplementedError, match='outlier error models'):
                smp.heldout(0, 2, 2, f, A, zt)
            o = [np.empty((1, 4)) for _ in range(4)]
            assert lib.bdrt_sampler_heldout(smp.handle, 0, 2, 2, 1, 0, 4, 0, _lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(zt),
                                            *[_lib.ptr(x) for x in o]) == -2
            assert b'outlier error models are refused' in lib.bdrt_last_error()
    # the draw limit, by the library itself
    S = loo.max_draws() + 1
    big, o = np.ones((1, S, 2)), [np.empty((1, 2)) for _ in range(4)]
    assert lib.bdrt_heldout_reduce(_lib.ptr(big), _lib.ptr(big), _lib.ptr(np.zeros((1, 2))), 1, S, 2, 1, *[_lib.ptr(x) for x in o]) == -2
    assert b'the kernel holds at most' in lib.bdrt_last_error()
    assert lib.bdrt_heldout_reduce(_lib.ptr(big), _lib.ptr(big), _lib.ptr(np.zeros((1, 2))), 1, 1, 2, 1, *[_lib.ptr(x) for x in o]) == -1
    # the library's own range checks on a sampler
    chains, n_draws = RUNS[0]
    smp, prob = _run(chains, n_draws)[:2]
    pk3 = problem_kwargs(N_SPECTRA)
    f, A, zt = _test_grid(pk3, 2, 1)
    Ap = np.ascontiguousarray(A[0].reshape(-1))
    o = [np.empty((N_SPECTRA, 4)) for _ in range(4)]
    tail = (_lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(zt)) + tuple(_lib.ptr(x) for x in o)
    assert lib.bdrt_sampler_heldout(smp.handle, 0, 3, chains, 0, 0, 4, 0, *tail) == -1
    assert b'bdrt_sampler_heldout: bad unit range' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_heldout(smp.handle, 0, 2 * chains, chains, 1, 0, 2, 0, *tail) == -1
    assert b'pair = 1 needs all 4' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_heldout(smp.handle, 0, 2 * chains, chains, 0, 2, 3, 0, *tail) == -1
    assert lib.bdrt_sampler_heldout(smp.handle, 1, 1 + chains, chains, 0, 0, 4, 0, *tail) == -1
    assert b'different spectra' in lib.bdrt_last_error()
    bad = f.copy(); bad[1] = -1.0
    assert lib.bdrt_sampler_heldout(smp.handle, 0, 2 * chains, chains, 0, 0, 4, 0, _lib.ptr(bad), *tail[1:]) == -1
    assert b'not a positive number' in lib.bdrt_last_error()


@pytest.mark.parametrize('unit', ['frequency', 'point'])
def test_a_non_finite_sigma_gives_nan_in_that_unit_only(unit):
    from bayes_drt_amd.loo import heldout_reduce
    chains, n_draws = RUNS[0]
    prob, Zh, sg, z = _run(chains, n_draws)[1:]
    nf = prob.nf
    ref = heldout_reduce(Zh, sg, z, unit=unit)
    s2 = sg.copy()
    s2[1, 17, 4] = np.inf                                                    # one draw of one real part
    s2[2, 3, nf + 9] = -1.0                                                  # and of one imaginary part
    got = heldout_reduce(Zh, s2, z, unit=unit)
    hit_sc = np.zeros((N_SPECTRA, 2 * nf), dtype=bool)
    if unit == 'frequency':
        hit_sc[1, [4, nf + 4]] = hit_sc[2, [9, nf + 9]] = True
        hit_u = hit_sc[:, :nf] | hit_sc[:, nf:]
    else:
        hit_sc[1, 4] = hit_sc[2, nf + 9] = True
        hit_u = hit_sc
    assert np.array_equal(np.isnan(got['lpd']), hit_u)
    assert np.array_equal(got['lpd'][~hit_u], ref['lpd'][~hit_u])
    for k in ('mean', 'sd', 'pit'):
        assert np.array_equal(np.isnan(got[k]), hit_sc), k
        assert np.array_equal(got[k][~hit_sc], ref[k][~hit_sc]), k


# ---------------------------------------------------------------------------------------------------- 6: through the Inverter
KW = dict(mode='sample', warmup=50, samples=50, chains=2, random_seed=8, check_outliers=False, check_diagnostics=False)


def _small(i=0):
    """The small spectrum of test_fit_many_stores_what_loo_many_would (the truncated grid), descending in frequency."""
    f, Z = _spectrum(NAMES[i])
    f, Z = f[4:], Z[4:]
    o = np.argsort(f)[::-1]
    return f[o], Z[o]


def test_fit_many_heldout_on_the_training_grid_is_the_posterior_predictive():
    """Covers the prediction matrices and the scaling: held out at its own training grid, a fit's predictive is the in-sample
    posterior predictive of `loo_predict`.  e_ref per output: the numpy statement of that output in float64 against
    np.longdouble on this fit's draws."""
    from bayes_drt_amd import engine
    from bayes_drt_amd.inversion import Inverter
    from scipy.special import erfc
    f, Z = _small()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        v = Inverter(basis_freq=BASIS).fit_many(f, [Z], heldout=(f, Z), loo_predict=True, loo_kw=dict(reff=None), **KW)[0]
    h, p = v.heldout_result, v.loo_predict_result
    assert np.array_equal(h.frequencies, f) and np.array_equal(p.frequencies, f) and h.n_draws == 100
    dat = v._stan_input
    blocks, kw, _ = engine.blocks_from_dat(v.stan_model_name, dat)
    A = [np.asarray(b['A'], dtype=float) for b in blocks]
    par = v._sample_result._params
    z = np.asarray(dat['Z'], dtype=float).reshape(-1)
    S = len(par)
    mom = {}
    # the two statements whose difference is e_ref: float64 against np.longdouble, or forward against reversed summation
    variants = [(np.float64, None), (np.longdouble, None)] if hc.LONGDOUBLE else [(np.float64, False), (np.float64, True)]
    for i, (T, rev) in enumerate(variants):                                  # `_moments` of loo_predict_numpy with w = 1 / S, in T
        Zh, sg = hn.transformed(blocks, par, dat['freq'], A, kw['sigma_min'], kw['induc_scale'], dtype=T, reverse=rev)
        d = Zh - z.astype(T)
        m1, m2 = np.sum(d, axis=0) / T(S), np.sum(sg * sg + d * d, axis=0) / T(S)
        phi = (0.5 * erfc((d / (sg * np.sqrt(T(2.0)))).astype(float))).astype(T)     # (erfc itself has no wider form)
        mom[i] = (z.astype(T) + m1, np.sqrt(m2 - m1 * m1), np.sum(phi, axis=0) / T(S))
    e = [float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for a, b in zip(mom[0], mom[1])]
    nf = len(f)
    got = (np.concatenate([h.Z_pred.real, h.Z_pred.imag]), np.concatenate([h.sigma_pred_re, h.sigma_pred_im]),
           np.concatenate([h.pit_re, h.pit_im]))
    want = (np.concatenate([p.Z_post.real, p.Z_post.imag]), np.concatenate([p.sigma_post_re, p.sigma_post_im]),
            np.concatenate([p.pit_post_re, p.pit_post_im]))
    for name, g, w, e_ref in zip(('Z_pred', 'sigma_pred', 'pit'), got, want, e):
        print('heldout inverter: %-10s e_ref %.3g  heldout - loo_predict %.3g' % (name, e_ref, _rel(g, w)))
        assert g.shape == (2 * nf,) and e_ref > 0 and _rel(g, w) <= 32 * e_ref, (name, _rel(g, w), e_ref)
    # the numpy statement itself, in the units of the impedance as supplied, and the log density
    y = hn.reduce(*hn.transformed(blocks, par, dat['freq'], A, kw['sigma_min'], kw['induc_scale']), z)
    assert np.allclose(h.elpd_i, y['lpd'] - 2 * np.log(v._Z_scale), rtol=1e-9, atol=1e-9) and h.elpd == float(np.sum(h.elpd_i))
    assert np.allclose(h.Z_pred, (y['mean'][:nf] + 1j * y['mean'][nf:]) * v._Z_scale, rtol=1e-9)


def test_fit_many_heldout_off_the_training_grid_is_predict_Z_distribution():
    """Three rows taken out of the grid: the prediction rows are built at frequencies the fit has not seen, and the scale is that
    of the training rows.  Z_pred is the mean over the draws of `predict_Z_distribution`, the host's numpy statement on the
    downloaded draws in the units of the impedance as supplied; both are float64 sums of K = 81 terms in another order, K u = 1e-14
    apart at worst, held to 1e-12 of the largest |Z| (a wrong row, scale or term shows at 1e-3).  sigma_pred, PIT and elpd_i are
    the numpy statement's on the same rows, to 1e-9."""
    from bayes_drt_amd import engine
    from bayes_drt_amd.inversion import Inverter
    f, Z = _small()
    test = np.zeros(len(f), dtype=bool)
    test[[3, 20, 41]] = True
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        v = Inverter(basis_freq=BASIS).fit_many(f[~test], [Z[~test]], heldout=(f[test], Z[test]), **KW)[0]
        Zd = v.predict_Z_distribution(f[test])
    assert not np.isin(f[test], v.f_train).any() and len(v.f_train) == len(f) - 3
    assert v._Z_scale == np.std(np.abs(Z[~test])) / np.sqrt((len(f) - 3) / 81)              # the training rows' scale
    h = v.heldout_result
    assert np.array_equal(h.frequencies, f[test]) and Zd.shape == (100, 3)
    assert np.max(np.abs(h.Z_pred - Zd.mean(axis=0))) <= 1e-12 * np.max(np.abs(Zd))
    dat = v._stan_input
    blocks, kw, _ = engine.blocks_from_dat(v.stan_model_name, dat)
    pm = v._get_prediction_matrices(f[test], ['DRT'])['DRT']
    A = [np.concatenate([pm['A_re'], pm['A_im']])]
    yZ, yS = hn.transformed(blocks, v._sample_result._params, f[test], A, kw['sigma_min'], kw['induc_scale'])
    assert np.max(np.abs((yZ[:, :3] + 1j * yZ[:, 3:]) * v._Z_scale - Zd)) <= 1e-12 * np.max(np.abs(Zd))
    zt = np.concatenate([Z[test].real, Z[test].imag]) / v._Z_scale
    y = hn.reduce(yZ, yS, zt)
    assert np.allclose(h.elpd_i, y['lpd'] - 2 * np.log(v._Z_scale), rtol=1e-9, atol=1e-9)
    assert np.allclose(np.concatenate([h.sigma_pred_re, h.sigma_pred_im]), y['sd'] * v._Z_scale, rtol=1e-9)
    assert np.allclose(np.concatenate([h.pit_re, h.pit_im]), y['pit'], rtol=1e-9, atol=1e-12)
    assert np.allclose(np.concatenate([h.resid_re, h.resid_im]), (zt - y['mean']) / y['sd'], rtol=1e-7, atol=1e-9)


def test_kfold_many_equals_separate_fits_bit_for_bit():
    from bayes_drt_amd import loo
    from bayes_drt_amd.inversion import Inverter
    f, Z0 = _small(0)
    Z1 = _small(1)[1]
    perm = np.random.default_rng(4).permutation(len(f))                       # an unsorted supplied grid
    f, Zs = f[perm], [Z0[perm], Z1[perm]]
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = inv.kfold_many(f, Zs, folds=3, **{k: v for k, v in KW.items() if k != 'mode'})
    labels = loo.fold_labels(f, 3)
    assert len(views) == 2 and not hasattr(inv, 'kfold_result') and not hasattr(inv, '_sample_result')
    filled = np.zeros(len(f), dtype=int)
    for lab in range(3):
        test = labels == lab
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sep = Inverter(basis_freq=BASIS).fit_many(f[~test], [Z[~test] for Z in Zs], heldout=[(f[test], Z[test]) for Z in Zs], **KW)
        filled[test] += 1
        for v, s in zip(views, sep):
            r, h = v.kfold_result, s.heldout_result
            assert np.array_equal(r.fold[test], np.full(test.sum(), lab)) and np.array_equal(r.frequencies[test], f[test])
            assert np.array_equal(r.elpd_i[test], h.elpd_i) and np.all(np.isfinite(h.elpd_i))
            for k in ('Z_pred', 'sigma_pred_re', 'sigma_pred_im', 'pit_re', 'pit_im', 'resid_re', 'resid_im'):
                assert np.array_equal(r[k][test], h[k]), k
    assert np.all(filled == 1)
    for v in views:
        r = v.kfold_result
        assert r.method == 'kfold' and r.n_units == len(f) and r.elpd_loo == float(np.sum(r.elpd_i)) and np.all(np.isnan(r.pareto_k))
    rows = loo.compare({'a': views[0].kfold_result, 'b': views[1].kfold_result})
    assert len(rows) == 2 and rows[0]['elpd_diff'] == 0.0 and np.isfinite(rows[1]['dse']) and np.isnan(rows[0]['p_loo'])


def test_reloo_replaces_the_flagged_units_by_exact_refits():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _small()
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, loo=True, loo_kw=dict(reff=None), **KW)
    old = inv.loo_result
    k = np.asarray(old.pareto_k, dtype=float)
    top = np.sort(k[np.isfinite(k)])[::-1]
    thr = 0.5 * (top[1] + top[2])                                            # exactly two units qualify
    cand = np.nonzero(k > thr)[0]
    assert len(cand) == 2
    fit_kw = {kk: v for kk, v in KW.items() if kk != 'mode'}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        new = inv.reloo(f[::-1], Z[::-1], k_threshold=thr, max_refits=None, **fit_kw)       # (any order of the grid)
        exact = []
        for i in cand:
            keep = np.arange(len(f)) != i
            s = Inverter(basis_freq=BASIS).fit_many(f[keep], [Z[keep]], heldout=(f[~keep], Z[~keep]), **KW)[0]
            assert s.heldout_result.frequencies.tolist() == [f[i]]
            exact.append(s.heldout_result.elpd_i[0])
    inv2 = Inverter(basis_freq=BASIS)
    inv2.__dict__.update(inv.__dict__)
    inv2.loo_result, inv2._loo_unit_part = old, ('point', 'both')
    with pytest.raises(ValueError, match=r"loo\(unit='frequency', part='both'\)"):
        inv2.reloo(f, Z, k_threshold=thr, max_refits=None, **fit_kw)
    assert new is inv.loo_result and new is not old and new.method == 'psis+refit'
    assert np.array_equal(np.nonzero(new.refit)[0], cand)
    assert np.array_equal(new.elpd_i[cand], exact) and np.all(np.isfinite(exact))
    rest = ~new.refit
    assert np.array_equal(new.elpd_i[rest], old.elpd_i[rest])
    for key in ('lpd_i', 'pareto_k', 'p_waic_i', 'n_tail'):
        assert np.array_equal(new[key], old[key]), key
    assert new.elpd_loo == float(np.sum(new.elpd_i)) and new.p_loo == float(np.sum(old.lpd_i - new.elpd_i))
    assert new.n_bad_k == int(np.sum((k > 0.7) & rest)) and new.elpd_waic == old.elpd_waic
