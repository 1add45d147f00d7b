"""Held-out prediction under the outlier error models on the GPU (bdrt_heldout_mix.hip): `heldout_mix_reduce`,
`heldout_transformed(..., sigma_out='prior')`, `Sampler.heldout(..., sigma_out='prior')` and `Inverter.kfold` / `reloo` on top.

The tolerance of the kernel is calibrated on the yardstick, never on the kernel (as tests/test_gpu_heldout.py does it):
tests/heldout_mix_numpy.py is evaluated in float64 and in np.longdouble, e_ref is the largest deviation over a case's entries
relative to the largest magnitude of that output, and the kernel must lie within 16 x e_ref of the float64 statement -- the
margin covers the other summation order and the device's exp, erfc and reciprocal square root, each first order in the unit
roundoff.  scipy's erfc has no np.longdouble form, so e_ref of `pit` is the float64 statement summed forward against backward.  A
case is a (S, mode, table); its entries are those of G = 3 groups, N2 = 2 and 6 and both units.

Measured on an MI355X (kernel deviation / e_ref, the largest over the sixteen cases; the test prints every one): lpd 2.6, mean 2.0,
sd 6.3, pit 3.0, with e_ref between 1.1e-16 and 2.3e-16 for lpd, mean and pit and between 3.2e-14 and 8.4e-14 for sd (the
difference of two second moments).  No device math function pushes an output past the factor of 16.
"""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests import heldout_cases as hc
from tests import heldout_mix_numpy as hm
from tests import heldout_numpy as hn

pytestmark = pytest.mark.gpu

FIELDS = ('lpd', 'mean', 'sd', 'pit')
SS = (2, 67, 513, 2049)                              # below a wave, ragged, just over one pass of the block, several passes
N2S = (2, 6)
UNITS = ('frequency', 'point')
G = 3
RESID = np.array([0.0, 3.0, 40.0, -3.0, 0.5, -40.0])    # in base sigmas: at 40 the tail nodes carry the sum


class _closing:
    def __init__(self, obj):
        self.obj = obj

    def __enter__(self):
        return self.obj

    def __exit__(self, *exc):
        self.obj.close()


def _table(mode, kind):
    from bayes_drt_amd import loo
    if kind == 'point mass':
        return np.zeros(1), np.ones(1), 0.0, mode == 1
    return loo.sigma_out_table(mode, 10.0, 5.0, 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(S, N2):
    """Zhat, sig_base [G, S, N2], z [G, N2]: base scales around 0.01, residuals of 0, 3 and 40 of them, shifted from group to group"""
    rs = np.random.default_rng(1000 * S + N2)
    sig = 0.01 * np.exp(0.2 * rs.standard_normal((G, S, N2)))
    Zh = 1.0 + 0.01 * rs.standard_normal((G, S, N2))
    z = 1.0 + 0.01 * np.stack([RESID[(np.arange(N2) + 2 * g) % 6] for g in range(G)])
    return Zh, sig, z


U_ROUND = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _reference(S, mode, kind):
    """({(N2, unit): the float64 statement, per field [G, ...]}, e_ref per field, largest magnitude per field) of a case.  The
    deviations are taken over the entries of group 0 (np.longdouble costs seconds at S = 2049), relative to the largest magnitude
    of the output over all groups; an e_ref below the unit roundoff 2^-53 counts as 2^-53: the two statements can agree to the bit
    (two draws summed forward and backward do), and no float64 result is closer than that to the exact one unless it is
    correctly rounded."""
    tab = _table(mode, kind)
    out, dev, mag = {}, {k: 0.0 for k in FIELDS}, {k: 0.0 for k in FIELDS}
    for N2 in N2S:
        Zh, sig, z = _inputs(S, N2)
        for unit in UNITS:
            y64 = [hm.reduce(Zh[g], sig[g], z[g], tab, unit) for g in range(G)]
            out[(N2, unit)] = {k: np.stack([r[k] for r in y64]) for k in FIELDS}
            rev = hm.reduce(Zh[0], sig[0], z[0], tab, unit, reverse=True)
            wide = hm.reduce(Zh[0], sig[0], z[0], tab, unit, dtype=np.longdouble) if hc.LONGDOUBLE else rev
            for k in FIELDS:
                ref = rev if k == 'pit' else wide
                dev[k] = max(dev[k], float(np.max(np.abs(y64[0][k].astype(ref[k].dtype) - ref[k]))))
                mag[k] = max(mag[k], float(np.max(np.abs(out[(N2, unit)][k]))))
    return out, {k: max(dev[k] / mag[k], U_ROUND) for k in FIELDS}, mag


@pytest.mark.parametrize('kind', ['prior', 'point mass'])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('S', SS)
def test_kernel_against_the_statement(S, mode, kind):
    """G in {1, 3}, N2 in {2, 6}, both units: within 16 x e_ref of the float64 statement; the unit of G = 1 has the bits of the same
    unit inside G = 3; with the point-mass table (Q = 1, y = 0, w = 1) every field is within 4 ulp of bdrt_heldout_reduce."""
    from bayes_drt_amd.loo import heldout_mix_reduce, heldout_reduce
    tab = _table(mode, kind)
    want, e_ref, mag = _reference(S, mode, kind)
    worst = {k: 0.0 for k in FIELDS}
    for N2 in N2S:
        Zh, sig, z = _inputs(S, N2)
        for unit in UNITS:
            got = heldout_mix_reduce(Zh, sig, z, tab, unit)
            one = heldout_mix_reduce(Zh[0], sig[0], z[0], tab, unit)
            mid = heldout_mix_reduce(Zh[1:2], sig[1:2], z[1:2], tab, unit)
            for k in FIELDS:
                assert got[k].shape == want[(N2, unit)][k].shape and np.all(np.isfinite(got[k])), (k, N2, unit)
                assert np.array_equal(one[k], got[k][0]) and np.array_equal(mid[k][0], got[k][1]), (k, N2, unit)
                worst[k] = max(worst[k], float(np.max(np.abs(got[k] - want[(N2, unit)][k]))) / mag[k])
            if kind == 'point mass':
                plain = heldout_reduce(Zh, sig, z, unit)
                for k in FIELDS:
                    ulp = np.max(np.abs(got[k] - plain[k]) / np.spacing(np.maximum(np.abs(plain[k]), np.finfo(float).tiny)))
                    assert ulp <= 4, (k, N2, unit, ulp)
    print('heldout mix: S = %4d mode %d %-10s  ' % (S, mode, kind) +
          '  '.join('%s e_ref %.2g ratio %.2f' % (k, e_ref[k], worst[k] / e_ref[k]) for k in FIELDS))
    for k in FIELDS:
        assert worst[k] <= 16 * e_ref[k], (k, worst[k], e_ref[k])


@pytest.mark.parametrize('unit', UNITS)
def test_a_non_finite_base_sigma_gives_nan_in_that_unit_only(unit):
    from bayes_drt_amd.loo import heldout_mix_reduce
    Zh, sig, z = _inputs(67, 6)
    tab = _table(1, 'prior')
    ref = heldout_mix_reduce(Zh, sig, z, tab, unit)
    s2 = sig.copy()
    s2[1, 17, 1] = np.inf
    s2[2, 3, 5] = -1.0
    got = heldout_mix_reduce(Zh, s2, z, tab, unit)
    hit_sc = np.zeros((G, 6), dtype=bool)
    if unit == 'frequency':
        hit_sc[1, [1, 4]] = hit_sc[2, [2, 5]] = True
        hit_u = hit_sc[:, :3] | hit_sc[:, 3:]
    else:
        hit_sc[1, 1] = hit_sc[2, 5] = True
        hit_u = hit_sc
    assert np.array_equal(np.isnan(got['lpd']), hit_u) and np.array_equal(got['lpd'][~hit_u], ref['lpd'][~hit_u])
    for k in ('mean', 'sd', 'pit'):
        assert np.array_equal(np.isnan(got[k]), hit_sc) and np.array_equal(got[k][~hit_sc], ref[k][~hit_sc]), k
    heavy = heldout_mix_reduce(Zh, sig, z, (tab[0], tab[1], np.inf, True), unit)     # alpha <= 2: no second moment
    assert np.all(np.isinf(heavy['sd'])) and np.array_equal(heavy['lpd'], ref['lpd']) and np.array_equal(heavy['pit'], ref['pit'])


# ---------------------------------------------------------------------------------------------------- the base transform
def _outlier_problem(mode):
    """mode 1: the one-block problem of the sharded tests with the `Series*_outliers` form; mode 2: a two-block family of
    tests/heldout_cases.py with one sigma_out per stacked row"""
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    if mode == 1:
        pk = problem_kwargs(1)
        return Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'], ups_alpha=1.0, ups_beta=0.1, outlier_mode=1), pk
    kw = dict(hc.family('Series-Parallel_pos')['kw'], outlier_mode=2, so_lambda=10.0)
    return Problem(**kw), kw


def _grid(kw, H, seed):
    f = np.asarray(kw['freq'], dtype=float)
    nf = len(f)
    rs = np.random.default_rng(seed)
    i = np.sort(rs.choice(nf - 1, size=H, replace=False))
    A = []
    for b in kw['blocks']:
        Ab = np.asarray(b['A'], dtype=float)
        A.append(np.concatenate([0.5 * (Ab[i] + Ab[i + 1]), 0.5 * (Ab[nf + i] + Ab[nf + i + 1])]))
    Z = np.atleast_2d(np.asarray(kw['Z'], dtype=float))
    z = np.concatenate([0.5 * (Z[:, i] + Z[:, i + 1]), 0.5 * (Z[:, nf + i] + Z[:, nf + i + 1])], axis=1)
    return np.sqrt(f[i] * f[i + 1]), A, z + 0.003 * rs.standard_normal(z.shape)


@pytest.mark.parametrize('mode', [1, 2])
def test_base_transform_of_an_outlier_problem(mode):
    """bdrt_heldout_mix_transformed runs heldout_kernel on a problem with outlier rows in its parameter vector: the statement of
    tests/heldout_numpy.py (whose offsets of x and of the error raws do not move), to 16 x its own rounding error; and a row at
    B = 1 has the bits of the same row inside B = 74."""
    from bayes_drt_amd.loo import heldout_transformed
    prob, kw = _outlier_problem(mode)
    with _closing(prob):
        H = 3
        f, A, _ = _grid(kw, H, 2)
        rs = np.random.default_rng(7)
        if mode == 1:
            par = np.exp(0.3 * rs.standard_normal((74, prob.D)))
        else:                                                                # the family's rows with the 2 Nf outlier rows put in
            base = hc.rows('Series-Parallel_pos', 74, seed=7)
            at = hn.layout(prob.Ks)['err'] + 4
            par = np.concatenate([base[:, :at], np.exp(0.3 * rs.standard_normal((74, 2 * prob.nf))), base[:, at:]], axis=1)
            assert par.shape[1] == prob.D == hn.layout(prob.Ks, 2 * prob.nf)['D']
        Zh, sg, eZ, eS, how = hc.statement_error(kw['blocks'], par, f, A, kw['sigma_min'], kw.get('induc_scale', 1.0))
        gZ, gS = heldout_transformed(prob, par, f, A, sigma_out='prior')
        dZ, dS = float(np.max(np.abs(gZ - Zh)) / np.max(np.abs(Zh))), float(np.max(np.abs(gS - sg)) / np.max(np.abs(sg)))
        print('heldout mix transform: mode %d  e_ref %.3g %.3g (%s)  kernel %.3g %.3g' % (mode, eZ, eS, how, dZ, dS))
        assert gZ.shape == gS.shape == (74, 2 * H) and dZ <= 16 * eZ and dS <= 16 * eS
        for i in (0, 1, 31, 64, 73):
            Zi, si = heldout_transformed(prob, par[i:i + 1], f, A, sigma_out='prior')
            assert np.array_equal(Zi[0], gZ[i]) and np.array_equal(si[0], gS[i]), i


# ---------------------------------------------------------------------------------------------------- device draws = host path
@functools.lru_cache(maxsize=None)
def _sampled(mode):
    from bayes_drt_amd import _lib
    from bayes_drt_amd.engine import Sampler
    prob, kw = _outlier_problem(mode)
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    n_sp = np.atleast_2d(np.asarray(kw['Z'])).shape[0]
    assert n_sp == 1
    smp = Sampler(prob, 4, 30, 40, 21, ctrl, spec=[0, 0, 0, 0], chain_ids=[0, 1, 2, 3])      # two groups of 2 chains
    smp.run()
    return smp, prob, kw, smp.results()[0].reshape(2, 80, prob.D)


@pytest.mark.parametrize('unit,part', [('frequency', 'both'), ('point', 'both'), ('point', 'real')])
@pytest.mark.parametrize('mode', [1, 2])
def test_sampler_heldout_equals_the_host_path_bit_for_bit(mode, unit, part):
    from bayes_drt_amd.loo import host_heldout, sigma_out_prior_table
    smp, prob, kw, draws = _sampled(mode)
    H = 2
    f, A, z1 = _grid(kw, H, 3)
    zt = np.concatenate([z1, z1 + 0.3])                                      # the second group: far off
    host = host_heldout(prob, draws, 2, f, A, zt, unit, part, sigma_out='prior')
    ncols = 2 * H if part == 'both' else H
    assert host['lpd'].shape == (2, H if unit == 'frequency' else ncols) and host['mean'].shape == (2, ncols)
    assert all(np.all(np.isfinite(host[k])) for k in FIELDS)
    per = (80 * (prob.D + 1 + 4 * H + 2 * ncols) + 4 * ncols) * 8             # one group's scratch: two chunks
    for budget in (None, per, 1):
        dev = smp.heldout(0, 4, 2, f, A, zt, unit=unit, part=part, chunk_bytes=budget, sigma_out='prior')
        for k in FIELDS:
            assert dev[k].shape == host[k].shape and np.array_equal(dev[k], host[k]), (k, budget)
    mid = smp.heldout(2, 4, 2, f, A, zt[1], unit=unit, part=part, sigma_out='prior')
    for k in FIELDS:
        assert np.array_equal(mid[k][0], host[k][1]), k
    # and the numpy statement on the same rows, to rounding
    c = {'both': slice(0, 2 * H), 'real': slice(0, H)}[part]
    par = prob.transformed(draws[1])[0]
    yZ, yS = hn.transformed(kw['blocks'], par, f, A, kw['sigma_min'], kw.get('induc_scale', 1.0))
    y = hm.reduce(yZ[:, c], yS[:, c], zt[1][c], sigma_out_prior_table(prob), unit)
    for k in FIELDS:
        assert np.allclose(host[k][1], y[k], rtol=1e-9, atol=1e-12), k


def test_sample_units_takes_the_keyword():
    from bayes_drt_amd import _lib
    from bayes_drt_amd.engine import sample_units
    smp, prob, kw, _ = _sampled(1)
    f, A, zt = _grid(kw, 2, 5)
    zt = np.concatenate([zt, zt])
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    res = sample_units(prob, 4, 30, 40, 21, ctrl, spec=[0, 0, 0, 0], chain_ids=[0, 1, 2, 3],
                       heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt, sigma_out='prior'))
    assert len(res) == 3 and set(res.heldout) == set(FIELDS) and np.array_equal(res[0], smp.results()[0])
    assert res.diagnostics is None and res.loo is None
    ref = smp.heldout(0, 4, 2, f, A, zt, sigma_out='prior')
    for k in FIELDS:
        assert np.array_equal(res.heldout[k], ref[k]), k


# ---------------------------------------------------------------------------------------------------- refusals on the device
def test_mix_refusals_on_the_device():
    from bayes_drt_amd import _lib, loo
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    lib = _lib.require_gpu()
    assert lib.bdrt_heldout_mix_max_nodes() == loo.MIX_MAX_NODES == 512
    o = [np.empty((1, 2)) for _ in range(4)]
    a = np.ones((1, 4, 2))
    zz = np.zeros((1, 2))
    y, w = np.ones(513), np.full(513, 1.0 / 513)

    def reduce(S, arr, Q, ey2=1.0):
        return lib.bdrt_heldout_mix_reduce(_lib.ptr(arr), _lib.ptr(arr), _lib.ptr(zz), 1, S, 2, 1, 1, _lib.ptr(y), _lib.ptr(w), Q, ey2,
                                           *[_lib.ptr(x) for x in o])
    assert reduce(4, a, 513) == -2 and b'the kernel holds at most 512' in lib.bdrt_last_error()
    assert reduce(4, a, 512) == 0 and reduce(4, a, 0) == -1 and reduce(1, a, 4) == -1 and reduce(4, a, 4, np.nan) == -1
    S = loo.max_draws() + 1
    big = np.ones((1, S, 2))
    assert reduce(S, big, 4) == -2 and b'the kernel holds at most' in lib.bdrt_last_error()
    assert reduce(S - 1, big, 512) == 0                                      # the largest launch there is: within the LDS of a CU
    neg = y.copy()
    neg[3] = -1.0
    assert lib.bdrt_heldout_mix_reduce(_lib.ptr(a), _lib.ptr(a), _lib.ptr(zz), 1, 4, 2, 1, 1, _lib.ptr(neg), _lib.ptr(w), 8, 1.0,
                                       *[_lib.ptr(x) for x in o]) == -1
    # a plain problem
    pk = problem_kwargs(1)
    smp1, outl = _sampled(1)[:2]
    f, A, zt = _grid(pk, 2, 1)
    Ap = np.ascontiguousarray(A[0].reshape(-1))
    with _closing(Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'])) as plain:
        par, out = np.ones((3, plain.D)), np.empty((3, 4))
        assert lib.bdrt_heldout_mix_transformed(plain.handle, _lib.ptr(par), 3, _lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(out), _lib.ptr(out)) == -2
        assert b'no outlier error model' in lib.bdrt_last_error()
        with pytest.raises(ValueError, match="sigma_out='prior' needs an outlier error model"):
            loo.heldout_transformed(plain, par, f, A, sigma_out='prior')
        from bayes_drt_amd.engine import Sampler
        with Sampler(plain, 2, 5, 4, 3, spec=[0, 0]) as smp:
            oo = [np.empty((1, 4)) for _ in range(4)]
            assert lib.bdrt_sampler_heldout_mix(smp.handle, 0, 2, 2, 1, 0, 4, 0, _lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(zt), 1, _lib.ptr(y),
                                                _lib.ptr(w), 8, 1.0, *[_lib.ptr(x) for x in oo]) == -2
            assert b'no outlier error model' in lib.bdrt_last_error()
    # the sampler entry's own checks
    oo = [np.empty((2, 4)) for _ in range(4)]
    z2 = np.concatenate([zt, zt])
    tail = (_lib.ptr(f), 2, _lib.ptr(Ap), _lib.ptr(z2), 1, _lib.ptr(y), _lib.ptr(w))
    outs = tuple(_lib.ptr(x) for x in oo)
    assert lib.bdrt_sampler_heldout_mix(smp1.handle, 0, 4, 2, 1, 0, 4, 0, *tail, 513, 1.0, *outs) == -2
    assert b'the kernel holds at most 512' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_heldout_mix(smp1.handle, 0, 3, 2, 1, 0, 4, 0, *tail, 8, 1.0, *outs) == -1
    assert b'bdrt_sampler_heldout_mix: bad unit range' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_heldout_mix(smp1.handle, 0, 4, 2, 1, 0, 2, 0, *tail, 8, 1.0, *outs) == -1
    assert b'pair = 1 needs all 4' in lib.bdrt_last_error()


def test_the_old_refusals_on_the_device_still_hold():
    """tests/test_gpu_heldout.py::test_refusals_on_the_device, unchanged: the entries of section (4b) keep refusing the outlier models"""
    from tests.test_gpu_heldout import test_refusals_on_the_device
    test_refusals_on_the_device()


# ---------------------------------------------------------------------------------------------------- through the Inverter
KW = dict(warmup=100, samples=100, chains=2, random_seed=8, check_diagnostics=False)
BASIS21 = np.logspace(5, -1, 21)
NOISE = 0.002                                        # sd of the simulated noise, in units of R = 1
BAD = 9                                              # the displaced frequency (fold 0 of 3)


def _simulated():
    """21 frequencies of R + RC-like ZARC, noise of sd NOISE, and the real part of one frequency displaced by 30 NOISE"""
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + (1j * 2 * np.pi * f * 1e-2) ** 0.8)
    rs = np.random.default_rng(11)
    Z = Z + NOISE * (rs.standard_normal(21) + 1j * rs.standard_normal(21))
    Z[BAD] += 30 * NOISE
    return f, Z


@functools.lru_cache(maxsize=None)
def _kfolds():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _simulated()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = Inverter(basis_freq=BASIS21).kfold(f, Z, folds=3, outliers=False, **KW)
        b = Inverter(basis_freq=BASIS21).kfold(f, Z, folds=3, outliers=True, sigma_out='prior', **KW)
    return a, b


def test_kfold_ranks_the_outlier_model_against_the_plain_one():
    from bayes_drt_amd import loo
    a, b = _kfolds()
    assert 'sigma_out' not in a and b['sigma_out'] == 'prior' and set(b) - set(a) == {'sigma_out'}
    for r in (a, b):
        assert r.method == 'kfold' and r.n_units == 21 and np.all(np.isfinite(r.elpd_i)) and np.isfinite(r.elpd_loo)
        assert np.all(np.isfinite(r.sigma_pred_re)) and np.all((r.pit_re >= 0) & (r.pit_re <= 1))
    print('kfold: elpd_i at the displaced frequency: plain %.2f, outliers %.2f; elpd_loo plain %.2f, outliers %.2f'
          % (a.elpd_i[BAD], b.elpd_i[BAD], a.elpd_loo, b.elpd_loo))
    assert b.elpd_i[BAD] - a.elpd_i[BAD] > 20
    rows = loo.compare({'plain': a, 'outliers': b})
    assert [r['name'] for r in rows] == ['outliers', 'plain'] and rows[0]['elpd_diff'] == 0.0 and rows[1]['elpd_diff'] < -20
    assert np.isfinite(rows[1]['dse'])


def test_reloo_of_an_outlier_model_replaces_exactly_the_flagged_unit():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _simulated()
    inv = Inverter(basis_freq=BASIS21)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', outliers=True, check_outliers=False, loo=True, loo_kw=dict(reff=None), **KW)
        old = inv.loo_result
        k = np.asarray(old.pareto_k, dtype=float)
        top = np.sort(k[np.isfinite(k)])[::-1]
        thr = 0.5 * (top[0] + top[1])                                        # exactly one unit qualifies
        cand = np.nonzero(k > thr)[0]
        assert len(cand) == 1
        with pytest.raises(NotImplementedError, match='outlier error models'):
            inv.reloo(f, Z, k_threshold=thr, max_refits=1, outliers=True, **KW)
        new = inv.reloo(f, Z, k_threshold=thr, max_refits=1, outliers=True, sigma_out='prior', **KW)
    i = int(cand[0])
    assert new is inv.loo_result and new.method == 'psis+refit' and np.array_equal(np.nonzero(new.refit)[0], cand)
    assert np.isfinite(new.elpd_i[i]) and new.elpd_i[i] != old.elpd_i[i]
    rest = ~new.refit
    assert np.array_equal(new.elpd_i[rest], old.elpd_i[rest]) and np.array_equal(new.pareto_k, old.pareto_k)
