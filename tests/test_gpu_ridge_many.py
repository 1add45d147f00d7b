"""GPU tests (-m gpu) of Inverter.ridge_fit_many and the two entries under it: the loop of `ridge_fit` calls over spectra of the
reference's hyper-ridge study (code_EchemActa/comparisons/hyper-ridge/hyper-ridge run fits.ipynb) as batches.  The ridge QPs
are nearly flat, so everything here is compared bit for bit with the single-spectrum path."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests.helpers import load

pytestmark = pytest.mark.gpu
BASIS = np.logspace(7, -3, 41)            # n = K + 2 = 43: no multiple of the 16-wide tile
TAU_PLOT = np.logspace(-7, 2, 60)
DDT = {'DDT': {'kernel': 'DDT', 'symmetry': 'planar', 'bc': 'transmissive', 'dist_type': 'parallel', 'basis_freq': np.logspace(6, -3, 37)}}


def _spectra(n=3, stem='2ZARC_uniform_0.25', sl=slice(None, None, 2)):
    """tests/test_gpu_fit_many.py::_spectra on every second frequency (41 of 81)"""
    c = load('csv_' + stem)
    Z = c['Z'][sl]
    f, z0 = Z[:, 0], Z[:, 1] + 1j * Z[:, 2]
    rs = np.random.RandomState(5)
    zs = [z0] + [z0 * (1.0 + 0.3 * k) + 0.003 * (rs.standard_normal(len(f)) + 1j * rs.standard_normal(len(f))) for k in range(1, n)]
    return f, zs


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------ bdrt_gram_batch
@pytest.mark.parametrize('R,n', [(21, 37), (42, 37), (3, 5), (81, 83), (162, 163)])
@pytest.mark.parametrize('with_l1', [False, True])
def test_gram_batch_equals_gram_of_the_host_weighted_rows(R, n, with_l1):
    from bayes_drt_amd import _lib
    lib = _lib.require_gpu()
    rs = np.random.RandomState(R * 1000 + n)
    ng = 3
    A = np.ascontiguousarray(rs.standard_normal((R, n)) * np.exp(rs.uniform(-3, 3, (R, 1))))
    Zs = (rs.uniform(0.5, 3.0, (ng, R)) + 1j * rs.uniform(-1.0, 1.0, (ng, R)))
    w = np.ascontiguousarray(1.0 / np.sqrt(np.real(Zs * Zs.conjugate())))          # 'modulus' weights: they depend on the spectrum
    t = np.ascontiguousarray(rs.standard_normal((ng, R)))
    L1 = np.ascontiguousarray(rs.uniform(0.0, 1.0, n)) if with_l1 else None
    G = np.full((ng, n, n), np.nan); q = np.full((ng, n), np.nan)
    _lib.check(lib.bdrt_gram_batch(_ptr(A), R, n, _ptr(w), _ptr(t), ng, _ptr(L1), _ptr(G), _ptr(q)), 'bdrt_gram_batch')
    for g in range(ng):
        WA = np.ascontiguousarray(np.diag(w[g]) @ A); WT = np.ascontiguousarray(np.diag(w[g]) @ t[g])
        assert np.array_equal(WA, w[g][:, None] * A)                   # the rounded products the kernel forms itself
        G1 = np.empty((n, n)); q1 = np.empty(n)
        _lib.check(lib.bdrt_gram(_ptr(WA), _ptr(WT), R, n, None, _ptr(L1), _ptr(G1), _ptr(q1)), 'bdrt_gram')
        assert np.array_equal(G[g], G1), (g, np.max(np.abs(G[g] - G1)))
        assert np.array_equal(q[g], q1), (g, np.max(np.abs(q[g] - q1)))


# ------------------------------------------------------------------ bdrt_ridge_ex against bdrt_ridge
def _setups(penalty, parts=('real', 'imag')):
    from bayes_drt_amd.inversion import Inverter
    f, zs = _spectra(1)
    inv = Inverter(basis_freq=BASIS)
    return [inv._ridge_setup(f, zs[0], p, penalty, 2, 0, True, True, None, False) for p in parts]


def _ridge_raw(setups, sel, lambdas, hyper_lambda, hl_beta=2.5, max_iter=6, mask=None, fbeta=None, flags_g=None, fbeta_b=None):
    """One launch of bdrt_ridge (mask, fbeta) or of bdrt_ridge_ex (flags_g, fbeta_b) on the data parts `setups`; every output."""
    from bayes_drt_amd import _lib
    from bayes_drt_amd.inversion import Inverter
    lib = _lib.require_gpu()
    st0 = setups[0]
    n, nb, ng = st0['n'], len(sel), len(setups)
    o = _lib.RidgeOptions()
    o.n, o.K, o.off, o.penalty = n, st0['K'], st0['off'], 1 if st0['penalty'] == 'integral' else 0
    o.max_iter, o.hyper_lambda, o.xtol = max_iter, int(hyper_lambda), 1e-3
    for i in range(3):
        o.reg_ord[i] = float(st0['reg_ord'][i])
    G = np.ascontiguousarray(np.stack([s['G'] for s in setups]))
    qb = np.ascontiguousarray(np.stack([-s['g'] + s['L1_vec'] for s in setups]))
    base = np.ascontiguousarray(np.stack(st0['base']))
    Ls = np.ascontiguousarray(np.stack(st0['Ls'])) if st0['Ls'] is not None else None
    lam = np.ascontiguousarray(lambdas, dtype=np.float64)
    terms = [Inverter._hyper_prior_terms(st0['penalty'], hl_beta, l) for l in lam]
    lam0s = np.ascontiguousarray(np.stack([t[2] for t in terms])); betas = np.ascontiguousarray(np.stack([t[3] for t in terms]))
    gsel = np.ascontiguousarray(sel, dtype=np.int32)
    lo = np.ascontiguousarray(st0['lo'], dtype=np.float64)
    out = dict(coef=np.full((nb, n), np.nan), lam=np.full((nb, 3, n), np.nan), cost=np.full(nb, np.nan), fun=np.full(nb, np.nan),
               iters=np.zeros(nb, dtype=np.int32), flags=np.zeros(nb, dtype=np.int32), hc=np.zeros((nb, max_iter, n)),
               hl=np.zeros((nb, max_iter, 3, n)), hf=np.zeros((nb, max_iter)), hk=np.zeros((nb, max_iter)))
    tail = [_ptr(G), _ptr(qb), _ptr(gsel), _ptr(base), _ptr(Ls), _ptr(lo), _ptr(lam), _ptr(lam0s), _ptr(betas), None] + \
        [_ptr(out[k]) for k in ('coef', 'lam', 'cost', 'fun', 'iters', 'flags', 'hc', 'hl', 'hf', 'hk')]
    if flags_g is None:
        o.zero_delta1, o.hl_fbeta = int(mask), float(fbeta or 0.0)
        _lib.check(lib.bdrt_ridge(C.byref(o), nb, ng, *tail), 'bdrt_ridge')
    else:
        zd = np.ascontiguousarray(flags_g, dtype=np.uint8); fb = np.ascontiguousarray(fbeta_b, dtype=np.float64)
        assert len(zd) == ng and len(fb) == nb
        _lib.check(lib.bdrt_ridge_ex(C.byref(o), _ptr(zd), _ptr(fb), nb, ng, *tail), 'bdrt_ridge_ex')
    return out


def _same_outputs(a, b, ja=slice(None), jb=slice(None)):
    for k in a:
        if k not in ('hc', 'hl'):
            assert np.array_equal(a[k][ja], b[k][jb]), k
    # the history rows a fit wrote (the entry leaves the rows beyond its last iteration as they were)
    for x, y, its in zip(zip(a['hc'][ja], a['hl'][ja]), zip(b['hc'][jb], b['hl'][jb]), a['iters'][ja]):
        assert np.array_equal(x[0][:its], y[0][:its]) and np.array_equal(x[1][:its], y[1][:its])


@pytest.mark.parametrize('penalty,hyper_lambda', [('discrete', True), ('integral', True), ('discrete', False)])
def test_ridge_ex_equals_ridge_bit_for_bit(penalty, hyper_lambda):
    setups = _setups(penalty)
    sel, lams = [0, 1, 0, 1], [1e-2, 1e-2, 1e-1, 1e-1]
    hb = 5 if penalty == 'integral' else 2.5
    old = _ridge_raw(setups, sel, lams, hyper_lambda, hl_beta=hb, mask=0b01, fbeta=0.0)
    new = _ridge_raw(setups, sel, lams, hyper_lambda, hl_beta=hb, flags_g=[1, 0], fbeta_b=[0.0] * 4)
    assert np.all(np.isfinite(old['coef'])) and np.all(old['iters'] >= 1)
    _same_outputs(old, new)


def test_one_hl_fbeta_per_fit_equals_one_launch_per_value():
    setups = _setups('discrete', parts=('both',))
    both = _ridge_raw(setups, [0, 0], [1e-2, 1e-2], True, flags_g=[0], fbeta_b=[0.1, 0.5])
    for j, fb in enumerate((0.1, 0.5)):
        one = _ridge_raw(setups, [0], [1e-2], True, mask=0, fbeta=fb)
        _same_outputs(both, one, slice(j, j + 1), slice(0, 1))
    assert not np.array_equal(both['coef'][0], both['coef'][1])


def test_flag_of_a_data_part_beyond_31():
    st = _setups('discrete', parts=('both',))[0]
    flags = np.zeros(33, dtype=np.uint8); flags[32] = 1
    new = _ridge_raw([st] * 33, [32, 0], [1e-2, 1e-2], True, max_iter=20, flags_g=flags, fbeta_b=[0.0, 0.0])
    old = _ridge_raw([st], [0], [1e-2], True, max_iter=20, mask=1, fbeta=0.0)
    _same_outputs(new, old, slice(0, 1), slice(0, 1))
    unset = _ridge_raw([st], [0], [1e-2], True, max_iter=20, mask=0, fbeta=0.0)
    _same_outputs(new, unset, slice(1, 2), slice(0, 1))
    print('iterations with the flag %d, without %d' % (new['iters'][0], new['iters'][1]))


# ------------------------------------------------------------------ ridge_fit_many against separate ridge_fit calls
def _assert_same_fit(v, one, f, name='DRT'):
    a, b = v.distribution_fits[name], one.distribution_fits[name]
    assert set(a) == set(b)
    assert np.array_equal(a['coef'], b['coef'])
    if 'scaled_coef' in b:
        assert np.array_equal(a['scaled_coef'], b['scaled_coef'])
    if 'lambda_vectors' in b:
        assert len(a['lambda_vectors']) == len(b['lambda_vectors'])
        for la, lb in zip(a['lambda_vectors'], b['lambda_vectors']):
            assert np.array_equal(la, lb)
    assert a['cost'] == b['cost'] and np.array_equal(a['opt_result']['x'], b['opt_result']['x'])
    assert v.R_inf == one.R_inf and v.inductance == one.inductance and v._Z_scale == one._Z_scale
    assert v.fit_type == one.fit_type == 'ridge'
    assert np.array_equal(v.f_train, one.f_train) and np.array_equal(v.Z_train, one.Z_train)
    ha, hb = v._iter_history, one._iter_history
    assert (ha is None) == (hb is None)
    if hb is not None:
        assert len(ha) == len(hb)
        for x, y in zip(ha, hb):
            assert np.array_equal(x['coef'], y['coef'])
    assert np.array_equal(v.predict_Z(f), one.predict_Z(f))
    assert np.array_equal(v.predict_distribution(name, eval_tau=TAU_PLOT), one.predict_distribution(name, eval_tau=TAU_PLOT))


def _make(dist=None, **kw):
    from bayes_drt_amd.inversion import Inverter
    return Inverter(distributions=dist, **kw) if dist is not None else Inverter(basis_freq=BASIS, **kw)


@pytest.mark.parametrize('case', ['defaults', 'huang', 'ordinary', 'real', 'signed', 'ddt'])
def test_ridge_fit_many_equals_separate_calls(case):
    kw = {'defaults': {}, 'huang': dict(preset='Huang'), 'ordinary': dict(hyper_lambda=False), 'real': dict(part='real'),
          'signed': dict(nonneg=False), 'ddt': {}}[case]
    dist = DDT if case == 'ddt' else None
    f, zs = _spectra(4, 'BimodalTP-DDT_uniform_0.25') if case == 'ddt' else _spectra(4)
    name = 'DDT' if case == 'ddt' else 'DRT'
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = _make(dist).ridge_fit_many(f, zs, **kw)
        assert len(views) == 4
        for Z, v in zip(zs, views):
            one = _make(dist)
            one.ridge_fit(f, Z, **kw)
            _assert_same_fit(v, one, f, name)
    assert not np.array_equal(views[0].distribution_fits[name]['coef'], views[1].distribution_fits[name]['coef'])


def test_lists_and_mixed_grids_come_back_in_input_order():
    f41, zs = _spectra(4)
    grids = [f41, f41[:33], f41, f41[:33]]
    zs = [Z[:len(g)] for Z, g in zip(zs, grids)]
    lam, fb, hb = [1e-2, 1e-1, 1e-3, 1e-2], [0.1, None, 0.5, 0.2], [2.5, 3.0, 2.5, 4.0]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = _make().ridge_fit_many(grids, zs, lambda_0=lam, hl_fbeta=fb, hl_beta=hb)
        for i, v in enumerate(views):
            one = _make()
            one.ridge_fit(grids[i], zs[i], lambda_0=lam[i], hl_fbeta=fb[i], hl_beta=hb[i])
            assert len(v.f_train) == len(grids[i])
            _assert_same_fit(v, one, grids[i])


def test_lambda_0_from_the_batched_cross_validation():
    f, zs = _spectra(3)
    lams = np.logspace(-6, 2, 5)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = _make().ridge_fit_many(f, zs, lambda_0='cv', cv_lambdas=lams)
        for Z, v in zip(zs, views):
            one = _make()
            one.ridge_fit(f, Z, lambda_0='cv', cv_lambdas=lams)
            tot = np.sort(one.cv_result['totcv'])
            print('totcv', one.cv_result['totcv'])
            assert tot[1] - tot[0] > 1e-6 * tot[0]                       # the choice of lambda_0 is no knife edge
            for k in ('lambda', 'recv', 'imcv', 'totcv'):
                assert np.allclose(v.cv_result[k], one.cv_result[k], rtol=1e-12, atol=0), k
            assert lams[np.argmin(v.cv_result['totcv'])] == lams[np.argmin(one.cv_result['totcv'])]
            _assert_same_fit(v, one, f)


def test_33_spectra_without_inductance_and_chunked_launches(monkeypatch):
    f, zs = _spectra(33)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = _make(fit_inductance=False).ridge_fit_many(f, zs)
        for Z, v in zip(zs, views):
            one = _make(fit_inductance=False)
            one.ridge_fit(f, Z)
            _assert_same_fit(v, one, f)
        monkeypatch.setenv('BDRT_RIDGE_CHUNK', '7')
        cut = _make(fit_inductance=False).ridge_fit_many(f, zs)
    for a, b in zip(views, cut):
        _assert_same_fit(a, b, f)


@pytest.mark.parametrize('algorithm', ['LBFGS', None])
def test_fit_many_map_ridge_start_of_spectrum_32(monkeypatch, algorithm):
    """`fit_many(mode='optimize')` solves the ridge starting points of all spectra in one launch: with the inductance not fitted
    every data part carries the convergence flag, also the parts beyond the 31 a bit mask could name.  (The flag acts from the
    second hyper-lambda iteration's convergence test on: the starting point's default of two iterations never consults it, so
    the ridge starts iterate to convergence here.)"""
    from bayes_drt_amd.inversion import Inverter
    monkeypatch.setenv('BDRT_RIDGE_START_ITER', '20')
    f, zs = _spectra(33, sl=slice(None, None, 4))
    basis = np.logspace(6.5, -2.5, 19)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        kw = dict(nonneg=True, mode='optimize', algorithm=algorithm, max_iter=60 if algorithm else 50000)
        views = Inverter(basis_freq=basis, fit_inductance=False).fit_many(f, zs, **kw)
        one = Inverter(basis_freq=basis, fit_inductance=False)
        one.fit(f, zs[32], **kw)
    v = views[32]
    assert len(v._opt_report['starts']) == len(one._opt_report['starts']) == 2
    for a, b in zip(v._opt_report['starts'], one._opt_report['starts']):
        assert all(a[k] == b[k] for k in ('iterations', 'n_evals', 'newton_iterations', 'return_code')), (a, b)
        assert a['lp'] == pytest.approx(b['lp'], rel=1e-9)
    assert v._opt_report['start'] == one._opt_report['start']
    assert np.allclose(v.distribution_fits['DRT']['coef'], one.distribution_fits['DRT']['coef'], rtol=1e-9, atol=1e-12)


def test_host_variant_runs_as_a_loop_of_ridge_fit():
    f, zs = _spectra(2)
    kw = dict(hyper_weights=True, hyper_lambda=False, max_iter=3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = _make().ridge_fit_many(f, zs, **kw)
        for Z, v in zip(zs, views):
            one = _make()
            one.ridge_fit(f, Z, **kw)
            _assert_same_fit(v, one, f)
            assert np.array_equal(v.distribution_fits['DRT']['weights'], one.distribution_fits['DRT']['weights'])


def test_instance_is_left_alone_and_views_can_be_refitted():
    f, zs = _spectra(2)
    base = _make()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = base.ridge_fit_many(f, zs, lambda_0=['cv', 1e-2], cv_lambdas=np.logspace(-4, 0, 3))
        assert base.distribution_fits == {} and base._iter_history is None and base.Z_train is None and base._Z_scale == 1.0
        assert base.distribution_matrices == {'DRT': {}} and list(base.f_train) == [0]
        for a in ('fit_type', 'R_inf', 'inductance', 'cv_result'):
            assert not hasattr(base, a), a
        assert hasattr(views[0], 'cv_result') and not hasattr(views[1], 'cv_result')
        v = views[1]
        v.ridge_fit(f, zs[0])
        one = _make()
        one.ridge_fit(f, zs[0])
        _assert_same_fit(v, one, f)
        v.fit(f, zs[0], nonneg=True, mode='optimize')
        assert v.fit_type == 'map' and v._opt_report['return_code'] == 0
    assert views[0].fit_type == 'ridge'
