"""Power-scaling sensitivity as far as it is reachable without a GPU: the numpy statement (tests/powerscale_numpy.py) has the
properties a cumulative Jensen-Shannon distance must have and classifies two toy normal-normal posteriors as the method's
paper does; the request is normalised as `loo.loo_request` normalises its own; the result survives save / load; the new entry
points are declared in the binding with the header's signatures."""
import os
import pickle
import re

import numpy as np
import pytest

from bayes_drt_amd import _lib
from bayes_drt_amd import powerscale as PS
from bayes_drt_amd.inversion import Inverter
from tests import powerscale_numpy as pw
from tests import psis_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASIS = np.logspace(6, -2, 81)


def _weights(rng, S, alpha, scale=30.0):
    return np.exp(pn.psislw((alpha - 1.0) * scale * rng.standard_normal(S))[0])


# ---------------------------------------------------------------------------------------------------- the distance
@pytest.mark.parametrize('S', [2, 37, 1000])
def test_uniform_weights_give_zero(S):
    rng = np.random.default_rng(S)
    x = rng.standard_normal(S)
    v = pw.cjs2(x, np.full(S, 1.0 / S))
    print('S = %d: cjs2 under uniform weights %.3g' % (S, v))
    assert 0.0 <= v <= 1e-12


def test_range_affine_invariance_ties_and_constant_columns():
    rng = np.random.default_rng(11)
    S = 513
    x = rng.standard_t(4, S)
    for alpha in (0.99, 1.01, 0.5, 2.0):
        w = _weights(rng, S, alpha)
        v = pw.cjs2(x, w)
        assert 0.0 <= v <= 1.0
        for a, b in ((3.5, -2.0), (1e-4, 7.0), (-2.5, 0.3), (-1.0, 0.0)):
            u = pw.cjs2(a * x + b, w)
            assert abs(u - v) <= 1e-12, (alpha, a, b, u, v)
    # one draw carries nearly all the weight: still within [0, 1]
    w = np.full(S, 1e-6 / (S - 1))
    w[5] = 1.0 - 1e-6
    assert 0.0 < pw.cjs2(x, w) <= 1.0
    # a constant column: 0, not NaN
    assert pw.cjs2(np.full(S, 2.5), _weights(rng, S, 0.99)) == 0.0
    # ties: the tied draws' weights may be swapped
    xt = np.round(x, 1)
    w = _weights(rng, S, 1.01)
    vals, counts = np.unique(xt, return_counts=True)
    i, j = np.nonzero(xt == vals[np.argmax(counts)])[0][:2]
    ws = w.copy()
    ws[i], ws[j] = w[j], w[i]
    assert xt[i] == xt[j] and w[i] != w[j]
    assert abs(pw.cjs2(xt, w) - pw.cjs2(xt, ws)) <= 1e-15
    # non-finite input
    xn = x.copy()
    xn[3] = np.nan
    assert np.isnan(pw.cjs2(xn, w)) and np.isnan(pw.cjs2(x, np.full(S, np.nan)))


def _toy(n, ybar, S=1000, seed=7):
    """Prior N(0, 1), n observations of unit variance with mean ybar: S exact posterior draws, their log prior and their
    log-likelihood (up to constants, which cancel)."""
    rng = np.random.default_rng(seed)
    theta = ybar * n / (n + 1.0) + rng.standard_normal(S) / np.sqrt(n + 1.0)
    L_pri = -0.5 * theta ** 2
    L_lik = -0.5 * n * (theta - ybar) ** 2
    out = []
    for L in (L_pri, L_lik):
        lo, hi = (pw.cjs2(theta, np.exp(pw.weights(L, a)[0])) for a in (pw.LOWER_ALPHA, pw.UPPER_ALPHA))
        out.append(pw.sensitivity(lo, hi))
    return out


def test_toy_posteriors_are_classified_as_stated():
    """Margins of a factor of ten on either side of the threshold 0.05."""
    prior, lik = _toy(100, 0.3)
    print('n = 100, ybar = 0.3: prior %.3g, likelihood %.3g' % (prior, lik))
    assert prior < 0.05 <= lik
    assert pw.diagnose([prior], [lik]) == ['-']
    prior, lik = _toy(4, 10.0)
    print('n = 4, ybar = 10: prior %.3g, likelihood %.3g' % (prior, lik))
    assert prior >= 0.05 and lik >= 0.05
    assert pw.diagnose([prior], [lik]) == ['prior-data conflict']


def test_the_statement_end_to_end_on_constructed_components():
    rng = np.random.default_rng(3)
    S, U, D = 200, 7, 3
    par = rng.standard_normal((S, D))
    ll = -0.5 * rng.standard_normal((S, U)) ** 2
    lp0 = ll.sum(axis=1) - 0.5 * np.sum(par ** 2, axis=1)
    r = pw.powerscale(lp0, ll, par)
    assert r['cjs2'].shape == (D, 2, 2) and r['pareto_k'].shape == (2, 2) and r['n_tail'].shape == (2, 2)
    assert np.all((r['cjs2'] >= 0) & (r['cjs2'] <= 1)) and np.all(np.isfinite(r['prior'])) and len(r['diagnosis']) == D
    L_pri, L_lik = pw.components(lp0, ll)
    assert np.allclose(L_pri, -0.5 * np.sum(par ** 2, axis=1), rtol=0, atol=1e-12)
    lp0[17] = np.inf                                                         # a non-finite component: NaN for that fit
    r = pw.powerscale(lp0, ll, par)
    assert np.all(np.isnan(r['prior'])) and np.all(np.isfinite(r['likelihood']))
    assert np.all(np.isnan(r['pareto_k'][0])) and np.all(r['n_tail'][0] == 0) and np.all(r['n_tail'][1] > 0)
    assert r['diagnosis'] == ['-'] * D


# ---------------------------------------------------------------------------------------------------- the package's host side
def test_diagnosis_table_and_sensitivity_match_the_statement():
    thr = 0.05
    prior = np.array([0.2, 0.05, 0.2, 0.049, 0.0, np.nan, 0.3])
    lik = np.array([0.2, 0.05, 0.01, 0.9, 0.0, 0.5, np.nan])
    want = ['prior-data conflict', 'prior-data conflict', 'strong prior / weak likelihood', '-', '-', '-',
            'strong prior / weak likelihood']
    assert PS.diagnose(prior, lik, thr) == want == pw.diagnose(prior, lik, thr)
    assert PS.LABELS == pw.LABELS
    cj = np.random.default_rng(0).uniform(0, 1e-3, (5, 2, 2))
    assert np.array_equal(PS.sensitivity(cj, 1.01), pw.sensitivity(cj[..., 0], cj[..., 1], 1.01))


def test_request_normalisation():
    d = PS.powerscale_request(dict(chains=3), 'sample_units', True)
    assert d == dict(PS.POWERSCALE_DEFAULTS, chains=3) and set(d) == set(PS.POWERSCALE_KEYS)
    d = PS.powerscale_request(None, 'powerscale_kw', False, PS.POWERSCALE_KW)
    assert d['chains'] is None and (d['lower_alpha'], d['upper_alpha'], d['threshold']) == (0.99, 1.01, 0.05)
    with pytest.raises(ValueError, match=r"sample_units: unknown keys \['alpha', 'unit'\] \(powerscale needs chains and takes"):
        PS.powerscale_request(dict(chains=2, alpha=1, unit='point'), 'sample_units', True)
    with pytest.raises(ValueError, match=r"powerscale_kw: unknown keys \['chains'\] \(known:"):
        PS.powerscale_request(dict(chains=2), 'powerscale_kw', False, PS.POWERSCALE_KW)
    with pytest.raises(ValueError, match=r'sample_units: powerscale needs chains \(got \[\]\)'):
        PS.powerscale_request({}, 'sample_units', True)
    for bad in (dict(lower_alpha=0.0), dict(lower_alpha=-0.5), dict(upper_alpha=0.0), dict(lower_alpha=1.01, upper_alpha=0.99),
                dict(lower_alpha=1.0), dict(upper_alpha=1.0), dict(upper_alpha=np.inf), dict(lower_alpha=np.nan),
                dict(upper_alpha='big')):
        with pytest.raises(ValueError, match='lower_alpha'):
            PS.powerscale_request(dict(bad, chains=2), 'sample_units', True)
    with pytest.raises(ValueError, match='threshold'):
        PS.powerscale_request(dict(chains=2, threshold=-1.0), 'sample_units', True)
    with pytest.raises(ValueError, match="part must be 'both', 'real' or 'imag'"):
        PS.powerscale_request(dict(chains=2, part='re'), 'sample_units', True)
    with pytest.raises(ValueError, match='chunk_bytes must not be negative'):
        PS.powerscale_request(dict(chains=2, chunk_bytes=-1), 'sample_units', True)
    assert PS.check_powerscale_kw(dict(threshold=0.1), 'real') == dict(part='real', lower_alpha=0.99, upper_alpha=1.01, threshold=0.1)


def test_fit_arguments_are_refused_before_any_gpu_work(monkeypatch):
    f = np.logspace(5, -1, 31)
    Z = 1.0 + 1.0 / (1.0 + (2j * np.pi * f * 1e-2) ** 0.8)
    called = []
    monkeypatch.setattr(Inverter, '_batch_jobs', lambda *a, **k: called.append('batch') or ([], []))
    monkeypatch.setattr(Inverter, '_fit_prepare', lambda *a, **k: called.append('prepare'))
    inv = Inverter(basis_freq=BASIS)
    with pytest.raises(ValueError, match="mode='sample'"):
        inv.fit(f, Z, mode='optimize', powerscale=True)
    with pytest.raises(ValueError, match="mode='sample'"):
        inv.fit_many(f, [Z, Z], mode='optimize', powerscale=True)
    with pytest.raises(ValueError, match='powerscale is not set'):
        inv.fit_many(f, [Z], mode='sample', powerscale_kw=dict(threshold=0.1))
    with pytest.raises(ValueError, match=r"unknown keys \['part'\]"):
        inv.fit_many(f, [Z], mode='sample', powerscale=True, powerscale_kw=dict(part='real'))
    with pytest.raises(ValueError, match='lower_alpha'):
        inv.fit(f, Z, mode='sample', powerscale=True, powerscale_kw=dict(lower_alpha=1.5))
    assert called == [] and not hasattr(inv, 'powerscale_result')
    assert inv.fit_many(f, [Z], mode='sample', powerscale=True, powerscale_kw=dict(threshold=0.1)) == [] and called == ['batch']
    # no sampling fit: the error of `loo()`
    inv.fit_type = 'map'
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        inv.powerscale()
    with pytest.raises(ValueError, match='only available for bayes_fit'):
        Inverter.powerscale_many([inv])


def _result():
    rng = np.random.default_rng(1)
    D = 6
    cj = rng.uniform(0, 1e-7, (D, 4))                                       # sensitivities of at most 0.022
    cj[2] = [4e-6, 5e-6, 1e-5, 2e-5]
    cj[4] = [9e-6, 8e-6, 1e-9, 1e-9]
    names = ['Rinf_raw', 'induc_raw', 'x[0]', 'x[1]', 'ups_raw[0]', 'd0_strength']
    return PS._result(cj, [0.1, 0.2, -0.1, 0.3], [40, 40, 40, 40], names, 0.99, 1.01, 0.05, 200)


def test_result_is_dict_like_and_survives_save_and_load(tmp_path):
    r = _result()
    assert isinstance(r, dict) and r.prior is r['prior'] and r.cjs2.shape == (6, 2, 2) and r.pareto_k.shape == (2, 2)
    assert r.n_tail.dtype == np.int32 and r.alphas == (0.99, 1.01) and r.threshold == 0.05 and r.n_draws == 200
    assert np.array_equal(r.prior, pw.sensitivity(r.cjs2[:, 0, 0], r.cjs2[:, 0, 1]))
    assert r.diagnosis[2] == 'prior-data conflict' and r.diagnosis[4] == 'strong prior / weak likelihood'
    assert r.flagged() == [n for n, p, l in zip(r.names, r.prior, r.likelihood) if p >= 0.05 or l >= 0.05] and 'x[0]' in r.flagged()
    text = str(r)
    assert 'x[0]' in text and 'prior-data conflict' in text and 'Rinf_raw' not in text
    with pytest.raises(AttributeError):
        r.nothing
    inv = Inverter(basis_freq=BASIS)
    inv.fit_type = 'bayes'
    inv.powerscale_result = r
    assert 'powerscale_result' in inv.get_fit_attributes('detail') and 'powerscale_result' not in inv.get_fit_attributes('core')
    fn = str(tmp_path / 'fit.pkl')
    inv.save_fit_data(fn)
    back = Inverter(basis_freq=BASIS)
    back.load_fit_data(fn)
    got = back.powerscale_result
    assert isinstance(got, PS.PowerscaleResult) and set(got) == set(r) and got.flagged() == r.flagged() and str(got) == text
    for k in r:
        assert np.array_equal(np.asarray(got[k]), np.asarray(r[k])), k
    assert pickle.loads(pickle.dumps(r)).names == r.names


# ---------------------------------------------------------------------------------------------------- the binding
def _header_params(name):
    txt = open(os.path.join(ROOT, 'include', 'bdrt.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)' % name, txt)
    assert m, name
    return [p.strip() for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']


@pytest.mark.parametrize('name', ['bdrt_powerscale', 'bdrt_sampler_powerscale', 'bdrt_powerscale_max_draws',
                                  'bdrt_debug_powerscale_cjs', 'bdrt_debug_powerscale_weights'])
def test_entry_points_are_declared_exported_and_bound_with_the_headers_signature(name):
    import ctypes as C
    lib = _lib.load_library()
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    params = _header_params(name)
    argtypes = getattr(lib, name).argtypes
    assert len(argtypes) == len(params), (name, params)
    for p, t in zip(params, argtypes):
        if '*' in p:
            assert t is C.c_void_p, (name, p)
        elif p.startswith('double'):
            assert t is C.c_double, (name, p)
        elif p.startswith('size_t'):
            assert t is C.c_size_t, (name, p)
        else:
            assert p.startswith('int') and t is C.c_int, (name, p)
