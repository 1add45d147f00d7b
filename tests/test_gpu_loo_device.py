"""PSIS-LOO and the LOO predictive check on a sampler's device draws (`Sampler.loo`, `Sampler.loo_predict`, bdrt_sampler_loo,
bdrt_sampler_loo_predict) against the host path on the same run's downloaded draws, and `fit_many(loo=..., loo_predict=...)`
against `loo_many` / `loo_predict_many` run afterwards.

Equality is the specification: with reff None, a number or an array every field equals the host path bit for bit, NaN patterns
and n_tail included.  That rests on the batch evaluator giving a row the same Z_hat and sigma_tot wherever the row sits in a
launch, which the first test states on its own.  reff='auto' is the one place where the paths may differ (the device's exp is not
numpy's): the device result must equal the host `psis_loo` given the returned reff bit for bit, and the returned reff is held to
`loo.relative_efficiency` on the same log-likelihoods within 100 x the largest relative deviation measured on the MI355X over the
shapes below (profiles/loo_device/parity.txt), never looser than 1e-8 relative, which is a condition on the kernel and not a
measurement; where both put 1, the entries are equal exactly."""
import copy
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests.helpers import load

pytestmark = pytest.mark.gpu

# measured on the MI355X (profiles/loo_device/parity.txt): largest |reff_device - reff_host| / reff_host over RUNS x UNIT_PART
MEASURED_REFF = 1.4e-15
TOL_REFF = min(100 * MEASURED_REFF, 1e-8)

N_SPECTRA = 3
RUNS = [(2, 37), (4, 250)]                           # S = 74: no multiple of the 32-wide transpose tile or of 64; S = 1000
UNIT_PART = [('frequency', 'both'), ('point', 'both'), ('point', 'real'), ('point', 'imag')]
LOO_FIELDS = ('lpd', 'elpd_loo', 'p_loo', 'pareto_k', 'p_waic', 'elpd_waic', 'n_tail')


def _problem():
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    pk = problem_kwargs(N_SPECTRA)
    return Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'], ups_alpha=1.0, ups_beta=0.1), pk


def test_transformed_does_not_depend_on_the_place_of_a_row_in_the_launch():
    """Runs only existing code: Z_hat and sigma_tot of 74 rows alone (B = 1), permuted, and embedded at rows that are no multiple
    of the evaluator's 16-row tile in batches of 200, 5000 and 20000 rows (the last is more tiles than workgroups, so
    workgroups walk several tiles)."""
    prob, _ = _problem()
    rs = np.random.RandomState(5)
    base = rs.uniform(-2, 2, (74, prob.D))
    _, Zh0, sg0 = prob.transformed(base)
    for i in (0, 1, 15, 16, 17, 73):
        _, Zh, sg = prob.transformed(base[i:i + 1])
        assert np.array_equal(Zh[0], Zh0[i]) and np.array_equal(sg[0], sg0[i]), i
    perm = rs.permutation(74)
    _, Zh, sg = prob.transformed(base[perm])
    assert np.array_equal(Zh, Zh0[perm]) and np.array_equal(sg, sg0[perm])
    for pre, B in ((5, 200), (37, 5000), (74, 20000)):
        big = rs.uniform(-2, 2, (B, prob.D))
        big[pre:pre + 74] = base
        _, Zh, sg = prob.transformed(big)
        assert np.array_equal(Zh[pre:pre + 74], Zh0) and np.array_equal(sg[pre:pre + 74], sg0), (pre, B)
    prob.close()


@functools.lru_cache(maxsize=None)
def _run(chains, n_draws):
    """One sampler run of N_SPECTRA x chains units, kept open: (sampler, problem, Z_hat, sigma_tot [G, S, 2 Nf] of the downloaded
    draws as `StanFit['Z_hat']` evaluates them -- `transformed` per fit --, z [G, 2 Nf])."""
    from bayes_drt_amd import _lib
    from bayes_drt_amd import parallel as par
    from bayes_drt_amd.engine import Sampler
    prob, pk = _problem()
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    spec, chain = par.make_units(N_SPECTRA, chains)
    smp = Sampler(prob, N_SPECTRA * chains, 30, n_draws, 21, ctrl, spec=spec, chain_ids=chain)
    smp.run()
    draws = smp.results()[0].reshape(N_SPECTRA, chains * n_draws, prob.D)
    tr = [prob.transformed(d) for d in draws]
    Zh, sg = np.stack([t[1] for t in tr]), np.stack([t[2] for t in tr])
    return smp, prob, Zh, sg, np.ascontiguousarray(pk['Z'], dtype=float)


def _cols(part, nf):
    return {'both': slice(0, 2 * nf), 'real': slice(0, nf), 'imag': slice(nf, 2 * nf)}[part]


@functools.lru_cache(maxsize=None)
def _host(chains, n_draws, unit, part):
    """(Z_hat, sigma_tot, z of the part's columns, ll) of a run: the inputs of the host path."""
    from bayes_drt_amd.loo import pointwise_log_lik
    _, prob, Zh, sg, z = _run(chains, n_draws)
    c = _cols(part, prob.nf)
    a = tuple(np.ascontiguousarray(v) for v in (Zh[:, :, c], sg[:, :, c], z[:, c]))
    return a + (pointwise_log_lik(*a, unit=unit),)


def _assert_equal(dev, host, fields, what):
    for k in fields:
        assert dev[k].shape == host[k].shape and dev[k].dtype == host[k].dtype, (what, k)
        assert np.array_equal(dev[k], host[k], equal_nan=True), (what, k)


@pytest.mark.parametrize('unit,part', UNIT_PART)
@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_device_path_equals_host_path_bit_for_bit(chains, n_draws, unit, part):
    from bayes_drt_amd.loo import PREDICT_FIELDS, psis_loo, psis_predict
    smp = _run(chains, n_draws)[0]
    Zh, sg, z, ll = _host(chains, n_draws, unit, part)
    U = ll.shape[2]
    assert U == {'frequency': smp.problem.nf, 'point': z.shape[1]}[unit]
    arr = np.exp(np.random.default_rng(n_draws + U).uniform(np.log(0.05), np.log(3.0), (N_SPECTRA, U)))
    for reff in (None, 0.37, arr):
        dev = smp.loo(0, smp.n_units, chains, unit=unit, part=part, reff=reff)
        _assert_equal(dev, psis_loo(ll, reff), LOO_FIELDS, ('loo', np.ndim(reff)))
        assert np.array_equal(dev['reff'], np.broadcast_to(1.0 if reff is None else reff, (N_SPECTRA, U)))
        devp = smp.loo_predict(0, smp.n_units, chains, unit=unit, part=part, reff=reff)
        _assert_equal(devp, psis_predict(Zh, sg, z, unit, reff), PREDICT_FIELDS + ('pareto_k', 'n_tail'), ('predict', np.ndim(reff)))
        assert np.array_equal(devp['reff'], dev['reff'])
        assert np.array_equal(devp['pareto_k'], dev['pareto_k']) and np.array_equal(devp['n_tail'], dev['n_tail'])
    assert np.all(np.isfinite(dev['elpd_loo']))
    if chains * n_draws == 1000:                     # (S / 5 = 200 against 3 sqrt(S / reff): the array's entries give both)
        assert len(set(dev['n_tail'].ravel().tolist())) > 1


@pytest.mark.parametrize('unit,part', UNIT_PART)
@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_auto_relative_efficiency(chains, n_draws, unit, part):
    """Largest relative deviation of the device's reff from `relative_efficiency` measured on the MI355X over these eight cases:
    1.39e-15, at (4, 250, 'point', 'both'); reff 0.0024 ... 0.055; no entry at 1 in either path (profiles/loo_device/parity.txt)."""
    from bayes_drt_amd.loo import PREDICT_FIELDS, psis_loo, psis_predict, relative_efficiency
    smp = _run(chains, n_draws)[0]
    Zh, sg, z, ll = _host(chains, n_draws, unit, part)
    dev = smp.loo(0, smp.n_units, chains, unit=unit, part=part, reff='auto')
    r = dev['reff']
    assert r.shape == ll[:, 0].shape and np.all(np.isfinite(r) & (r > 0))
    _assert_equal(dev, psis_loo(ll, r), LOO_FIELDS, 'loo')
    devp = smp.loo_predict(0, smp.n_units, chains, unit=unit, part=part, reff='auto')
    assert np.array_equal(devp['reff'], r)
    _assert_equal(devp, psis_predict(Zh, sg, z, unit, r), PREDICT_FIELDS + ('pareto_k', 'n_tail'), 'predict')
    ref = relative_efficiency(ll, chains)
    rel = np.abs(r - ref) / ref
    print('reff auto %s: largest relative deviation %.3g; reff %.3g ... %.3g; entries at 1: %d device, %d host'
          % ((chains, n_draws, unit, part), rel.max(), r.min(), r.max(), int(np.sum(r == 1.0)), int(np.sum(ref == 1.0))))
    assert np.array_equal(r == 1.0, ref == 1.0)
    assert rel.max() <= TOL_REFF
    assert len(np.unique(r)) > 1


@pytest.mark.parametrize('chains,n_draws', RUNS)
def test_chunks_and_unit_ranges(chains, n_draws):
    """One group per chunk and two of three (a ragged last chunk) against the single chunk; the middle spectrum alone against
    its row of the full call."""
    smp = _run(chains, n_draws)[0]
    lib, n2 = smp._lib, 2 * smp.problem.nf
    for name, predict in (('loo', 0), ('loo_predict', 1)):
        call = getattr(smp, name)
        for reff, mode in ((None, 0), ('auto', 2)):
            per = int(lib.bdrt_sampler_loo_group_bytes(smp.handle, chains, 1, n2, mode, predict))
            assert per > chains * n_draws * (smp.problem.D + 2 * n2) * 8
            full = call(0, smp.n_units, chains, reff=reff)
            for budget in (per, 2 * per + per // 2, 1):              # (1: a group that alone exceeds the budget is a chunk of one)
                got = call(0, smp.n_units, chains, reff=reff, chunk_bytes=budget)
                _assert_equal(got, full, tuple(full), (name, reff, budget))
            mid = call(chains, 2 * chains, chains, reff=reff)
            for k in full:
                assert np.array_equal(mid[k][0], full[k][1], equal_nan=True), (name, reff, k)


def test_refusals():
    from bayes_drt_amd import _lib
    from bayes_drt_amd.engine import Sampler
    chains, n_draws = RUNS[0]
    smp, prob = _run(chains, n_draws)[:2]
    n2 = 2 * prob.nf
    for call in (smp.loo, smp.loo_predict):
        with pytest.raises(ValueError, match='do not split into groups of 2 chains'):
            call(0, 3, chains)
        with pytest.raises(ValueError, match='do not split'):
            call(0, smp.n_units + chains, chains)
        with pytest.raises(ValueError, match="unit='frequency' needs part='both'"):
            call(0, smp.n_units, chains, part='real')
        with pytest.raises(ValueError, match='reff must be positive and finite'):
            call(0, smp.n_units, chains, reff=-1.0)
    # the library refuses the same on its own
    out = [np.empty((N_SPECTRA, n2)) for _ in range(5)]
    nt = np.empty((N_SPECTRA, n2), dtype=np.int32)
    args = [_lib.ptr(o) for o in out[:4]] + [_lib.ptr(nt), _lib.ptr(out[4])]
    lib = smp._lib
    assert lib.bdrt_sampler_loo(smp.handle, 0, 3, chains, 0, 0, n2, 0, None, 0, *args) == -1
    assert b'bdrt_sampler_loo: bad unit range' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_loo(smp.handle, 0, 2 * chains, chains, 1, 0, prob.nf, 0, None, 0, *args) == -1
    assert b'pair = 1 needs all' in lib.bdrt_last_error()
    assert lib.bdrt_sampler_loo(smp.handle, 0, 2 * chains, chains, 0, prob.nf, prob.nf + 1, 0, None, 0, *args) == -1
    assert lib.bdrt_sampler_loo(smp.handle, 0, 2 * chains, chains, 0, 0, n2, 1, None, 0, *args) == -1
    # chains of two spectra are no group
    assert lib.bdrt_sampler_loo(smp.handle, 1, 1 + chains, chains, 0, 0, n2, 0, None, 0, *args) == -1
    assert b'different spectra' in lib.bdrt_last_error()
    # a sampler without draws
    with Sampler(prob, 2, 5, 0, 3, spec=[0, 0]) as empty:
        for call in (empty.loo, empty.loo_predict):
            with pytest.raises(ValueError, match='holds no draws'):
                call(0, 2, 2)
        assert lib.bdrt_sampler_loo(empty.handle, 0, 2, 2, 0, 0, n2, 0, None, 0, *args) == -1
        assert b'bdrt_sampler_loo: bad unit range' in lib.bdrt_last_error()


def test_sample_units_appends_the_reductions():
    from bayes_drt_amd import _lib
    from bayes_drt_amd import parallel as par
    from bayes_drt_amd.engine import sample_units
    chains, n_draws = RUNS[0]
    smp, prob = _run(chains, n_draws)[:2]
    ctrl = _lib.NutsControl()
    prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    spec, chain = par.make_units(N_SPECTRA, chains)
    res = sample_units(prob, N_SPECTRA * chains, 30, n_draws, 21, ctrl, spec=spec, chain_ids=chain, diagnostics_chains=chains,
                       loo=dict(chains=chains, predict=True, unit='point', reff=0.5))
    assert len(res) == 3 and set(res.loo) == {'loo', 'predict'} and len(res.diagnostics) == 4 and res.heldout is None
    assert np.array_equal(res[0], smp.results()[0])
    _assert_equal(res.loo['loo'], smp.loo(0, smp.n_units, chains, unit='point', reff=0.5), LOO_FIELDS + ('reff',), 'loo')
    ref = smp.loo_predict(0, smp.n_units, chains, unit='point', reff=0.5)
    _assert_equal(res.loo['predict'], ref, tuple(ref), 'predict')
    bare = sample_units(prob, 2, 5, 5, 1, ctrl, spec=[0, 0])
    assert len(bare) == 3 and bare.diagnostics is None and bare.loo is None and bare.heldout is None


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


def test_fit_many_stores_what_loo_many_would():
    """Three spectra on one grid and a fourth on a shorter one (a second engine call, which reduces its own view)."""
    from bayes_drt_amd.inversion import Inverter
    fs, zs = zip(*[_spectrum(n) for n in NAMES])
    fs, zs = list(fs) + [fs[0][4:]], [np.array(Z) for Z in zs] + [np.array(zs[0][4:])]
    kw = dict(mode='sample', warmup=40, samples=40, chains=3, random_seed=8, check_outliers=False, check_diagnostics=False)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        views = Inverter(basis_freq=BASIS).fit_many(fs, zs, loo=True, loo_predict=True, loo_kw=dict(reff=None), **kw)
        plain = Inverter(basis_freq=BASIS).fit_many(fs[:1], zs[:1], **kw)
    assert all(not hasattr(v, 'loo_result') and not hasattr(v, 'loo_predict_result') for v in plain)
    cp = [copy.copy(v) for v in views]
    many = Inverter.loo_many(cp[:3], reff=None) + Inverter.loo_many(cp[3:], reff=None)
    pred = Inverter.loo_predict_many(cp[:3], reff=None) + Inverter.loo_predict_many(cp[3:], reff=None)
    for v, c, m, p in zip(views, cp, many, pred):
        assert v.loo_result is not c.loo_result and c.loo_result is m
        assert type(v.loo_result) is type(m) and type(v.loo_predict_result) is type(p)
        _equal_results(v.loo_result, m)
        _equal_results(v.loo_predict_result, p)
    assert views[3].loo_result.n_units == len(fs[3]) and views[0].loo_result.n_draws == 120


def test_fit_stores_what_loo_would():
    from bayes_drt_amd.inversion import Inverter
    f, Z = _spectrum(NAMES[0])
    inv = Inverter(basis_freq=BASIS)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        inv.fit(f, Z, mode='sample', warmup=40, samples=40, chains=3, random_seed=3, check_diagnostics=False, loo=True,
                loo_predict=True, loo_kw=dict(reff=None, unit='point'))
    got, gotp = inv.loo_result, inv.loo_predict_result
    _equal_results(got, inv.loo(unit='point', reff=None))
    _equal_results(gotp, inv.loo_predict(unit='point', reff=None))
    assert got.n_units == 2 * len(f) and got.n_draws == 120
