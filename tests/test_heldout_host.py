"""Held-out prediction, K-fold and exact refits: what needs no GPU.

  * the yardstick (tests/heldout_numpy.py), evaluated at the training grid of a golden Stan data dict of each family, reproduces
    the CPU oracle's Z_hat and sigma_tot for random parameter rows;
  * fold assignment (`loo.fold_labels`), result assembly from fabricated arrays (`loo.heldout_result`, `loo.kfold_result`,
    `loo.reloo_result`, ranked by `loo.compare`);
  * every ValueError and NotImplementedError of the new entry points fires before the library is loaded."""
import numpy as np
import pytest

from tests import heldout_cases as hc
from tests import heldout_numpy as hn

# The oracle and the yardstick are two float64 statements of the same sums of K <= 101 terms: they differ by rounding alone, a few
# K u relative to the largest entry at worst (1e-13); a wrong term of either shows at 1e-3.
TOL_ORACLE = 1e-12


@pytest.mark.parametrize('name', sorted(hc.FAMILIES))
def test_yardstick_reproduces_the_oracle_on_the_training_grid(name):
    from oracle import oracle as orc
    kw = hc.family(name)['kw']
    om = orc.OracleModel(**kw)
    assert om.D == hn.layout(om.Ks)['D'] and om.layout()['x'] == hn.layout(om.Ks)['x'] and om.layout()['err'] == hn.layout(om.Ks)['err']
    f, A = hc.train_grid(name)
    P = hc.rows(name, 5, seed=3)
    Zh, sg = hn.transformed(kw['blocks'], P, f, A, kw['sigma_min'], kw['induc_scale'])
    for i, p in enumerate(P):
        ref = om.forward(om.unconstrain(p))
        for got, want in ((Zh[i], ref['Z_hat']), (sg[i], ref['sigma_tot'])):
            assert np.max(np.abs(got - want)) <= TOL_ORACLE * np.max(np.abs(want)), (name, i)


def test_yardstick_sums_and_types_agree():
    """The explicit forward and reversed sums and the np.longdouble statement are the float64 statement up to rounding."""
    name = 'Series-2Parallel_pos'
    kw = hc.family(name)['kw']
    f, A = hc.grid(name, 3)
    P = hc.rows(name, 7)
    args = (kw['blocks'], P, f, A, kw['sigma_min'], kw['induc_scale'])
    base = hn.transformed(*args)
    for other in (hn.transformed(*args, reverse=False), hn.transformed(*args, reverse=True),
                  hn.transformed(*args, dtype=np.longdouble)):
        for a, b in zip(base, other):
            assert a.shape == (7, 6) and np.max(np.abs(a - b.astype(float))) <= 1e-13 * np.max(np.abs(a))
    Zh, sg, eZ, eS, how = hc.calibrate(name, P, f, A)
    assert np.array_equal(Zh, base[0]) or not hc.LONGDOUBLE
    assert 0 < eZ < 1e-14 and 0 < eS < 1e-14 and how in ('longdouble', 'reversed summation')


def test_yardstick_reduce_is_the_equal_weight_mixture():
    """lpd against a direct evaluation of the mixture density; the moments are `loo_predict_numpy`'s *_post."""
    from tests import loo_predict_numpy as lp
    rs = np.random.default_rng(2)
    S, N2 = 57, 6
    mu, sg, z = rs.normal(size=(S, N2)), np.exp(rs.normal(-1, 0.3, (S, N2))), rs.normal(size=N2)
    sg[:, 2] = np.nan                                                        # unit 2 of 'frequency', scalar 2 of 'point'
    for unit in ('frequency', 'point'):
        got, ref = hn.reduce(mu, sg, z, unit), lp.predict(mu, sg, z, unit)
        for k in hn.FIELDS:
            assert np.array_equal(got[k], ref[k + '_post'], equal_nan=True), (unit, k)
        dens = np.exp(-0.5 * ((z - mu) / sg) ** 2) / (sg * np.sqrt(2 * np.pi))
        if unit == 'frequency':
            dens = dens[:, :3] * dens[:, 3:]
        want = np.log(dens.mean(axis=0))
        assert np.isnan(got['lpd'][2]) and np.sum(np.isnan(got['lpd'])) == 1
        ok = np.isfinite(want)
        assert np.allclose(got['lpd'][ok], want[ok], rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------- fold assignment
def test_fold_labels_interleave_the_sorted_grid():
    from bayes_drt_amd.loo import fold_labels
    f = np.logspace(5, -1, 23)
    lab = fold_labels(f, 5)
    assert np.array_equal(lab, np.arange(23) % 5)                            # already descending
    perm = np.random.default_rng(0).permutation(23)
    lab_p = fold_labels(f[perm], 5)
    assert np.array_equal(lab_p, lab[perm])                                  # the fold goes with the frequency, not the position
    assert np.array_equal(fold_labels(f[::-1], 5), lab[::-1])
    for k in (2, 3, 10, 23):
        lab = fold_labels(f[perm], k)
        assert lab.shape == (23,) and set(lab.tolist()) == set(range(k))     # every frequency in exactly one fold, none empty
        for j in range(k):                                                   # every fold spans the whole range
            assert np.array_equal(np.sort(f[perm][lab == j])[::-1], f[j::k])
    assert np.array_equal(fold_labels(f, np.int64(4)), np.arange(23) % 4)


def test_fold_labels_accepts_label_arrays_and_refuses():
    from bayes_drt_amd.loo import fold_labels
    f = np.logspace(3, 0, 7)
    given = np.array([3, 3, 0, 7, 0, 7, 3])
    assert np.array_equal(fold_labels(f, given), given)
    assert np.array_equal(fold_labels(f, [0.0, 1.0, 0, 1, 0, 1, 0]), [0, 1, 0, 1, 0, 1, 0])
    for bad, msg in ((1, 'at least 2'), (0, 'at least 2'), (2.5, 'at least 2'), (8, 'would be empty'),
                     (np.zeros(7, dtype=int), 'no training data'), (np.arange(6), '6 fold labels for 7'),
                     (np.zeros((7, 1), dtype=int), 'fold labels for 7'), ([0.5, 1, 0, 1, 0, 1, 0], 'integers')):
        with pytest.raises(ValueError, match=msg):
            fold_labels(f, bad)


# ---------------------------------------------------------------------------------------------------- result assembly
def _fake_reduce(H, ncols, U, seed):
    rs = np.random.default_rng(seed)
    return dict(lpd=rs.normal(-1, 1, U), mean=rs.normal(size=ncols), sd=np.exp(rs.normal(size=ncols)), pit=rs.uniform(size=ncols))


def test_heldout_result_units_scale_and_parts():
    from bayes_drt_amd.loo import heldout_result
    H, sc = 4, 7.5
    f = np.array([30.0, 2.0, 500.0, 0.1])
    z = np.random.default_rng(1).normal(size=2 * H)
    p = _fake_reduce(H, 2 * H, H, 0)
    r = heldout_result(p, z, f, 'both', 'frequency', 80, sc)
    assert np.array_equal(r.frequencies, f) and r.n_draws == 80
    assert np.array_equal(r.elpd_i, p['lpd'] - 2 * np.log(sc)) and r.elpd == float(np.sum(r.elpd_i))
    assert np.array_equal(r.Z_pred, (p['mean'][:H] + 1j * p['mean'][H:]) * sc)
    assert np.array_equal(r.sigma_pred_re, p['sd'][:H] * sc) and np.array_equal(r.sigma_pred_im, p['sd'][H:] * sc)
    assert np.array_equal(r.pit_re, p['pit'][:H]) and np.array_equal(r.pit_im, p['pit'][H:])
    assert np.array_equal(r.resid_im, ((z - p['mean']) / p['sd'])[H:])
    pp = _fake_reduce(H, 2 * H, 2 * H, 1)
    r = heldout_result(pp, z, f, 'both', 'point', 80, sc)
    assert np.array_equal(r.elpd_i, pp['lpd'] - np.log(sc)) and len(r.elpd_i) == 2 * H
    pi = _fake_reduce(H, H, H, 2)
    r = heldout_result(pi, z[H:], f, 'imag', 'point', 80, sc)
    assert np.all(np.isnan(r.Z_pred.real)) and np.array_equal(r.Z_pred.imag, pi['mean'] * sc)
    assert np.all(np.isnan(r.sigma_pred_re)) and np.all(np.isnan(r.pit_re)) and np.array_equal(r.resid_im, (z[H:] - pi['mean']) / pi['sd'])
    with pytest.raises(ValueError, match="needs part='both'"):
        heldout_result(pi, z[H:], f, 'imag', 'frequency', 80, sc)
    with pytest.raises(ValueError, match='do not fit'):
        heldout_result(pi, z, f, 'both', 'frequency', 80, sc)


def _fake_folds(f, labels, unit, seed):
    from bayes_drt_amd.loo import heldout_result
    out = {}
    for lab in np.unique(labels).tolist():
        idx = np.nonzero(labels == lab)[0]
        H = len(idx)
        p = _fake_reduce(H, 2 * H, H if unit == 'frequency' else 2 * H, seed + lab)
        out[lab] = heldout_result(p, np.zeros(2 * H), f[idx], 'both', unit, 60 + lab, 2.0)
    return out


def test_kfold_result_is_in_grid_order_and_compare_ranks_it():
    from bayes_drt_amd.loo import compare, fold_labels, kfold_result
    f = np.logspace(4, -1, 11)[np.random.default_rng(3).permutation(11)]
    labels = fold_labels(f, 3)
    folds = _fake_folds(f, labels, 'frequency', 0)
    r = kfold_result(labels, folds)
    assert r.method == 'kfold' and r.n_units == 11 and np.array_equal(r.fold, labels) and np.array_equal(r.frequencies, f)
    for lab, fr in folds.items():
        idx = np.nonzero(labels == lab)[0]
        assert np.array_equal(r.elpd_i[idx], fr.elpd_i) and np.array_equal(r.Z_pred[idx], fr.Z_pred)
        assert np.array_equal(r.pit_im[idx], fr.pit_im) and np.array_equal(r.sigma_pred_re[idx], fr.sigma_pred_re)
    assert r.elpd_loo == float(np.sum(r.elpd_i)) and r.se == float(np.sqrt(11 * np.var(r.elpd_i)))
    assert np.isnan(r.p_loo) and np.all(np.isnan(r.pareto_k)) and r.pareto_k.shape == (11,) and r.n_bad_k == 0 and r.n_draws == 60
    other = kfold_result(labels, _fake_folds(f, labels, 'frequency', 50))
    rows = compare({'a': r, 'b': other})
    best = max((r, other), key=lambda x: x.elpd_loo)
    assert rows[0]['elpd_loo'] == best.elpd_loo and rows[0]['elpd_diff'] == 0.0 and rows[1]['elpd_diff'] < 0
    assert rows[1]['dse'] == float(np.sqrt(11 * np.var(r.elpd_i - other.elpd_i)))
    # points: real halves, then imaginary halves, each in grid order
    pf = _fake_folds(f, labels, 'point', 7)
    rp = kfold_result(labels, pf, unit='point')
    assert rp.n_units == 22 and np.array_equal(rp.fold, np.concatenate([labels, labels]))
    for lab, fr in pf.items():
        idx = np.nonzero(labels == lab)[0]
        assert np.array_equal(rp.elpd_i[idx], fr.elpd_i[:len(idx)]) and np.array_equal(rp.elpd_i[11 + idx], fr.elpd_i[len(idx):])
    with pytest.raises(ValueError, match='different numbers of observations'):
        compare({'a': r, 'p': rp})
    with pytest.raises(ValueError, match='folds'):
        kfold_result(labels, {k: v for k, v in folds.items() if k != 1})


def _fake_loo(n, seed=0):
    from bayes_drt_amd import loo
    rs = np.random.default_rng(seed)
    k = rs.uniform(-0.2, 0.6, n)
    k[[2, 5, 9]] = [0.9, 1.4, 0.75]
    p = dict(lpd=rs.normal(2, 1, n), p_waic=rs.uniform(0, 1, n), pareto_k=k, n_tail=np.full(n, 12, dtype=np.int32))
    p['elpd_loo'] = p['lpd'] - rs.uniform(0, 1, n)
    p['p_loo'], p['elpd_waic'] = p['lpd'] - p['elpd_loo'], p['lpd'] - p['p_waic']
    was = loo.logger.disabled
    loo.logger.disabled = True
    try:
        return loo._result(p, 2, 100, np.log(3.0))
    finally:
        loo.logger.disabled = was


def test_reloo_bookkeeping():
    from bayes_drt_amd.loo import reloo_candidates, reloo_result
    r = _fake_loo(12)
    assert r.n_bad_k == 3 and reloo_candidates(r).tolist() == [2, 5, 9]
    assert reloo_candidates(r, 1.0).tolist() == [5] and len(reloo_candidates(r, -np.inf, None)) == 12
    with pytest.raises(ValueError, match='kfold'):
        reloo_candidates(r, 0.7, 2)
    assert reloo_candidates(r, 0.7, 3).tolist() == [2, 5, 9]
    new = reloo_result(r, {2: -4.0, 5: -6.5})
    assert new is not r and 'refit' not in r and r.elpd_i[2] != -4.0                    # the old result is left as it was
    assert new.refit.tolist() == [i in (2, 5) for i in range(12)] and new.method == 'psis+refit'
    assert new.elpd_i[2] == -4.0 and new.elpd_i[5] == -6.5
    keep = ~new.refit
    assert np.array_equal(new.elpd_i[keep], r.elpd_i[keep])
    for k in ('lpd_i', 'pareto_k', 'p_waic_i', 'n_tail'):
        assert np.array_equal(new[k], r[k]), k
    for k in ('elpd_waic', 'p_waic', 'se_waic', 'n_units', 'n_draws'):
        assert new[k] == r[k], k
    assert new.elpd_loo == float(np.sum(new.elpd_i)) and new.se == float(np.sqrt(12 * np.var(new.elpd_i)))
    assert new.p_loo == float(np.sum(r.lpd_i - new.elpd_i)) and new.n_bad_k == 1     # unit 9 is above 0.7 and was not refit
    assert reloo_result(r, {}).n_bad_k == 3 and not reloo_result(r, {}).refit.any()
    with pytest.raises(ValueError):
        reloo_result(r, {12: 0.0})


# ---------------------------------------------------------------------------------------------------- refusals without the library
class _FakeDat:
    outlier_mode = 0


class _FakeProblem:
    def __init__(self, Ks=(5, 4), outlier_mode=0):
        self.Ks, self.D, self.nf = list(Ks), 2 + 2 * sum(Ks) + 4 + 3 * len(Ks), 9
        self.dat = _FakeDat()
        self.dat.outlier_mode = outlier_mode


class _FakeSampler:
    def __init__(self, problem, n_units=6, n_draws=10):
        self.problem, self.n_units, self.n_draws, self.handle, self._lib = problem, n_units, n_draws, None, None


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
    from bayes_drt_amd.engine import sample_units
    prob, H = _FakeProblem(), 3
    f = np.array([10.0, 1.0, 0.1])
    A = [np.zeros((2 * H, 5)), (np.zeros((H, 4)), np.zeros((H, 4)))]
    par = np.ones((2, prob.D))
    for args, msg in (((prob, par[:, :-1], f, A), r'params must be \[B, 30\]'), ((prob, par, f, A[:1]), '1 blocks of prediction rows'),
                      ((prob, par, f, [A[0], np.zeros((2 * H, 5))]), 'block 1: prediction rows'),
                      ((prob, par, f[:2], A), 'block 0: prediction rows'), ((prob, par, [1.0, -2.0, 3.0], A), 'positive finite'),
                      ((prob, par, [], A), 'positive finite')):
        with pytest.raises(ValueError, match=msg):
            loo.heldout_transformed(*args)
    with pytest.raises(NotImplementedError, match='outlier error models'):
        loo.heldout_transformed(_FakeProblem(outlier_mode=2), par, f, A)
    Zh, z = np.ones((2, 5, 6)), np.zeros((2, 6))
    for args, msg in (((Zh, Zh[:, :4], z), 'do not fit'), ((Zh, Zh, z[:1]), 'do not fit'), ((Zh[:, :, :5], Zh[:, :, :5], z[:, :5]), 'even number'),
                      ((Zh[:, :1], Zh[:, :1], z), 'at least 2 draws')):
        with pytest.raises(ValueError, match=msg):
            loo.heldout_reduce(*args)
    with pytest.raises(ValueError, match="unit must be 'frequency' or 'point'"):
        loo.heldout_reduce(Zh, Zh, z, unit='scalar')
    smp = _FakeSampler(prob)
    zt = np.zeros((3, 2 * H))
    for kw, msg in ((dict(chains=4), 'do not split into groups of 4'), (dict(unit_hi=8), 'do not split'), (dict(part='real'), "needs part='both'"),
                    (dict(part='half'), "part must be"), (dict(unit='scalar'), "unit must be"), (dict(z_test=zt[:2]), r'z_test must be \[3, 6\]'),
                    (dict(z_test=zt[:, :H], unit='point', part='real'), r'z_test must be \[3, 6\]'), (dict(chunk_bytes=-1), 'chunk_bytes'),
                    (dict(A_test_blocks=A[:1]), 'blocks of prediction rows')):
        a = dict(unit_lo=0, unit_hi=6, chains=2, freq_test=f, A_test_blocks=A, z_test=zt)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            loo.sampler_heldout(smp, **a)
    with pytest.raises(ValueError, match='holds no draws'):
        loo.sampler_heldout(_FakeSampler(prob, n_draws=0), 0, 6, 2, f, A, zt)
    with pytest.raises(ValueError, match='at least 2 draws'):
        loo.sampler_heldout(_FakeSampler(prob, n_draws=1), 0, 6, 1, f, A, np.zeros((6, 2 * H)))
    with pytest.raises(NotImplementedError, match='outlier error models'):
        loo.sampler_heldout(_FakeSampler(_FakeProblem(outlier_mode=1)), 0, 6, 2, f, A, zt)
    with pytest.raises(ValueError, match=r'draws must be \[G, S, 30\]'):
        loo.host_heldout(prob, np.zeros((3, 20, 5)), 2, f, A, zt)
    with pytest.raises(ValueError, match='heldout needs chains'):
        sample_units(prob, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f))
    with pytest.raises(ValueError, match='heldout needs chains'):
        sample_units(prob, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt, reff=1))
    with pytest.raises(ValueError, match="needs part='both'"):
        sample_units(prob, 6, 5, 5, 1, heldout=dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt, part='imag'))


def test_heldout_request_is_complete_and_checked(no_library):
    from bayes_drt_amd import loo
    prob, H = _FakeProblem(), 3
    f, zt = np.array([10.0, 1.0, 0.1]), np.zeros((3, 2 * H))
    A = [np.zeros((2 * H, 5)), (np.zeros((H, 4)), np.zeros((H, 4)))]
    need = dict(chains=2, freq_test=f, A_test_blocks=A, z_test=zt)
    got = loo.heldout_request(need, prob, 'f')
    assert set(got) == set(loo.HELDOUT_KEYS) and all(got[k] is v for k, v in need.items())
    assert (got['unit'], got['part'], got['chunk_bytes'], got['sigma_out']) == ('frequency', 'both', None, None)
    given = dict(need, unit='point', part='imag', chunk_bytes=1 << 20)
    assert loo.heldout_request(given, prob, 'f') == dict(given, sigma_out=None)
    for k in need:
        with pytest.raises(ValueError, match='f: heldout needs chains, freq_test, A_test_blocks, z_test'):
            loo.heldout_request({j: v for j, v in need.items() if j != k}, prob, 'f')
    for kw, msg in ((dict(reff=1), 'heldout needs chains'), (dict(part='imag'), "needs part='both'"), (dict(unit='scalar'), 'unit must be'),
                    (dict(chunk_bytes=-1), 'chunk_bytes'), (dict(A_test_blocks=A[:1]), 'blocks of prediction rows'),
                    (dict(sigma_out='posterior'), 'sigma_out must be None'), (dict(sigma_out='prior'), 'needs an outlier error model')):
        with pytest.raises(ValueError, match=msg):
            loo.heldout_request(dict(need, **kw), prob, 'f')
    with pytest.raises(NotImplementedError, match='outlier error models'):
        loo.heldout_request(need, _FakeProblem(outlier_mode=1), 'f')


def test_fit_many_builds_every_held_request_before_the_first_batch(monkeypatch, no_library):
    """What only `_batch_jobs` can tell -- grids that differ in their last bits and share a batch, outliers='auto' that chose the
    outlier model -- is refused with no batch started, although an earlier batch was in order."""
    import copy
    from bayes_drt_amd.inversion import Inverter
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + 1j * 2 * np.pi * f * 1e-3)
    held = (f[:2], Z[:2])
    inv, started, jobs = Inverter(), [], []

    def fake_jobs(self, frequencies, Z_list, *a, **k):
        views = [copy.copy(self) for _ in Z_list]
        for v in views:
            v._Z_scale = 2.0
        return views, jobs
    monkeypatch.setattr(Inverter, '_batch_jobs', fake_jobs)
    monkeypatch.setattr(Inverter, '_fit_batch', staticmethod(lambda *a, **k: started.append(a)))
    monkeypatch.setattr(Inverter, '_fit_finish', lambda *a, **k: None)
    monkeypatch.setattr(Inverter, '_get_prediction_matrices',
                        lambda self, fr, names: {n: dict(A_re=np.zeros((len(fr), 4)), A_im=np.zeros((len(fr), 4))) for n in names})
    plain = dict(model_type='Series', outliers=False, sigma_min=0.002)
    jobs[:] = [dict(plain, batch_key='a'), dict(plain, batch_key='b'), dict(plain, batch_key='b')]
    grids = [f[2:], f[2:], np.nextafter(f[2:], np.inf)]                      # (the last two: one batch, told apart only by the bits)
    with pytest.raises(ValueError, match='must share f_test'):
        inv.fit_many(grids, [Z[2:]] * 3, mode='sample', heldout=[held, held, (f[:2][::-1], Z[:2][::-1])])
    assert started == []
    jobs[:] = [dict(plain, batch_key='a'), dict(plain, batch_key='b', outliers=True)]
    with pytest.raises(NotImplementedError, match='outlier error models'):
        inv.fit_many(f[2:], [Z[2:]] * 2, mode='sample', outliers='auto', heldout=held)
    assert started == []
    # in order: every batch starts with its finished request
    jobs[:] = [dict(plain, batch_key='a'), dict(plain, batch_key='b'), dict(plain, batch_key='a')]
    assert len(inv.fit_many(f[2:], [Z[2:]] * 3, mode='sample', heldout=held, heldout_unit='point')) == 3
    assert [a[11] for a in started] == [[0, 2], [1]]                         # (index)
    for a in started:
        h = a[13]
        assert set(h) == {'chains', 'freq_test', 'A_test_blocks', 'z_test', 'unit', 'part', 'sigma_out'} and h['sigma_out'] is None
        assert h['unit'] == 'point' and h['z_test'].shape == (len(a[11]), 4) and np.array_equal(h['z_test'][0], np.r_[Z[:2].real, Z[:2].imag] / 2.0)


def test_draw_limit_is_refused_on_the_host():
    from bayes_drt_amd import loo
    S = loo.max_draws() + 1
    with pytest.raises(ValueError, match='the kernel holds at most'):
        loo.heldout_reduce(np.ones((1, S, 2)), np.ones((1, S, 2)), np.zeros((1, 2)))
    prob = _FakeProblem()
    f, A = np.array([1.0]), [np.zeros((2, 5)), np.zeros((2, 4))]
    with pytest.raises(ValueError, match='the kernel holds at most'):
        loo.sampler_heldout(_FakeSampler(prob, n_units=2, n_draws=S), 0, 2, 1, f, A, np.zeros((2, 2)))


def test_inverter_refuses_before_the_library_loads(no_library):
    from bayes_drt_amd.inversion import Inverter
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + 1j * 2 * np.pi * f * 1e-3)
    inv = Inverter()
    held = (f[:2], Z[:2])
    with pytest.raises(ValueError, match="heldout needs the draws of mode='sample'"):
        inv.fit(f[2:], Z[2:], heldout=held)
    with pytest.raises(ValueError, match="heldout needs the draws of mode='sample'"):
        inv.fit_many(f[2:], [Z[2:]], mode='optimize', heldout=held)
    for call in (lambda **k: inv.fit(f[2:], Z[2:], **k), lambda **k: inv.fit_many(f[2:], [Z[2:], Z[2:]], **k)):
        with pytest.raises(NotImplementedError, match='outlier error models'):
            call(mode='sample', outliers=True, heldout=held)
        with pytest.raises(ValueError, match='same length'):
            call(mode='sample', heldout=(f[:2], Z[:3]))
        with pytest.raises(ValueError, match='heldout must be'):
            call(mode='sample', heldout=(f[:2], Z[:2], 'frequency'))
        with pytest.raises(ValueError, match='frequencies must be positive'):
            call(mode='sample', heldout=(-f[:2], Z[:2]))
        with pytest.raises(ValueError, match="unit must be"):
            call(mode='sample', heldout=held, heldout_unit='scalar')
    with pytest.raises(ValueError, match='one such pair per spectrum'):
        inv.fit_many(f[2:], [Z[2:], Z[2:]], mode='sample', heldout=[held])
    # spectra of one batch with different f_test: refused before the first batch is sampled
    with pytest.raises(ValueError, match='must share f_test'):
        inv.fit_many(f[2:], [Z[2:], Z[2:]], mode='sample', heldout=[held, (f[:2][::-1], Z[:2][::-1])])
    with pytest.raises(ValueError, match='must share f_test'):
        inv.fit_many([f[2:], f[3:], f[2:]], [Z[2:], Z[3:], Z[2:]], mode='sample', heldout=[held, held, (f[:1], Z[:1])])
    with pytest.raises(NotImplementedError, match='outlier error models'):
        inv.fit_many(f[2:], [Z[2:], Z[2:]], mode='sample', outliers=[False, True], heldout=held)
    # K-fold
    for folds, msg in ((1, 'at least 2'), (22, 'would be empty'), (np.zeros(21, dtype=int), 'no training data'), (np.arange(20), '20 fold labels for 21')):
        with pytest.raises(ValueError, match=msg):
            inv.kfold_many(f, [Z], folds=folds)
        with pytest.raises(ValueError, match=msg):
            inv.kfold(f, Z, folds=folds)
    with pytest.raises(ValueError, match="needs mode='sample'"):
        inv.kfold_many(f, [Z], folds=3, mode='optimize')
    with pytest.raises(NotImplementedError, match='outlier error models'):
        inv.kfold_many(f, [Z], folds=3, outliers=True)
    with pytest.raises(ValueError, match='is set by kfold itself'):
        inv.kfold_many(f, [Z], folds=3, heldout=held)
    with pytest.raises(ValueError, match="unit must be"):
        inv.kfold_many(f, [Z], folds=3, unit='scalar')
    assert inv.kfold_many(f, [], folds=3) == []
    # exact refits
    with pytest.raises(ValueError, match=r"loo\(unit='frequency', part='both'\)"):
        inv.reloo(f, Z)
    inv.loo_result, inv._loo_unit_part = _fake_loo(12), ('frequency', 'both')
    with pytest.raises(ValueError, match=r"loo\(unit='frequency', part='both'\)"):
        inv.reloo(f, Z)                                                      # 12 units for 21 frequencies
    inv.loo_result = _fake_loo(21)
    for up in (('point', 'real'), ('point', 'imag'), ('point', 'both'), None):           # as many units, but they are points
        inv._loo_unit_part = up
        with pytest.raises(ValueError, match=r"loo\(unit='frequency', part='both'\)"):
            inv.reloo(f, Z)
    inv._loo_unit_part = ('frequency', 'both')
    with pytest.raises(ValueError, match='kfold'):
        inv.reloo(f, Z, max_refits=2)
    with pytest.raises(NotImplementedError, match='outlier error models'):
        inv.reloo(f, Z, outliers=True)
    before = dict(inv.loo_result)
    got = inv.reloo(f, Z, k_threshold=2.0)                                   # nothing qualifies: no refit, no library
    assert got is inv.loo_result and not got.refit.any() and got.method == 'psis+refit' and got.n_bad_k == 3
    assert np.array_equal(got.elpd_i, before['elpd_i']) and got.elpd_loo == float(np.sum(before['elpd_i']))
    assert not hasattr(inv, 'kfold_result') and not hasattr(inv, 'heldout_result')


def test_heldout_pairs_may_be_sequences():
    from bayes_drt_amd.inversion import Inverter
    f, Z = np.array([10.0, 1.0]), np.array([1 + 1j, 2 - 1j])
    arg = Inverter._heldout_arguments
    for held in ((f, Z), (f.tolist(), Z.tolist()), [f.tolist(), Z], ([10.0, 1.0], [1 + 1j, 2 - 1j])):
        got = arg(held, 'frequency', 2, 'sample', 'both', [False, False], None)
        assert len(got['pairs']) == 2 and all(np.array_equal(p[0], f) and np.array_equal(p[1], Z) for p in got['pairs'])
    got = arg([(f.tolist(), Z.tolist()), (f[:1], Z[:1])], 'point', 2, 'sample', 'both', [False, False], None)
    assert [len(p[0]) for p in got['pairs']] == [2, 1] and got['unit'] == 'point'
    assert arg((f, Z), 'frequency', 1, 'sample', 'imag', [False], None)['unit'] == 'point'
    with pytest.raises(ValueError, match='heldout must be'):
        arg([(f, Z)], 'frequency', 2, 'sample', 'both', [False, False], None)


def test_heldout_is_refused_inside_a_process_group(monkeypatch, no_library):
    import torch.distributed as dist
    from bayes_drt_amd.inversion import Inverter
    monkeypatch.setattr(dist, 'is_available', lambda: True)
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    f = np.logspace(4, 0, 21)
    Z = 1.0 + 1.0 / (1.0 + 1j * 2 * np.pi * f * 1e-3)
    inv = Inverter()
    with pytest.raises(NotImplementedError, match='process group with more than one rank'):
        inv.fit_many(f[2:], [Z[2:]], mode='sample', heldout=(f[:2], Z[:2]))
    with pytest.raises(NotImplementedError, match='process group with more than one rank'):
        inv.kfold_many(f, [Z], folds=3)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 1)
    assert Inverter._heldout_arguments((f[:2], Z[:2]), 'frequency', 1, 'sample', 'both', [False], None) is not None
