"""parallel.sample_sharded(..., loo=..., rank_diagnostics=True) on spawned ranks (gloo, one device): `loo`, `loo_predict` and the
rank-normalised diagnostics of gather='draws' and of gather='summary' equal the host path (`loo.host_psis_loo`,
`loo.host_psis_predict`, `diagnostics.rank_diagnostics`) on the draws the same run gathered, bit for bit, on every rank.
World 2 with (3 spectra, 2 chains): every rank reduces its own units on its device.  World 2 with (1 spectrum, 4 chains): fewer
spectra than ranks, every rank reduces the gathered draws on the host path.  World 3 with 5 spectra: a ragged partition."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _run(world, n_spectra, chains):
    import torch.multiprocessing as mp
    from tests.loo_sharded_worker import rank_main
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=rank_main, args=(r, world, port, n_spectra, chains, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=400) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return got


@pytest.mark.timeout(600)
@pytest.mark.parametrize('world,n_spectra,chains', [(2, 3, 2), (2, 1, 4), (3, 5, 2)])
def test_sharded_loo_equals_host_path_on_gathered_draws(world, n_spectra, chains):
    from bayes_drt_amd import loo as L
    from bayes_drt_amd.diagnostics import rank_diagnostics
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    from tests.loo_sharded_worker import LOO, flatten
    got = _run(world, n_spectra, chains)
    assert sorted(got) == list(range(world))
    res, summ = got[0]['draws'], got[0]['summary']
    pk = problem_kwargs(n_spectra)
    prob = Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'], ups_alpha=1.0, ups_beta=0.1)
    D, n_draws = prob.D, res['draws'].shape[1]
    blocks = res['draws'].reshape(n_spectra, chains * n_draws, D)
    ref = flatten({'loo': L.host_psis_loo(prob, blocks, pk['Z'], chains, reff=LOO['reff']),
                   'loo_predict': L.host_psis_predict(prob, blocks, pk['Z'], chains, reff=LOO['reff']),
                   'rank': rank_diagnostics(blocks, chains, is_pos=prob.is_pos)})
    nf = prob.nf
    prob.close()
    assert ref['loo/elpd_loo'].shape == (n_spectra, nf) and ref['loo_predict/mean'].shape == (n_spectra, 2 * nf)
    assert ref['rank/rhat'].shape == (n_spectra, D) and np.all(np.isfinite(ref['loo/elpd_loo']))
    assert 'draws' not in summ
    for name, out in (('draws', res), ('summary', summ)):
        assert {k for k in out if '/' in k} == set(ref), name
        for k, v in ref.items():
            assert out[k].shape == v.shape and out[k].dtype == v.dtype, (name, k)
            assert np.array_equal(out[k], v, equal_nan=True), (name, k)
    assert np.array_equal(summ['mean'], res['mean'])
    # identical on every rank
    for r in range(1, world):
        for name in ('draws', 'summary'):
            assert set(got[r][name]) == set(got[0][name]) - {'draws'}, (r, name)
            for k, v in got[r][name].items():
                assert np.array_equal(v, got[0][name][k], equal_nan=True), (r, name, k)
