"""parallel.sample_sharded(..., diagnostics=True) on 2 ranks (gloo, one device): the per-rank device reductions of n_eff / Rhat,
gathered per spectrum, equal path (b) (bdrt_diagnostics) on the draws the same run gathers, bit for bit."""
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _run(world, n_spectra, chains, gather):
    import torch.multiprocessing as mp
    from tests.diag_sharded_worker import rank_main
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=rank_main, args=(r, world, port, n_spectra, chains, gather, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=400)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return out


@pytest.mark.timeout(600)
@pytest.mark.parametrize('n_spectra,chains', [(3, 2), (1, 4)])
def test_sharded_diagnostics_equal_host_path_on_gathered_draws(n_spectra, chains):
    from bayes_drt_amd.diagnostics import column_diagnostics
    from bayes_drt_amd.model import Problem
    from tests.diag_sharded_worker import problem_kwargs
    res = _run(2, n_spectra, chains, 'draws')
    summ = _run(2, n_spectra, chains, 'summary')
    pk = problem_kwargs(n_spectra)
    prob = Problem(pk['blocks'], pk['Z'], pk['freq'], sigma_min=pk['sigma_min'], ups_alpha=1.0, ups_beta=0.1)
    D, n_draws = prob.D, res['draws'].shape[1]
    _, _, ne, rh = column_diagnostics(res['draws'].reshape(n_spectra, chains * n_draws, D), chains, is_pos=prob.is_pos)
    prob.close()
    assert res['n_eff'].shape == (n_spectra, D) and res['Rhat'].shape == (n_spectra, D)
    assert np.array_equal(res['n_eff'], ne, equal_nan=True) and np.array_equal(res['Rhat'], rh, equal_nan=True)
    assert 'draws' not in summ
    assert np.array_equal(summ['n_eff'], ne, equal_nan=True) and np.array_equal(summ['Rhat'], rh, equal_nan=True)
    assert np.array_equal(summ['mean'], res['mean'])
