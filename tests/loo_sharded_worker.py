"""Rank process of tests/test_gpu_loo_sharded.py: a gloo group of `world` ranks on the box's one device, each rank with the real
GPU worker, running parallel.sample_sharded(..., loo=..., rank_diagnostics=True) once per gather mode in the same group; every
rank hands its results to the parent (they must be identical)."""
import os

import numpy as np

LOO = dict(loo=True, predict=True, reff=None)
RUN = dict(warmup=30, n_draws=40, seed=21, control={'max_treedepth': 5})


def flatten(res):
    """{'loo': {'lpd': a}} -> {'loo/lpd': a}: plain arrays for the queue."""
    out = {}
    for k, v in res.items():
        if isinstance(v, dict):
            out.update({'%s/%s' % (k, kk): np.asarray(vv) for kk, vv in v.items()})
        else:
            out[k] = np.asarray(v)
    return out


def rank_main(rank, world, port, n_spectra, chains, q):
    import torch.distributed as dist
    from bayes_drt_amd import parallel as par
    from tests.diag_sharded_worker import problem_kwargs
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        pk = problem_kwargs(n_spectra) if rank == 0 else None
        out = {}
        for gather in ('draws', 'summary'):
            res = par.sample_sharded(pk, n_spectra, chains, RUN['warmup'], RUN['n_draws'], seed=RUN['seed'], control=RUN['control'],
                                     gather=gather, loo=LOO, rank_diagnostics=True)
            out[gather] = flatten(res)
        if rank > 0:
            out['draws'].pop('draws')                # (rank 0's copy is enough for the parent; the rest is compared)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()
