"""Rank process of tests/test_gpu_diagnostics_sharded.py: a gloo group of `world` ranks on the box's one device, each rank with
the real GPU worker, running parallel.sample_sharded(..., diagnostics=True); rank 0 hands the result to the parent."""
import os

import numpy as np


def problem_kwargs(n_spectra):
    from tests.helpers import load
    d = load('dat_sample_2ZARC_uniform_0.25_K81')
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=True)
    rs = np.random.RandomState(2)
    Z = np.stack([d['Z'] * (1 + 0.01 * k) + 0.002 * rs.standard_normal(d['Z'].shape) for k in range(n_spectra)])
    return dict(blocks=[blk], Z=Z, freq=d['freq'], sigma_min=float(d['sigma_min']), ups_alpha=1.0, ups_beta=0.1, induc_scale=1.0)


def rank_main(rank, world, port, n_spectra, chains, gather, q):
    import torch.distributed as dist
    from bayes_drt_amd import parallel as par
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        pk = problem_kwargs(n_spectra) if rank == 0 else None
        res = par.sample_sharded(pk, n_spectra, chains, 30, 40, seed=21, control={'max_treedepth': 5}, gather=gather,
                                 diagnostics=True)
        if rank == 0:
            q.put({k: np.asarray(v) for k, v in res.items()})
    finally:
        dist.destroy_process_group()
