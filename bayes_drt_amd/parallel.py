"""Multi-GPU execution: one process per GPU, units (spectrum, chain) sharded with NO data-path collective.

The path shards naturally: chains are independent given the data (the reference runs one process per
chain, bayes_drt/inversion.py:1218-1221) and spectra are independent fits.  Communication is limited to
  (1) one broadcast of the shared problem description from rank 0 (matrices, grids, scalars: a few MB) and one SCATTER of
      the spectra (each rank receives the rows of Z it samples), and
  (2) one gather at the end -- per-spectrum posterior SUMMARIES (mean + percentiles, reduced on each GPU by
      bdrt_sampler_summary) or, on request, the raw draws, taken straight from HBM (no host round trip) --
over RCCL / xGMI when the process group backend is "nccl", gloo on CPU tensors in the tests.
Partition (`partition_units`): whole spectra per rank when there are at least as many spectra as ranks (BASELINE
config 4), otherwise the chains of the few spectra are spread over the ranks (configs 3 and 5: one spectrum, 4 chains
=> 4 GPUs busy).  Draws are a function of (seed, chain id) only, so results do not depend on the partition.
"""
import numpy as np

_INT_LIMIT = 2 ** 53        # integers travel inside a float64 buffer: exact below this


def shard_bounds(n_items, world, rank):
    """Contiguous block partition: ranks [0, n_items % world) get one extra item."""
    base, extra = divmod(n_items, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def make_units(n_spectra, chains):
    """unit u -> (spectrum, chain id): spectrum-major so that a block partition keeps whole spectra on one GPU."""
    spec = np.repeat(np.arange(n_spectra, dtype=np.int32), chains)
    chain = np.tile(np.arange(chains, dtype=np.int32), n_spectra)
    return spec, chain


def partition_units(n_spectra, chains, world):
    """[(unit_lo, unit_hi)] per rank over the spectrum-major unit list.
    n_spectra >= world: block partition by SPECTRUM (a rank keeps whole spectra, so its summaries are complete);
    fewer spectra than ranks: block partition of the UNITS themselves (chains of one spectrum on several GPUs)."""
    if n_spectra >= world:
        return [tuple(chains * b for b in shard_bounds(n_spectra, world, r)) for r in range(world)]
    return [shard_bounds(n_spectra * chains, world, r) for r in range(world)]


def _dist():
    import torch.distributed as dist
    return dist


def _device_for_group(group=None):
    import torch
    dist = _dist()
    backend = dist.get_backend(group)
    return torch.device('cuda', torch.cuda.current_device()) if backend == 'nccl' else torch.device('cpu')


def broadcast_arrays(arrays, src=0, group=None):
    """Broadcast a dict of real numpy arrays / scalars from `src` to every rank (one metadata object + one flat fp64
    buffer, i.e. a single large collective instead of one per array)."""
    import torch
    dist = _dist()
    rank = dist.get_rank(group)
    meta = [None]
    if rank == src:
        meta[0] = []
        for k, v in arrays.items():
            a = np.asarray(v)
            if a.dtype.kind not in 'fiub':
                raise TypeError('broadcast_arrays: %s has dtype %s; only real floating / integer / bool arrays travel' % (k, a.dtype))
            if a.dtype.kind in 'iu' and a.size and np.max(np.abs(a.astype(np.float64))) >= _INT_LIMIT:
                raise ValueError('broadcast_arrays: integer values of %s exceed 2^53' % k)
            meta[0].append((k, a.shape, str(a.dtype)))
    dist.broadcast_object_list(meta, src=src, group=group)
    dev = _device_for_group(group)
    total = int(sum(int(np.prod(shape)) if len(shape) else 1 for _, shape, _ in meta[0]))
    if rank == src:
        flat = np.concatenate([np.asarray(arrays[k], dtype=np.float64).ravel() for k, _, _ in meta[0]]) if total else np.zeros(0)
        buf = torch.from_numpy(flat).to(dev)
    else:
        buf = torch.empty(total, dtype=torch.float64, device=dev)
    if total:
        dist.broadcast(buf, src=src, group=group)
    flat = buf.cpu().numpy()
    out, o = {}, 0
    for k, shape, dtype in meta[0]:
        n = int(np.prod(shape)) if len(shape) else 1
        a = flat[o:o + n].reshape(shape)
        out[k] = a.astype(dtype) if dtype != 'float64' else a.copy()
        o += n
    return out


def gather_rows(local, counts, group=None):
    """All-gather row blocks of unequal length (counts[r] rows on rank r): returns the concatenation (numpy) on every
    rank.  `local`: numpy array, torch tensor, or an object with `__cuda_array_interface__` (device memory of the sampler):
    for an "nccl" group a device-resident block is gathered where it is."""
    import torch
    dist = _dist()
    world = dist.get_world_size(group)
    dev = _device_for_group(group)
    if hasattr(local, '__cuda_array_interface__') and dev.type == 'cuda':
        t_local = torch.as_tensor(local, device=dev)
    elif hasattr(local, '__cuda_array_interface__'):
        raise TypeError('gather_rows: a device buffer needs an nccl process group')
    elif isinstance(local, torch.Tensor):
        t_local = local.to(dev, dtype=torch.float64)
    else:
        t_local = torch.from_numpy(np.ascontiguousarray(local, dtype=np.float64)).to(dev)
    tail = tuple(t_local.shape[1:])
    width = int(np.prod(tail)) if len(tail) else 1
    maxc = int(max(counts)) if len(counts) else 0
    if maxc == 0:
        return np.zeros((0,) + tail)
    pad = torch.zeros((maxc, width), dtype=torch.float64, device=dev)
    if t_local.shape[0]:
        pad[:t_local.shape[0]] = t_local.reshape(t_local.shape[0], width)
    outs = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(outs, pad, group=group)
    full = torch.cat([outs[r][:counts[r]] for r in range(world)], dim=0)
    return full.cpu().numpy().reshape((int(sum(counts)),) + tail)


def scatter_rows(full, counts, width, src=0, group=None):
    """Scatter row blocks of unequal length from `src`: rank r receives rows [sum(counts[:r]), sum(counts[:r + 1])) of
    `full` ([sum(counts), width], needed on `src` only) as a numpy array [counts[r], width].  One collective; the blocks are
    padded to the longest one (a scatter moves equal pieces)."""
    import torch
    dist = _dist()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    dev = _device_for_group(group)
    maxc = int(max(counts)) if len(counts) else 0
    if maxc == 0 or width == 0:
        return np.zeros((0, width))
    out = torch.empty((maxc, width), dtype=torch.float64, device=dev)
    pieces = None
    if rank == src:
        a = np.ascontiguousarray(np.asarray(full, dtype=np.float64).reshape(int(sum(counts)), width))
        pieces, o = [], 0
        for r in range(world):
            blk = np.zeros((maxc, width))
            blk[:counts[r]] = a[o:o + counts[r]]
            o += counts[r]
            pieces.append(torch.from_numpy(blk).to(dev))
    dist.scatter(out, pieces, src=src, group=group)
    return out[:counts[rank]].cpu().numpy()


class GpuWorker:
    """Per-rank worker: the problem in this rank's HBM + the device-resident NUTS chains of this rank's units."""

    def __init__(self, problem_kwargs):
        from .model import Problem
        kw = dict(problem_kwargs)
        blocks = kw.pop('blocks'); Z = kw.pop('Z'); freq = kw.pop('freq')
        self.problem = Problem(blocks, Z, freq, **kw)
        self.D = self.problem.D
        self.sampler = None

    def run(self, spec, chain_ids, warmup, n_draws, seed, control, init_theta=None):
        import ctypes as C
        from . import _lib
        from .engine import Sampler
        ctrl = _lib.NutsControl()
        self.problem._lib.bdrt_nuts_defaults(C.byref(ctrl))
        for k, v in (control or {}).items():
            setattr(ctrl, k, v)
        self.sampler = Sampler(self.problem, len(spec), warmup, n_draws, seed, ctrl, spec=spec, chain_ids=chain_ids,
                               init_theta=init_theta)
        self.sampler.run()
        _, self._lp, diag = self.sampler.results(want_draws=False)
        self._stats = np.array([[d['n_leapfrog'], d['n_divergent'], d['n_max_treedepth'], d['stepsize'], d['mean_accept']]
                                for d in diag]).reshape(len(spec), 5)

    def lp(self):
        return self._lp

    def stats(self):
        return self._stats

    def draws(self, device):
        """[n_units, n_draws, D]: the device buffer itself for a cuda group, a host copy otherwise."""
        if device.type == 'cuda':
            return self.sampler.draws_device()
        return self.sampler.results()[0]

    def summary(self, unit_lo, unit_hi, q):
        return self.sampler.summary(unit_lo, unit_hi, q)

    def is_pos(self):
        return self.problem.is_pos

    def diagnostics(self, unit_lo, unit_hi, chains):
        """(mean, sd, n_eff, Rhat) [spectra x D] of this rank's units [unit_lo, unit_hi), reduced on the sampler's device draws."""
        return self.sampler.diagnostics(unit_lo, unit_hi, chains)

    def rank_diagnostics(self, unit_lo, unit_hi, chains):
        """Rank-normalised diagnostics (dict, each [spectra x D]) of this rank's units, reduced on the sampler's device draws."""
        return self.sampler.rank_diagnostics(unit_lo, unit_hi, chains)

    def loo(self, unit_lo, unit_hi, chains, **kw):
        """PSIS-LOO per observation (`Sampler.loo`: dict, each [spectra x units]) of this rank's units, reduced on the device."""
        return self.sampler.loo(unit_lo, unit_hi, chains, **kw)

    def loo_predict(self, unit_lo, unit_hi, chains, **kw):
        """The LOO predictive moments (`Sampler.loo_predict`) of this rank's units, reduced on the device."""
        return self.sampler.loo_predict(unit_lo, unit_hi, chains, **kw)

    @staticmethod
    def reduce_rank_diagnostics(blocks, chains, is_pos):
        """The same reduction on host-resident unconstrained draws [spectra, chains * draws, D] (bdrt_rank_diagnostics)."""
        from .diagnostics import rank_diagnostics
        return rank_diagnostics(blocks, chains, is_pos=is_pos)

    @staticmethod
    def reduce_loo(problem_kwargs, blocks, chains, predict, **kw):
        """`loo` / `loo_predict` on host-resident unconstrained draws [spectra, chains * draws, D]: the host path
        (`loo.host_psis_loo` / `loo.host_psis_predict`) against the spectra of `problem_kwargs`."""
        from . import loo as _loo
        from .model import Problem
        pk = dict(problem_kwargs)
        bl = pk.pop('blocks'); Z = np.atleast_2d(pk.pop('Z')); freq = pk.pop('freq')
        prob = Problem(bl, Z, freq, **pk)
        try:
            return (_loo.host_psis_predict if predict else _loo.host_psis_loo)(prob, blocks, Z, chains, **kw)
        finally:
            prob.close()

    @staticmethod
    def reduce_diagnostics(blocks, chains, is_pos):
        """The same reduction on host-resident unconstrained draws [spectra, chains * draws, D] (bdrt_diagnostics)."""
        from .diagnostics import column_diagnostics
        return column_diagnostics(blocks, chains, is_pos=is_pos)

    @staticmethod
    def reduce(block, is_pos, q):
        """(mean [D], pct [len(q), D]) of the constrained parameters over the rows of `block` (unconstrained draws): the
        arithmetic of `summary`, on host-resident draws (bdrt_summary)."""
        from . import post
        return post.summary(block, q, is_pos)

    def close(self):
        if self.sampler is not None:
            self.sampler.close()
        self.problem.close()


def _pack_problem(problem_kwargs):
    flat = {}
    kw = dict(problem_kwargs)
    blocks = kw.pop('blocks')
    flat['n_blocks'] = np.array(len(blocks))
    for b, blk in enumerate(blocks):
        for k in ('A', 'L0', 'L1', 'L2'):
            a = np.asarray(blk[k])
            if a.dtype.kind not in 'fiu':
                raise TypeError('problem matrix %s of block %d must be real (got %s)' % (k, b, a.dtype))
            flat['b%d_%s' % (b, k)] = a.astype(np.float64)
        flat['b%d_flags' % b] = np.array([float(bool(blk.get('parallel', False))), float(bool(blk.get('nonneg', False))),
                                         float(blk.get('x_scale', 1.0))])
    for k, v in kw.items():
        if v is not None:
            a = np.asarray(v)
            if a.dtype.kind not in 'fiub':
                raise TypeError('problem entry %s must be real (got %s)' % (k, a.dtype))
            flat['kw_' + k] = a.astype(np.float64)
    return flat


def _unpack_problem(flat):
    nb = int(flat['n_blocks'])
    blocks = []
    for b in range(nb):
        fl = flat['b%d_flags' % b]
        blocks.append(dict(A=flat['b%d_A' % b], L0=flat['b%d_L0' % b], L1=flat['b%d_L1' % b], L2=flat['b%d_L2' % b],
                           parallel=bool(fl[0]), nonneg=bool(fl[1]), x_scale=float(fl[2])))
    kw = {'blocks': blocks}
    for k, v in flat.items():
        if k.startswith('kw_'):
            name = k[3:]
            kw[name] = v if v.ndim else (int(v) if name in ('outlier_mode',) else (bool(v) if name == 'use_x_sum' else float(v)))
    return kw


_RANK_FIELDS = ('rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'sd')
_LOO_FIELDS = ('lpd', 'elpd_loo', 'pareto_k', 'p_waic', 'n_tail', 'reff')


def _loo_jobs(loo_kw):
    """[(result key, predict)] of the reductions the request (`loo.loo_request`'s dict, or None) asks for."""
    if loo_kw is None:
        return []
    return [(k, p) for k, p, on in (('loo', False, loo_kw['loo']), ('loo_predict', True, loo_kw['predict'])) if on]


def _loo_call_kw(loo_kw, s_lo, s_hi):
    """Keyword arguments of `Sampler.loo` for spectra [s_lo, s_hi): an array reff [n_spectra, units] is cut to their rows."""
    kw = {k: loo_kw[k] for k in ('unit', 'part', 'reff', 'chunk_bytes')}
    r = kw['reff']
    if r is not None and not isinstance(r, str) and np.ndim(r) == 2:
        kw['reff'] = np.asarray(r, dtype=float)[s_lo:s_hi]
    return kw


def _gather_fields(r, rows, group, predict):
    """All-gather the per-spectrum rows of a `Sampler.loo` / `Sampler.loo_predict` dict, every field side by side in one
    collective (n_tail travels as a float: exact).  rows[r]: spectra of rank r, at least one each."""
    from .loo import PREDICT_FIELDS
    names = (PREDICT_FIELDS + ('pareto_k', 'n_tail', 'reff')) if predict else _LOO_FIELDS
    w = [r[k].shape[1] for k in names]
    full = gather_rows(np.concatenate([np.asarray(r[k], dtype=np.float64) for k in names], axis=1), rows, group)
    out, o = {}, 0
    for k, wk in zip(names, w):
        out[k] = full[:, o:o + wk].astype(np.int32) if k == 'n_tail' else np.ascontiguousarray(full[:, o:o + wk])
        o += wk
    if not predict:
        out['p_loo'], out['elpd_waic'] = out['lpd'] - out['elpd_loo'], out['lpd'] - out['p_waic']
    return out


def sample_sharded(problem_kwargs, n_spectra, chains, warmup, n_draws, seed=1234, control=None, group=None,
                   worker_cls=None, gather='draws', q=(2.5, 50.0, 97.5), init_theta=None, diagnostics=False, loo=None,
                   rank_diagnostics=False):
    """Sample `chains` chains for each of `n_spectra` spectra on all ranks of the process group.

    problem_kwargs (needed on rank 0 only; other ranks may pass None): dict(blocks=[...], Z=[n_spectra x 2nf], freq=...,
    **scalars) as for model.Problem.  Returns, identically on every rank and for any world size, a dict with
      stats [n_units, 5]   per chain: leapfrogs, divergent, max-treedepth hits, step size, mean accept (unit order)
      lp    [n_units, n_draws]
      mean  [n_spectra, D], pct [n_spectra, len(q), D]   posterior summary of the CONSTRAINED parameters per spectrum
      draws [n_units, n_draws, D] (unconstrained)        only with gather='draws'
    gather='summary' moves n_spectra*(1+len(q))*D numbers instead of the draws; when the chains of a
    spectrum are spread over ranks (fewer spectra than ranks) the summary needs all of them, so the draws are gathered
    in that case regardless.
    init_theta (rank 0; optional): [n_units, D] unconstrained start points in unit order (Stan `init=` values; default: the
    sampler's own random starts); each rank receives the rows of its units with the scatter of the spectra.
    diagnostics=True adds n_eff [n_spectra, D] and Rhat [n_spectra, D]: the convergence diagnostics of the constrained
    parameters per spectrum (bayes_drt_amd.diagnostics), each rank reducing its own spectra in one launch on its sampler's
    device draws; when the chains of a spectrum are spread over ranks, every rank reduces the gathered draws instead.
    rank_diagnostics=True adds 'rank', the dict of `diagnostics.rank_diagnostics` (each entry [n_spectra, D]), the same way.
    loo=dict(loo=True, predict=False, unit='frequency', part='both', reff='auto', chunk_bytes=None) (given on every rank, like
    `gather` and `q`) adds 'loo', the dict of `loo.psis_loo` plus 'reff', each entry [n_spectra, units], and / or 'loo_predict',
    the dict of `loo.psis_predict` plus 'reff': each rank reduces its own spectra on its sampler's device draws
    (`Sampler.loo`, `Sampler.loo_predict`) and only these rows travel, so gather='summary' has them without any draw leaving a
    GPU; when the chains of a spectrum are spread over ranks, every rank reduces the gathered draws through the host path
    (`loo.host_psis_loo`).  With reff None, a number or an array [n_spectra, units] the two ways agree bit for bit, so the result
    does not depend on the world size; reff='auto' is the device's relative efficiency in the first case and
    `loo.relative_efficiency` in the second, which may differ in the last bits of 'reff' ('reff' says what was used)."""
    if gather not in ('draws', 'summary'):
        raise ValueError("gather must be 'draws' or 'summary'")
    dist = _dist()
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    spec, chain = make_units(n_spectra, chains)
    parts = partition_units(n_spectra, chains, world)
    u0, u1 = parts[rank]
    whole = n_spectra >= world                                     # every spectrum lives on exactly one rank
    counts = [hi - lo for lo, hi in parts]
    # (1) the shared problem (matrices, grids, scalars) is BROADCAST; (2) the spectra are SCATTERED by rank -- each rank
    # receives the rows of Z it samples -- unless the chains of a spectrum are spread over ranks (fewer spectra
    # than ranks: every rank then needs the few spectra, and they travel with the broadcast)
    Zfull = None
    status = [None]
    if rank == 0:
        # (arguments are checked HERE and the verdict travels first: an exception on rank 0 alone would leave the other ranks
        # waiting in the broadcast below until the process-group timeout)
        try:
            flat0 = _pack_problem(problem_kwargs)
            Zfull = np.atleast_2d(flat0['kw_Z'])
            if Zfull.shape[0] != n_spectra:
                raise ValueError('sample_sharded: Z has %d spectra, n_spectra = %d' % (Zfull.shape[0], n_spectra))
            if init_theta is not None:
                init_theta = np.ascontiguousarray(np.asarray(init_theta, dtype=np.float64))
                if init_theta.ndim != 2 or init_theta.shape[0] != n_spectra * chains:
                    raise ValueError('sample_sharded: init_theta must be [n_spectra * chains, D]')
                # the width is checked HERE too: a wrong one would only surface inside `worker.run` on the ranks that own
                # units, while ranks without units wait in the gathers (layout of include/bdrt.h: 2 offsets, x per block,
                # 4 error parameters, 2 Nf outlier parameters, ups per block, 3 penalty strengths per block)
                n_blk = int(flat0['n_blocks'])
                D0 = 6 + sum(2 * flat0['b%d_A' % b].shape[1] + 3 for b in range(n_blk))
                if int(np.asarray(flat0.get('kw_outlier_mode', 0))):
                    D0 += Zfull.shape[1]
                if init_theta.shape[1] != D0:
                    raise ValueError('sample_sharded: init_theta has %d columns, the model has D = %d parameters'
                                     % (init_theta.shape[1], D0))
            if loo is not None:
                from . import loo as _loo
                req = _loo.loo_request(loo, 'sample_sharded', need_chains=False)
                pair, mode = _loo.check_device_args(req['unit'], req['part'], req['reff'], 'sample_sharded')
                if mode == 1:
                    ncols = _loo.part_columns(req['part'], Zfull.shape[1] // 2)[1]
                    np.broadcast_to(np.asarray(req['reff'], dtype=float), (n_spectra, ncols // 2 if pair else ncols))
                if chains * n_draws > _loo.max_draws() or chains * n_draws < 2:
                    raise ValueError('sample_sharded: loo needs 2 ... %d draws per spectrum, not %d' % (_loo.max_draws(), chains * n_draws))
            if whole:
                flat0.pop('kw_Z')
                flat0['Z_width'] = np.array(Zfull.shape[1])
            flat0['init_width'] = np.array(0 if init_theta is None else init_theta.shape[1])
        except Exception as e:          # noqa: BLE001 -- re-raised on every rank
            status[0] = '%s: %s' % (type(e).__name__, e)
    dist.broadcast_object_list(status, src=0, group=group)
    if status[0] is not None:
        raise ValueError('sample_sharded (rank 0): ' + status[0])
    from .loo import loo_request                                   # (rank 0 has passed the request: every rank normalises it)
    loo_kw = None if loo is None else loo_request(loo, 'sample_sharded', need_chains=False)
    flat = broadcast_arrays(flat0 if rank == 0 else None, src=0, group=group)
    init_width = int(flat.pop('init_width'))
    init_local = scatter_rows(init_theta, counts, init_width, src=0, group=group) if init_width else None
    if whole:
        width = int(flat.pop('Z_width'))
        rows = [c // chains for c in counts]                        # whole spectra per rank
        flat['kw_Z'] = scatter_rows(Zfull, rows, width, src=0, group=group)
    kw = _unpack_problem(flat)
    dev = _device_for_group(group)
    q = [float(v) for v in np.atleast_1d(q)]
    cls = worker_cls or GpuWorker
    worker = None
    D = None
    if u1 > u0:
        s0, s1 = int(spec[u0]), int(spec[u1 - 1]) + 1
        local_kw = dict(kw)
        # only this rank's spectra go to HBM: what the scatter delivered, or this rank's rows of the broadcast copy
        local_kw['Z'] = np.atleast_2d(kw['Z']) if whole else np.atleast_2d(kw['Z'])[s0:s1]
        worker = cls(local_kw)
        if init_local is not None:
            worker.run(spec[u0:u1] - s0, chain[u0:u1], warmup, n_draws, seed, control, init_theta=init_local)
        else:
            worker.run(spec[u0:u1] - s0, chain[u0:u1], warmup, n_draws, seed, control)
        D = int(worker.D)
    # ranks without work learn D (and which parameters are <lower=0>) from the first rank that has some
    owners = [r for r in range(world) if counts[r] > 0]
    if not owners:
        empty = dict(stats=np.zeros((0, 5)), lp=np.zeros((0, n_draws)), mean=np.zeros((0, 0)), pct=np.zeros((0, len(q), 0)),
                     draws=np.zeros((0, n_draws, 0)))
        if diagnostics:
            empty.update(n_eff=np.zeros((0, 0)), Rhat=np.zeros((0, 0)))
        if rank_diagnostics:
            empty['rank'] = {}
        empty.update({k: {} for k, _ in _loo_jobs(loo_kw)})
        return empty
    dd = [(D, np.asarray(worker.is_pos(), dtype=bool).tolist()) if worker is not None else None]
    dist.broadcast_object_list(dd, src=owners[0], group=group)
    D, is_pos = int(dd[0][0]), np.asarray(dd[0][1], dtype=bool)
    out = {}
    out['stats'] = gather_rows(worker.stats() if worker else np.zeros((0, 5)), counts, group)
    out['lp'] = gather_rows(worker.lp() if worker else np.zeros((0, n_draws)), counts, group)
    need_draws = gather == 'draws' or not whole
    if need_draws:
        local = worker.draws(dev) if worker else np.zeros((0, n_draws, D))
        out['draws'] = gather_rows(local, counts, group)
    if whole:
        # per-spectrum summaries reduced where the draws are; gather [1 + nq, D] per spectrum
        ns_local = (u1 - u0) // chains
        loc = np.zeros((ns_local, 1 + len(q), D))
        for i in range(ns_local):
            m, p = worker.summary(i * chains, (i + 1) * chains, q)
            loc[i, 0], loc[i, 1:] = m, p
        summ = gather_rows(loc, [c // chains for c in counts], group)
        out['mean'], out['pct'] = summ[:, 0], summ[:, 1:]
        if diagnostics:
            dl = np.zeros((ns_local, 2, D))
            if ns_local:
                _, _, ne, rh = worker.diagnostics(0, u1 - u0, chains)
                dl[:, 0], dl[:, 1] = ne, rh
            dg = gather_rows(dl, [c // chains for c in counts], group)
            out['n_eff'], out['Rhat'] = dg[:, 0], dg[:, 1]
        if rank_diagnostics:
            from .diagnostics import _rank_dict
            rl = np.zeros((ns_local, 5, D))
            r = worker.rank_diagnostics(0, u1 - u0, chains)
            for k, name in enumerate(_RANK_FIELDS):
                rl[:, k] = r[name]
            rg = gather_rows(rl, [c // chains for c in counts], group)
            out['rank'] = _rank_dict(*[rg[:, k] for k in range(5)])
        for key, predict in _loo_jobs(loo_kw):
            lk = _loo_call_kw(loo_kw, u0 // chains, u1 // chains)
            r = (worker.loo_predict if predict else worker.loo)(0, u1 - u0, chains, **lk)
            out[key] = _gather_fields(r, [c // chains for c in counts], group, predict)
    else:
        # the chains of a spectrum are on several ranks: reduce the gathered draws (every rank, same arithmetic)
        mean = np.empty((n_spectra, D)); pct = np.empty((n_spectra, len(q), D))
        for sidx in range(n_spectra):
            block = out['draws'][sidx * chains:(sidx + 1) * chains].reshape(chains * n_draws, D)
            mean[sidx], pct[sidx] = cls.reduce(block, is_pos, q)
        out['mean'], out['pct'] = mean, pct
        if diagnostics:
            blocks = out['draws'].reshape(n_spectra, chains * n_draws, D)
            _, _, out['n_eff'], out['Rhat'] = cls.reduce_diagnostics(blocks, chains, is_pos)
        if rank_diagnostics:
            out['rank'] = cls.reduce_rank_diagnostics(out['draws'].reshape(n_spectra, chains * n_draws, D), chains, is_pos)
        for key, predict in _loo_jobs(loo_kw):
            lk = _loo_call_kw(loo_kw, 0, n_spectra)
            lk.pop('chunk_bytes')
            out[key] = cls.reduce_loo(kw, out['draws'].reshape(n_spectra, chains * n_draws, D), chains, predict, **lk)
        if gather == 'summary':
            out.pop('draws')
    if worker is not None:
        worker.close()
    return out
