"""Measure the power-scaling sensitivity check on the GPU.

    python tools/powerscale_timing.py [runs] [numpy_fits]     # -> profiles/powerscale/timing.txt

The benchmark's synthetic spectra at 81 frequencies x 161 basis functions, nonneg=True, 4 chains x 1000 draws after 200 warm-up,
driven through the engine as bench.py drives it (`Inverter.batch_stan_data`, one `Sampler`): one spectrum, then a batch of 60.
Host clock around whole calls, one untimed call of each first, then `runs` (default five) of each:
  * the sampler's own run (`Sampler.run` and the copy of the draws to the host), once per batch size: what the check is set against;
  * `Sampler.powerscale` on the draws where the sampler left them;
  * the same statistic by the numpy statement (tests/powerscale_numpy.py) on the draws copied to the host, through the host entry
    points the GPU tests use (`Problem.logp_grad(jacobian=False)`, `Problem.transformed`, `psis_numpy.pointwise_log_lik`): timed on
    the first `numpy_fits` (default two) spectra of the batch and scaled to the batch, which the record says.
Recorded, not asserted."""
import ctypes as C
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'powerscale')


def _stat(ts, unit='s'):
    return 'median %.3f %s (%.3f ... %.3f) of %d' % (float(np.median(ts)), unit, min(ts), max(ts), len(ts))


def main(runs, numpy_fits):
    import bench
    from bayes_drt_amd import _lib
    from bayes_drt_amd import parallel as par
    from bayes_drt_amd import powerscale as PS
    from bayes_drt_amd.engine import Sampler
    from bayes_drt_amd.inversion import Inverter
    from bayes_drt_amd.stan_models import load_pickle
    from tests import powerscale_numpy as pw
    from tests import psis_numpy as pn
    chains, samples, warmup = 4, 1000, 200
    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    for n in (1, 60):
        f, zs = bench.synth_spectra(n, raw=True)
        basis = np.logspace(10, -6, bench.K)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            name, dat = Inverter(basis_freq=basis).batch_stan_data(np.asarray(f, dtype=float), [np.asarray(Z) for Z in zs], nonneg=True)
        model = load_pickle(name)
        prob = model._prepare(dat)
        ctrl = _lib.NutsControl()
        prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
        ctrl.adapt_delta, ctrl.adapt_t0 = 0.9, 10
        spec, chain = par.make_units(n, chains)
        t0 = time.perf_counter()
        smp = Sampler(prob, n * chains, warmup, samples, 5, ctrl, spec=spec, chain_ids=chain)
        smp.run()
        draws = smp.results()[0].reshape(n, chains * samples, prob.D)
        t_run = time.perf_counter() - t0
        say('%d spectr%s x %d chains x %d draws, %d frequencies x %d basis functions, D = %d: sampling and the copy of the draws %.2f s (one run)'
            % (n, 'um' if n == 1 else 'a', chains, samples, prob.nf, bench.K, prob.D, t_run))
        smp.powerscale(0, smp.n_units, chains)                               # untimed: module load, kernel attributes, allocator
        td = []
        for _ in range(runs):
            t0 = time.perf_counter()
            dev = smp.powerscale(0, smp.n_units, chains)
            td.append(time.perf_counter() - t0)
        say('  Sampler.powerscale                                  ' + _stat(td))
        sens = PS.sensitivity(dev['cjs2'].reshape(n, prob.D, 2, 2), 1.01)
        say('  sensitivities over the batch: prior median %.3g (%.3g ... %.3g), likelihood median %.3g (%.3g ... %.3g); parameters at or '
            'above 0.05: prior %d, likelihood %d of %d; Pareto k %.2f ... %.2f'
            % (np.median(sens[..., 0]), sens[..., 0].min(), sens[..., 0].max(), np.median(sens[..., 1]), sens[..., 1].min(),
               sens[..., 1].max(), int(np.sum(sens[..., 0] >= 0.05)), int(np.sum(sens[..., 1] >= 0.05)), n * prob.D,
               dev['pareto_k'].min(), dev['pareto_k'].max()))
        Z = np.atleast_2d(np.asarray(dat['Z'], dtype=float))
        m = min(n, numpy_fits)
        th, worst = [], 0.0
        for g in range(m):
            t0 = time.perf_counter()
            theta = draws[g]
            lp0 = prob.logp_grad(theta, jacobian=False, spec=np.full(len(theta), g), want_grad=False)[0]
            par_, Zh, sg = prob.transformed(theta)
            ref = pw.powerscale(lp0, pn.pointwise_log_lik(Zh, sg, Z[g]), par_)
            th.append(time.perf_counter() - t0)
            worst = max(worst, float(np.abs(dev['cjs2'][g].reshape(-1, 2, 2) - ref['cjs2']).max()))
        say('  numpy statement on the host draws, per spectrum     ' + _stat(th) + '; largest |cjs2 device - numpy| %.3g' % worst)
        say('  -> the batch: device %.3f s, numpy %.1f s (%d x the per-spectrum median); the check adds %.2f %% to the sampling time'
            % (np.median(td), n * np.median(th), n, 100.0 * np.median(td) / t_run))
        smp.close()
        prob.close()
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, 'timing.txt'), 'w') as fh:
        fh.write('Power-scaling sensitivity: end-to-end time (MI355X, gfx950; tools/powerscale_timing.py %d %d)\n\n'
                 'single process; host clock around whole calls (each ends in copies back to the host); one untimed call first; the\n'
                 'benchmark\'s synthetic spectra (bench.synth_spectra), nonneg=True, warm-up 200:\n\n' % (runs, numpy_fits))
        fh.write('\n'.join('  ' + ln for ln in lines) + '\n')
    print('wrote', os.path.join(OUT, 'timing.txt'))


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 5, int(sys.argv[2]) if len(sys.argv) > 2 else 2)
