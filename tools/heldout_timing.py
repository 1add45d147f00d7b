"""Measure K-fold cross-validation and exact refits on the GPU.

    python tools/heldout_timing.py time [runs]     # -> profiles/heldout/timing.txt
    python tools/heldout_timing.py agreement [seed ... | merge]   # -> profiles/heldout/agreement.txt (default seeds 5 6)

`time`: 64 spectra x 4 chains x 1000 draws at 81 x 161 with folds=10, host clock around whole calls, one untimed fold of each
path first, then `runs` (default five) of each, alternating; every fold of the spelt-out paths prints its own time:
  * `kfold_many` (the held-out reduction on the sampler's device draws);
  * the same folds with the reduction done by the host path on the downloaded draws (`loo.host_heldout`);
  * `fit_many` alone on the ten training grids.
`agreement`: one synthetic spectrum of the benchmark; PSIS elpd_i against the exact-refit elpd_i of EVERY frequency
(`reloo(k_threshold=-inf, max_refits=None)`) for two seeds, and the seed-to-seed differences beside them.  A seed is 82 fits
one after the other, so seeds can be run in calls of their own: each leaves profiles/heldout/agreement_seed<N>.txt, and the
record is written from the seeds that are there.  Recorded, not asserted: the Monte Carlo error of either side is unmeasured."""
import logging
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'heldout')


def spectra(n):
    """The benchmark's own synthetic spectra (bench.py): 81 frequencies, fitted on its 161-point basis with nonneg=True."""
    import bench
    f, zs = bench.synth_spectra(n, raw=True)
    return np.asarray(f, dtype=float), [np.asarray(Z) for Z in zs], np.logspace(10, -6, bench.K)


def _stat(ts):
    return 'median %.2f s (%.2f ... %.2f) of %d' % (float(np.median(ts)), min(ts), max(ts), len(ts))


def time_main(runs):
    from bayes_drt_amd import loo
    from bayes_drt_amd.inversion import Inverter
    n, chains, samples, warmup, folds = 64, 4, 1000, 200, 10
    f, zs, basis = spectra(n)
    kw = dict(nonneg=True, warmup=warmup, samples=samples, chains=chains, random_seed=5, check_outliers=False, check_diagnostics=False)
    labels = loo.fold_labels(f, folds)

    def device():
        t0 = time.perf_counter()
        views = Inverter(basis_freq=basis).kfold_many(f, zs, folds=folds, **kw)
        return time.perf_counter() - t0, [v.kfold_result for v in views]

    def host(reduce=True, only=None):
        """the folds of `kfold_many` spelt out: fit_many on the training rows, then the host path on the views' draws"""
        t0 = time.perf_counter()
        base = Inverter(basis_freq=basis)._pinned_copy(f)
        per = [dict() for _ in zs]
        for lab in (range(folds) if only is None else only):
            t1 = time.perf_counter()
            test = labels == lab
            views = base.fit_many(f[~test], [Z[~test] for Z in zs], mode='sample', **kw)
            t2 = time.perf_counter()
            if reduce:
                jobs = [dict(outliers=False, model_type=views[0].stan_model_name.split('_')[0])] * n
                held = Inverter._heldout_job(views, jobs, dict(pairs=[(f[test], Z[test]) for Z in zs], unit='frequency', sigma_out=None), 'both', chains)
                prob = views[0]._sample_result._model.problem
                res = loo.host_heldout(prob, np.stack([v._sample_result.theta for v in views]), chains, held['freq_test'],
                                       held['A_test_blocks'], held['z_test'])
                for i, v in enumerate(views):
                    v._store_heldout(res, i, held, chains * samples)
                    per[i][lab] = v.heldout_result
            print('  fold %d: fit_many %.2f s%s (evaluator %d)' % (lab, t2 - t1, ', host_heldout %.2f s' % (time.perf_counter() - t2) if reduce else '',
                                                                views[0]._sample_result._model.problem.evaluator()), flush=True)
        dt = time.perf_counter() - t0
        return dt, [loo.kfold_result(labels, p) for p in per] if reduce and only is None else None

    lines = []

    def say(text):
        lines.append(text)
        print(text, flush=True)

    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        # untimed: ONE fold of each path (module load, kernel attributes, allocator)
        test = labels == 0
        Inverter(basis_freq=basis)._pinned_copy(f).fit_many(f[~test], [Z[~test] for Z in zs], heldout=[(f[test], Z[test]) for Z in zs],
                                                            mode='sample', **kw)
        host(True, only=[0])
        say('%d spectra x %d chains x %d draws, %d frequencies x %d basis functions, folds = %d (held-out frequencies per fold: %s)'
            % (n, chains, samples, len(f), len(basis), folds, sorted(set(np.bincount(labels).tolist()))))
        td, th, tf = [], [], []
        for r in range(runs):
            t, rd = device()
            td.append(t)
            say('run %d: kfold_many %.2f s' % (r, t))
            t, rh = host()
            th.append(t)
            same = all(np.array_equal(a.elpd_i, b.elpd_i) and np.array_equal(a.Z_pred, b.Z_pred) and np.array_equal(a.pit_re, b.pit_re)
                       for a, b in zip(rd, rh))
            say('run %d: the same folds with host_heldout on the downloaded draws %.2f s; device and host results agree bit for bit: %s'
                % (r, t, same))
            tf.append(host(False)[0])
            say('run %d: fit_many alone x %d %.2f s' % (r, folds, tf[-1]))
    say('kfold_many (reduction on the device draws)        ' + _stat(td))
    say('the same folds, host_heldout on downloaded draws  ' + _stat(th))
    say('fit_many alone x %d                               ' % folds + _stat(tf))
    say('held-out share: device path %.2f s, host path %.2f s (medians minus the median of fit_many alone)'
        % (np.median(td) - np.median(tf), np.median(th) - np.median(tf)))
    say('elpd_kfold of the first three spectra: ' + ', '.join('%.2f (se %.2f)' % (r.elpd_loo, r.se) for r in rd[:3]))
    _write('timing.txt', 'K-fold cross-validation of many spectra: end-to-end time (MI355X, gfx950; tools/heldout_timing.py time %d)\n\n'
           'single process; host clock around whole calls (each ends in copies back to the host); one untimed FOLD of each path first, then\n'
           '%d run(s) of each, one after the other; the benchmark\'s synthetic spectra (bench.synth_spectra), nonneg=True, warm-up 200:\n\n' % (runs, runs),
           lines)


def agreement_main(seeds):
    from bayes_drt_amd.inversion import Inverter
    f, zs, basis = spectra(1)
    Z = zs[0]
    kw = dict(nonneg=True, warmup=200, samples=250, chains=4, check_outliers=False, check_diagnostics=False)
    os.makedirs(OUT, exist_ok=True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for seed in seeds:
            inv = Inverter(basis_freq=basis)
            t0 = time.perf_counter()
            inv.fit(f, Z, mode='sample', loo=True, random_seed=seed, **kw)
            psis = inv.loo_result
            t1 = time.perf_counter()
            exact = inv.reloo(f, Z, k_threshold=-np.inf, max_refits=None, random_seed=seed, **kw)
            t2 = time.perf_counter()
            print('seed %d: fit + PSIS-LOO %.1f s, %d exact refits %.1f s' % (seed, t1 - t0, int(exact.refit.sum()), t2 - t1), flush=True)
            np.savetxt(os.path.join(OUT, 'agreement_seed%d.txt' % seed),
                       np.column_stack([np.sort(f)[::-1], psis.pareto_k, psis.elpd_i, exact.elpd_i]),
                       header='seed %d; fit + PSIS-LOO %.1f s; %d refits %.1f s; p_loo PSIS %.6f exact %.6f\nf / Hz, pareto_k, PSIS elpd_i, exact-refit elpd_i'
                       % (seed, t1 - t0, len(f), t2 - t1, psis.p_loo, exact.p_loo))
    have = sorted(int(n[len('agreement_seed'):-4]) for n in os.listdir(OUT) if n.startswith('agreement_seed') and n.endswith('.txt'))
    tabs = {s_: np.loadtxt(os.path.join(OUT, 'agreement_seed%d.txt' % s_)) for s_ in have}
    heads = {s_: open(os.path.join(OUT, 'agreement_seed%d.txt' % s_)).readline().strip('# \n') for s_ in have}
    lines = ['one synthetic spectrum of the benchmark (2 ZARC elements + noise, fitted by the model family that generated it: well specified),',
             '%d frequencies x %d basis functions, nonneg=True, 4 chains x 250 draws after 200 warm-up; reff=auto; reloo(k_threshold=-inf, max_refits=None)'
             % (len(f), len(basis)), 'seeds run: %s%s' % (have, '' if len(have) > 1 else ' -- ONE seed only: there is no seed-to-seed column yet'), '']
    lines += [heads[s_] for s_ in have] + ['']
    for s_ in have:
        t = tabs[s_]
        d = t[:, 2] - t[:, 3]
        n = len(t)
        lines.append('seed %d: elpd_loo PSIS %.3f (se %.3f), exact %.3f (se %.3f); units with k > 0.7: %d; |PSIS - exact| largest %.3f, median %.3f'
                     % (s_, t[:, 2].sum(), np.sqrt(n * np.var(t[:, 2])), t[:, 3].sum(), np.sqrt(n * np.var(t[:, 3])), int(np.sum(t[:, 1] > 0.7)),
                        np.max(np.abs(d)), np.median(np.abs(d))))
    if len(have) > 1:
        a, b = tabs[have[0]], tabs[have[1]]
        lines.append('largest seed-to-seed |difference|: PSIS %.3f, exact %.3f' % (np.max(np.abs(a[:, 2] - b[:, 2])), np.max(np.abs(a[:, 3] - b[:, 3]))))
    lines += ['', '    f / Hz |' + ' |'.join('  k (s%d)  PSIS s%d  exact s%d     diff' % (s_, s_, s_) for s_ in have) +
              (' | seed diff PSIS    exact' if len(have) > 1 else '')]
    for i in range(len(tabs[have[0]])):
        row = '%10.4g |' % tabs[have[0]][i, 0] + ' |'.join('  %7.2f  %7.3f  %8.3f  %7.3f' % (t[i, 1], t[i, 2], t[i, 3], t[i, 2] - t[i, 3])
                                                           for t in (tabs[s_] for s_ in have))
        if len(have) > 1:
            row += ' | %14.3f  %7.3f' % (a[i, 2] - b[i, 2], a[i, 3] - b[i, 3])
        lines.append(row)
    lines += ['', 'Recorded, not asserted: the Monte Carlo error of either side is unmeasured; the seed-to-seed column is its only witness here.']
    _write('agreement.txt', 'PSIS-LOO elpd_i against exact-refit elpd_i, every frequency (MI355X, gfx950; tools/heldout_timing.py agreement)\n\n', lines)


def _write(name, head, lines):
    os.makedirs(OUT, exist_ok=True)
    out = OUT
    with open(os.path.join(out, name), 'w') as fh:
        fh.write(head + '\n'.join('  ' + ln if ln else '' for ln in lines) + '\n')
    print('wrote', os.path.join(out, name))


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'time'
    if mode == 'time':
        logging.basicConfig(level=logging.WARNING, format='%(asctime)s %(message)s')
        logging.getLogger('bayes_drt_amd').setLevel(logging.ERROR)
        logging.getLogger('bayes_drt_amd.kfold').setLevel(logging.INFO)      # one line per fold
        time_main(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == 'agreement':
        logging.basicConfig(level=logging.WARNING, format='%(asctime)s %(message)s')
        logging.getLogger('bayes_drt_amd').setLevel(logging.ERROR)
        logging.getLogger('bayes_drt_amd.reloo').setLevel(logging.INFO)      # one line per refit
        # (`agreement merge`: no run, the record from the seeds that are there)
        agreement_main([] if sys.argv[2:] == ['merge'] else ([int(a) for a in sys.argv[2:]] or [5, 6]))
    else:
        sys.exit(__doc__)
