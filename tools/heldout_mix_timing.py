"""Time K-fold cross-validation under the outlier error model against the plain model.

    python tools/heldout_mix_timing.py kfold [out.txt]     # -> profiles/heldout_mix/timing.txt
    python tools/heldout_mix_timing.py reduce [calls]      # the mixture reduce alone, for a kernel trace around it

`kfold`: one measured spectrum (49 frequencies) on a basis of K = 81, 4 chains x 250 draws, folds=3; host clock around whole calls, one
untimed call of each first, then three of each, alternating: `kfold(outliers=True, sigma_out='prior')` and `kfold(outliers=False)`.
`reduce`: `loo.heldout_mix_reduce` on arrays of one fold's shape (S = 1000 draws, 26 frequencies, both scalars of each), for
`rocprofv3 --kernel-trace --stats -- python tools/heldout_mix_timing.py reduce`, whose figure for heldout_mix_reduce_kernel is
the kernel time.  A record, not a threshold."""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'heldout_mix', 'timing.txt')
KW = dict(warmup=200, samples=250, chains=4, random_seed=5, check_diagnostics=False)
BASIS = np.logspace(6, -2, 81)


def spectrum():
    from tests.helpers import load
    d = load('kat_trunc_uniform_0.25')
    f, Z = np.array(d['data_freq'], dtype=float)[4:], np.array(d['data_Z'])[4:]
    o = np.argsort(f)[::-1]
    return f[o], Z[o]


def kfold_main(out):
    from bayes_drt_amd import loo
    from bayes_drt_amd.inversion import Inverter
    f, Z = spectrum()
    calls = {'outliers=True, sigma_out=\'prior\'': dict(outliers=True, sigma_out='prior'), 'outliers=False': dict(outliers=False)}
    times, res = {k: [] for k in calls}, {}
    for run in range(4):
        for name, kw in calls.items():
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                res[name] = Inverter(basis_freq=BASIS).kfold(f, Z, folds=3, **kw, **KW)
            dt = time.perf_counter() - t0
            print('run %d  %-36s %.2f s' % (run, name, dt), flush=True)
            if run:
                times[name].append(dt)
    lines = ['kfold(folds=3) of one spectrum, %d frequencies, K = %d, %d chains x %d draws (warm-up %d); host clock around the whole call,'
             % (len(f), len(BASIS), KW['chains'], KW['samples'], KW['warmup']),
             'one untimed call of each first, then three of each, alternating.  A record, not a threshold.', '']
    for name, ts in times.items():
        lines.append('  kfold(%-36s median %.2f s (%.2f ... %.2f) of %d   elpd_loo %.2f (se %.2f)'
                     % (name + ')', float(np.median(ts)), min(ts), max(ts), len(ts), res[name].elpd_loo, res[name].se))
    rows = loo.compare({'plain': res['outliers=False'], 'outliers': res["outliers=True, sigma_out='prior'"]})
    lines.append('  loo.compare: ' + '; '.join('%s elpd_diff %.2f dse %.2f' % (r['name'], r['elpd_diff'], r['dse']) for r in rows))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def reduce_main(calls):
    from bayes_drt_amd import loo
    rs = np.random.default_rng(0)
    S, H = KW['chains'] * KW['samples'], 26
    sig = 0.01 * np.exp(0.2 * rs.standard_normal((1, S, 2 * H)))
    Zh = 1.0 + 0.01 * rs.standard_normal((1, S, 2 * H))
    z = 1.0 + 0.01 * rs.standard_normal((1, 2 * H))
    tab = loo.sigma_out_table(1, 10.0, 5.0, 1.0)
    for _ in range(calls):
        t0 = time.perf_counter()
        r = loo.heldout_mix_reduce(Zh, sig, z, tab)
        print('heldout_mix_reduce: S = %d, %d frequencies, Q = %d: host-staged call %.2f ms' % (S, H, len(tab[0]), 1e3 * (time.perf_counter() - t0)))
    assert np.all(np.isfinite(r['lpd']))


if __name__ == '__main__':
    what = sys.argv[1] if len(sys.argv) > 1 else 'kfold'
    if what == 'kfold':
        kfold_main(sys.argv[2] if len(sys.argv) > 2 else OUT)
    elif what == 'reduce':
        reduce_main(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    else:
        sys.exit(__doc__)
