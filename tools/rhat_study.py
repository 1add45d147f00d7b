"""How often the automatic check's R-hat warning fires on the published fits (Run fits.ipynb cells 5 and 14 settings:
2 chains x (200 + 200), random init), over five seeds; and what the check costs in wall time.

  trunc   the ten 53-frequency truncated spectra (cell 14; sigma_min 0.005 for the noiseless one, nonneg off), one fit_many per
          seed: spectra whose check reports R-hat (pystan: every one of them), the largest Rhat of each spectrum
  study   the 60 spectra of cell 5 (tests/golden/hmc_suite.npz), one fit_many per seed: their flat count is above 1000, so
          the check skips n_eff / Rhat as pystan did; the largest Rhat over all columns is computed here with fit.summary()
Prints one JSON line per part."""
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import load  # noqa: E402

SEEDS = (1234, 1, 2, 3, 4)
TRUNC = ['trunc_%s_%s' % (k, n) for k in ('Macdonald', 'Orazem', 'uniform') for n in ('0.25', '1.0', '2.5')] + ['trunc_noiseless']


def trunc_study(Inverter):
    fs, zs, sm = [], [], []
    for n in TRUNC:
        d = load('kat_' + n)
        fs.append(np.array(d['data_freq'], dtype=float)); zs.append(np.array(d['data_Z']))
        sm.append(0.005 if 'noiseless' in n else 0.002)
    assert all(len(f) == 53 and np.array_equal(f, fs[0]) for f in fs)
    basis = np.logspace(6, -2, 81)
    fired, maxr, walls = [], [], {}
    for seed in SEEDS:
        for check in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                t0 = time.time()
                views = Inverter(basis_freq=basis).fit_many(fs[0], zs, sigma_min=sm, nonneg=False, mode='sample', warmup=200,
                                                            samples=200, chains=2, random_seed=seed, check_diagnostics=check)
                walls.setdefault(check, []).append(time.time() - t0)
        fired.append([not v._sample_result.hmc_check['Rhat'] for v in views])
        maxr.append([float(np.nanmax(v._sample_result.hmc_check['Rhat_values'])) for v in views])
    return dict(part='trunc', spectra=TRUNC, seeds=list(SEEDS), rhat_warning=np.array(fired).astype(int).tolist(),
                fired_fraction=float(np.mean(fired)), max_rhat=np.round(maxr, 3).tolist(),
                wall_s_check_off=np.round(walls[False], 2).tolist(), wall_s_check_on=np.round(walls[True], 2).tolist())


def study_60(Inverter):
    S = load('hmc_suite')
    stems = [str(s) for s in S['stems']]
    f = S['Z'][0][:, 0]
    Z = [S['Z'][i][:, 1] + 1j * S['Z'][i][:, 2] for i in range(len(stems))]
    nonneg = [not s.startswith('ZARC-RL') for s in stems]
    smin = [0.005 if 'noiseless' in s else 0.002 for s in stems]
    maxr, walls = [], {}
    for seed in SEEDS:
        for check in (False, True):
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                t0 = time.time()
                views = Inverter(basis_freq=f).fit_many(f, Z, nonneg=nonneg, sigma_min=smin, mode='sample', warmup=200, samples=200,
                                                        chains=2, random_seed=seed, check_diagnostics=check)
                walls.setdefault(check, []).append(time.time() - t0)
        maxr.append([float(np.nanmax(v._sample_result.summary()['summary'][:, -1])) for v in views])
    m = np.array(maxr)
    return dict(part='study60', seeds=list(SEEDS), max_rhat_per_seed=np.round(m.max(axis=1), 3).tolist(),
                spectra_above_1p1_per_seed=(m > 1.1).sum(axis=1).tolist(), median_of_spectrum_max=float(np.median(m)),
                wall_s_check_off=np.round(walls[False], 2).tolist(), wall_s_check_on=np.round(walls[True], 2).tolist())


def main():
    from bayes_drt_amd.inversion import Inverter
    for fn in (trunc_study, study_60):
        print(json.dumps(fn(Inverter)), flush=True)


if __name__ == '__main__':
    main()
