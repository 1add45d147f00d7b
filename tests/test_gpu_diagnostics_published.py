"""Published behaviour of the automatic check (-m gpu), measured with tools/rhat_study.py (profiles/diag/rhat_study.txt).

pystan printed the R-hat warning after every truncated-spectrum fit of Run fits.ipynb cell 14 (2 chains x (200 + 200)).  Ours,
over five seeds on the ten 53-frequency spectra: 41 of 50 fits (per seed 6, 9, 8, 8, 10 of 10); the fits where it stays quiet
have a largest Rhat of 1.06 ... 1.099, just under the threshold.  The 60-spectrum study (cell 5) is above 1000 flat names, so
pystan and the automatic check skip n_eff / Rhat there; computed anyway, its largest Rhat is 1.19 ... 57.9 per seed, with 5 to
16 spectra above 1.1.  The bands below are those the measurement clearly supports."""
import logging
import warnings

import numpy as np
import pytest

from tests.helpers import load

pytestmark = pytest.mark.gpu
SEEDS = (1234, 1, 2, 3, 4)
TRUNC = ['trunc_%s_%s' % (k, n) for k in ('Macdonald', 'Orazem', 'uniform') for n in ('0.25', '1.0', '2.5')] + ['trunc_noiseless']


def test_rhat_warning_fires_on_most_truncated_spectrum_fits(caplog):
    from bayes_drt_amd import diagnostics as dg
    from bayes_drt_amd.inversion import Inverter
    fs, zs, sm = [], [], []
    for n in TRUNC:
        d = load('kat_' + n)
        fs.append(np.array(d['data_freq'], dtype=float)); zs.append(np.array(d['data_Z']))
        sm.append(0.005 if 'noiseless' in n else 0.002)
    fired = []
    for seed in SEEDS:
        caplog.clear()
        with warnings.catch_warnings(), caplog.at_level(logging.WARNING, logger='bayes_drt_amd'):
            warnings.simplefilter('ignore')
            views = Inverter(basis_freq=np.logspace(6, -2, 81)).fit_many(fs[0], zs, sigma_min=sm, nonneg=False, mode='sample',
                                                                        warmup=200, samples=200, chains=2, random_seed=seed)
        lines = [r.getMessage() for r in caplog.records]
        f = [not v._sample_result.hmc_check['Rhat'] for v in views]
        # the logged line and the check's verdict agree spectrum by spectrum
        assert [('spectrum %d: ' % i + dg.RHAT_MESSAGE) in lines for i in range(len(views))] == f
        fired.append(f)
    fired = np.array(fired)
    print('R-hat warning on the truncated spectra, per seed:', fired.sum(axis=1).tolist(), 'of', fired.shape[1])
    assert fired.mean() >= 0.6 and fired.sum(axis=1).min() >= 4


def test_sixty_spectrum_study_has_unmixed_chains_that_the_skip_hides():
    from bayes_drt_amd import diagnostics as dg
    from bayes_drt_amd.inversion import Inverter
    S = load('hmc_suite')
    stems = [str(s) for s in S['stems']]
    f = S['Z'][0][:, 0]
    Z = [S['Z'][i][:, 1] + 1j * S['Z'][i][:, 2] for i in range(len(stems))]
    nonneg = [not s.startswith('ZARC-RL') for s in stems]
    smin = [0.005 if 'noiseless' in s else 0.002 for s in stems]
    for seed in SEEDS[:2]:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            views = Inverter(basis_freq=f).fit_many(f, Z, nonneg=nonneg, sigma_min=smin, mode='sample', warmup=200, samples=200,
                                                    chains=2, random_seed=seed)
        assert dg.flat_parameter_count(views[0].stan_model_name, views[0]._stan_input) > dg.MAX_FLAT
        assert all(v._sample_result.hmc_check['Rhat_values'] is None for v in views)       # skipped, as pystan did
        m = np.array([np.nanmax(v._sample_result.summary()['summary'][:, -1]) for v in views])
        print('seed %d: largest Rhat %.3f, %d spectra above 1.1' % (seed, m.max(), (m > 1.1).sum()))
        assert m.max() > 1.1 and 1 <= (m > 1.1).sum() <= 30
