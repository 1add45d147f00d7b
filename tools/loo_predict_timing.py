"""Time the LOO predictive checks (bdrt_loo_predict.hip) on the published study's shape, DESIGN.md section 3.5e.

    python tools/loo_predict_timing.py    # host clock around calls that end in a device synchronise and the copy back

`loo_predict_many` over 60 fits (4 chains x 1000 draws, 81 frequencies; synthetic Z_hat / sigma_tot draws as in
tools/loo_timing.py, so the sampler is not part of the time), the existing `loo_many` on the same arrays, and the numpy
statement's loop (tests/loo_predict_numpy.py) on one core, timed for 3 of the fits and scaled."""
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayes_drt_amd import loo as L  # noqa: E402
from bayes_drt_amd.engine import SavedFit  # noqa: E402
from tests import loo_predict_numpy as lp  # noqa: E402


def main():
    logging.getLogger('bayes_drt_amd').setLevel(logging.ERROR)
    rng = np.random.default_rng(0)
    nfit, S, Nf = 60, 4000, 81
    fits, zs = [], []
    for _ in range(nfit):
        z = rng.standard_normal(2 * Nf)
        sg = np.exp(rng.normal(np.log(3e-3), 0.2, (S, 2 * Nf)))
        fits.append(SavedFit({'Z_hat': z + 0.7 * sg * rng.standard_normal((S, 2 * Nf)), 'sigma_tot': sg}, 4, 1000))
        zs.append(z)
    L.loo_predict_many(fits[:2], zs[:2])                                    # warm-up (module load, LDS attribute)
    L.loo_many(fits[:2], zs[:2])
    for name, fn in (('loo_predict_many', L.loo_predict_many), ('loo_many', L.loo_many)):
        for reff in ('auto', None):
            walls = []
            for _ in range(3):
                t0 = time.perf_counter()
                res = fn(fits, zs, reff=reff)
                walls.append(time.perf_counter() - t0)
            print('%s, 60 fits x 4000 draws x 81 frequencies, reff=%s: %.3f ... %.3f s' % (name, reff, min(walls), max(walls)),
                  flush=True)
        if name == 'loo_predict_many':
            k = np.concatenate([r.pareto_k for r in res])
            print('  n_tail %d ... %d, k-hat %.2f ... %.2f' % (min(r.n_tail.min() for r in res), max(r.n_tail.max() for r in res),
                                                              k.min(), k.max()), flush=True)
    t0 = time.perf_counter()
    for f, z in zip(fits[:3], zs[:3]):
        lp.predict(f['Z_hat'], f['sigma_tot'], z, 'frequency')
    print('numpy statement, one core, 3 fits timed and scaled to 60: %.1f s' % ((time.perf_counter() - t0) * 20), flush=True)


if __name__ == '__main__':
    main()
