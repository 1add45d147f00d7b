"""Time the PSIS-LOO reductions (bdrt_loo.hip) on the shapes of DESIGN.md section 3.5c.

    python tools/loo_timing.py            # host clock around calls that end in a device synchronise and the copy back
    python tools/loo_timing.py launch     # the large launch only, once -- under `rocprofv3 --kernel-trace --stats -- python ...`
                                          # for the device times of the kernels

Shapes: `loo_many` over the published study (60 spectra, 4 chains x 1000 draws, 81 frequencies; synthetic Z_hat / sigma_tot
draws, so the sampler is not part of the time) and one `bdrt_psis_loo` launch over the 512-spectrum batch (41 472 columns x
8000 draws), next to `post.percentile` over a matrix of the same bytes, alternating, in one process.  The numpy statement is
timed on one core for 40 columns and scaled."""
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayes_drt_amd import loo as L, post  # noqa: E402
from bayes_drt_amd.engine import SavedFit  # noqa: E402
from tests import psis_numpy as pn  # noqa: E402


def study(rng):
    nfit, S, Nf = 60, 4000, 81
    fits, zs = [], []
    for _ in range(nfit):
        z = rng.standard_normal(2 * Nf)
        sg = np.exp(rng.normal(np.log(3e-3), 0.2, (S, 2 * Nf)))
        fits.append(SavedFit({'Z_hat': z + 0.7 * sg * rng.standard_normal((S, 2 * Nf)), 'sigma_tot': sg}, 4, 1000))
        zs.append(z)
    L.loo_many(fits[:2], zs[:2])                                          # warm-up (module load, LDS attribute)
    for reff in ('auto', None):
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            L.loo_many(fits, zs, reff=reff)
            walls.append(time.perf_counter() - t0)
        print('loo_many, 60 fits x 4000 draws x 81 frequencies, reff=%s: %.3f ... %.3f s' % (reff, min(walls), max(walls)),
              flush=True)
    t0 = time.perf_counter()
    for f, z in zip(fits[:10], zs[:10]):
        L.loo(f, z)
    print('the first 10 of them through loo(), one call each: %.3f s' % (time.perf_counter() - t0), flush=True)


def launch(rng, reps):
    G, S, N = 512, 8000, 81
    ll = np.empty((G, S, N))
    for g in range(G):
        ll[g] = rng.standard_normal((S, N), dtype=np.float32) * 1.3 + 5.0
    X = ll.reshape(S, G * N)                                              # the same bytes as [draws, columns]
    q = np.array([2.5, 50.0, 97.5])
    L.psis_loo(ll[:1])
    post.percentile(X[:, :N], q, axis=0)
    for _ in range(reps):
        t0 = time.perf_counter()
        p = L.psis_loo(ll)
        a = time.perf_counter() - t0
        t0 = time.perf_counter()
        post.percentile(X, q, axis=0)
        b = time.perf_counter() - t0
        print('%d columns x %d draws (%.2f GB): psis_loo call %.3f s, post.percentile call %.3f s, both with the copy to the '
              'device' % (G * N, S, ll.nbytes / 1e9, a, b), flush=True)
    print('n_tail %d ... %d, k-hat %.2f ... %.2f' % (p['n_tail'].min(), p['n_tail'].max(), np.nanmin(p['pareto_k']),
                                                    np.nanmax(p['pareto_k'])), flush=True)
    t0 = time.perf_counter()
    pn.loo(ll[0, :, :40])
    print('numpy statement, one core, 40 columns timed and scaled to %d: %.0f s' % (G * N, (time.perf_counter() - t0) * G * N / 40),
          flush=True)


def main():
    logging.getLogger('bayes_drt_amd').setLevel(logging.ERROR)
    rng = np.random.default_rng(0)
    only_launch = len(sys.argv) > 1 and sys.argv[1] == 'launch'
    if not only_launch:
        study(rng)
    launch(rng, 1 if only_launch else 3)


if __name__ == '__main__':
    main()
