"""Time the HMC diagnostics kernel (bdrt_diag.hip) and the numpy statement on the shapes of DESIGN.md section 9.

    python tools/diag_timing.py            # under `rocprofv3 --kernel-trace --stats -- python ...` for the device times

Shapes: the published study (60 spectra x 2 chains x 200 draws x 1066 flat columns) and one eighth of the benchmark batch
(64 of the 512 spectra x 8 chains x 1000 draws x D = 331; the full batch is 10.8 GB of draws, eight such launches).
Draws are AR(1) series with mixed coefficients.  Prints one JSON line per shape."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bayes_drt_amd.diagnostics import column_diagnostics  # noqa: E402
from tests import diag_numpy as dn  # noqa: E402


def series(rng, G, M, N, C):
    phi = rng.choice([0.0, 0.5, 0.9], size=C)
    X = np.empty((G, M, N, C))
    X[:, :, 0] = rng.standard_normal((G, M, C))
    e = rng.standard_normal((G, M, N, C))
    for t in range(1, N):
        X[:, :, t] = phi * X[:, :, t - 1] + e[:, :, t]
    return X


def main():
    rng = np.random.default_rng(0)
    for G, M, N, C in ((60, 2, 200, 1066), (64, 8, 1000, 331)):
        X = series(rng, G, M, N, C)
        flat = X.reshape(G, M * N, C)
        column_diagnostics(flat[:1], M)                          # warm-up (module load, LDS attribute)
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            column_diagnostics(flat, M)
            walls.append(time.perf_counter() - t0)
        cols = min(C, 40)                                        # numpy statement on a sample of columns, scaled up
        t0 = time.perf_counter()
        dn.diagnostics(X[:1, :, :, :cols])
        t_np = (time.perf_counter() - t0) * G * C / cols
        print(json.dumps(dict(G=G, M=M, N=N, C=C, gbytes=X.nbytes / 1e9, wall_s_incl_copy=min(walls),
                              numpy_one_core_s_est=t_np)), flush=True)


if __name__ == '__main__':
    main()
