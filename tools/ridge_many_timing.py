"""Timing of the reference's hyper-ridge study shape (code_EchemActa/comparisons/hyper-ridge/hyper-ridge run fits.ipynb):
60 spectra, 81 frequencies, K = 81; per spectrum a Re-Im cross-validation over 31 lambda_0 (ordinary ridge), then one
hyper-lambda fit from the chosen lambda_0.

    python tools/ridge_many_timing.py [--spectra 60] [--reps 5] [--out profiles/ridge_many/timing.txt]

Times, in one process, (a) the loop of `ridge_fit(lambda_0='cv', hyper_lambda=False)` + `ridge_fit(lambda_0=min_lam, hl_fbeta=...)`
calls and, where the build has it, (b) the one `ridge_fit_many` call per stage; each figure follows one warm-up call and is the
median of `--reps` repetitions.  The stages of (b) are timed by wrapping the methods it calls.  A build without
`ridge_fit_many` (the parent commit) reports (a) only: the loop needs no new code."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bayes_drt_amd.inversion import Inverter          # noqa: E402
from tests.helpers import load                        # noqa: E402

F_BETA = 0.1
CV_LAMBDAS = np.logspace(-10, 5, 31)


def spectra(n):
    Z = load('csv_2ZARC_uniform_0.25')['Z']
    f, z0 = Z[:, 0], Z[:, 1] + 1j * Z[:, 2]
    rs = np.random.RandomState(5)
    return f, [z0] + [z0 * (1.0 + 0.02 * k) + 0.003 * (rs.standard_normal(len(f)) + 1j * rs.standard_normal(len(f))) for k in range(1, n)]


def loop(f, zs):
    out = []
    for Z in zs:
        inv = Inverter(basis_freq=f)
        inv.ridge_fit(f, Z, lambda_0='cv', hyper_lambda=False, cv_lambdas=CV_LAMBDAS)
        lam = inv.cv_result['lambda'][np.argmin(inv.cv_result['totcv'])]
        inv.ridge_fit(f, Z, lambda_0=lam, hl_fbeta=F_BETA)
        out.append(inv)
    return out


def many(f, zs):
    base = Inverter(basis_freq=f)
    cv = base.ridge_fit_many(f, zs, lambda_0='cv', hyper_lambda=False, cv_lambdas=CV_LAMBDAS)
    lams = [v.cv_result['lambda'][np.argmin(v.cv_result['totcv'])] for v in cv]
    return base.ridge_fit_many(f, zs, lambda_0=lams, hl_fbeta=F_BETA)


class Stages:
    """wall time inside the stage methods of ridge_fit_many (scoring = what remains of the call)"""
    names = ('_ridge_setup_host', '_ridge_gram_many', '_ridge_solve_device')

    def __init__(self):
        self.t = {}
        self.saved = {k: Inverter.__dict__[k] for k in self.names}

    def __enter__(self):
        for k in self.names:
            raw = self.saved[k]
            fn = raw.__func__ if isinstance(raw, (staticmethod, classmethod)) else raw

            def timed(*a, _fn=fn, _k=k, **kw):
                t0 = time.perf_counter()
                try:
                    return _fn(*a, **kw)
                finally:
                    key = _k if _k != '_ridge_solve_device' else ('cv launch' if kw.get('history') is False else 'final launch')
                    self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
            setattr(Inverter, k, staticmethod(timed) if isinstance(raw, staticmethod) else timed)
        return self

    def __exit__(self, *exc):
        for k, raw in self.saved.items():
            setattr(Inverter, k, raw)


def median_time(fn, reps):
    fn()                                               # warm-up: library load, matrix builds, kernel attributes
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spectra', type=int, default=60)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    f, zs = spectra(a.spectra)
    lines = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        t_loop, all_loop = median_time(lambda: loop(f, zs), a.reps)
        rec = dict(spectra=a.spectra, nf=len(f), K=len(f), cv_lambdas=len(CV_LAMBDAS), reps=a.reps, loop_s=t_loop,
                   loop_all_s=all_loop)
        if hasattr(Inverter, 'ridge_fit_many'):
            t_many, all_many = median_time(lambda: many(f, zs), a.reps)
            ref, got = loop(f, zs), many(f, zs)
            same = all(np.array_equal(r.distribution_fits['DRT']['coef'], g.distribution_fits['DRT']['coef']) for r, g in zip(ref, got))
            stage_runs = []
            for _ in range(a.reps):
                with Stages() as st:
                    t0 = time.perf_counter(); many(f, zs); tot = time.perf_counter() - t0
                d = dict(st.t); d['scoring and views'] = tot - sum(st.t.values()); d['total'] = tot
                stage_runs.append(d)
            stages = {k: statistics.median(r.get(k, 0.0) for r in stage_runs) for k in stage_runs[0]}
            rec.update(many_s=t_many, many_all_s=all_many, ratio_loop_over_many=t_loop / t_many, bit_equal_coef=bool(same),
                       stages_s={{'_ridge_setup_host': 'host set-up', '_ridge_gram_many': 'gram'}.get(k, k): v for k, v in stages.items()})
    lines.append(json.dumps(rec))
    txt = '\n'.join(lines) + '\n'
    sys.stdout.write(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as fh:
            fh.write(txt)


if __name__ == '__main__':
    main()
