"""Cases shared by tests/test_heldout_host.py and tests/test_gpu_heldout.py: one golden Stan data dict per family, random
constrained parameter rows around the stored fit, held-out grids between the training frequencies, and the calibration of the
yardstick's own rounding error (tests/heldout_numpy.py in float64 against np.longdouble)."""
import functools

import numpy as np

from tests import heldout_numpy as hn
from tests.helpers import kat_to_model

# family -> (golden fit, edits of its blocks).  The golden fits hold no single-block Parallel model: that family is the
# Series_pos data with its one block read as an admittance.
FAMILIES = {
    'Series': ('trunc_uniform_0.25', None),
    'Series_pos': ('RC-ZARC_uniform_0.25', None),
    'Parallel': ('RC-ZARC_uniform_0.25', [dict(parallel=True, nonneg=True)]),
    'Series-Parallel': ('DRT-2-TpDDT_uniform_0.25', [dict(nonneg=False), {}]),
    'Series-Parallel_pos': ('DRT-2-TpDDT_uniform_0.25', None),
    'Series-2Parallel_pos': ('DRT-TpDDT-BpDDT_uniform_0.25', None),
}
HS = (1, 3, 17)                                      # 17: no multiple of any tile edge
BS = (1, 74, 5000)
LONGDOUBLE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def family(name):
    """dict(kw=Problem / OracleModel keyword arguments, params=the stored constrained parameter vector)"""
    kat, edits = FAMILIES[name]
    m = kat_to_model(kat)
    kw = dict(m['kw'])
    kw['blocks'] = [dict(b, **(e or {})) for b, e in zip(kw['blocks'], edits or [None] * len(kw['blocks']))]
    assert kw['outlier_mode'] == 0
    return dict(kw=kw, params=np.array(m['params'], dtype=float))


def rows(name, B, seed=0):
    """B constrained parameter rows: the stored fit with every entry scaled by exp(0.2 N(0, 1)) (signs and zeros stay)."""
    p = family(name)['params']
    return p[None, :] * np.exp(0.2 * np.random.default_rng(seed).standard_normal((B, len(p))))


def grid(name, H, seed=0):
    """H frequencies that are not on the training grid, each the geometric mean of two neighbours, and per block the stacked
    prediction rows [2 H, K]: the mean of the neighbours' rows (a smooth kernel's row at a frequency in between, closely)."""
    kw = family(name)['kw']
    f = np.asarray(kw['freq'], dtype=float)
    nf = len(f)
    i = np.sort(np.random.default_rng(100 + seed).choice(nf - 1, size=H, replace=False))
    A = []
    for b in kw['blocks']:
        Ab = np.asarray(b['A'], dtype=float)
        A.append(np.concatenate([0.5 * (Ab[i] + Ab[i + 1]), 0.5 * (Ab[nf + i] + Ab[nf + i + 1])]))
    return np.sqrt(f[i] * f[i + 1]), A


def train_grid(name):
    """The training grid itself with the problem's own A."""
    kw = family(name)['kw']
    return np.asarray(kw['freq'], dtype=float), [np.asarray(b['A'], dtype=float) for b in kw['blocks']]


def statement_error(blocks, params, freq, A, sigma_min, induc_scale):
    """The float64 statement and its own rounding error: (Z_hat, sigma_tot, e_Z, e_sigma, how).  e is the largest deviation of the
    float64 statement over the entries, relative to the largest magnitude of that output -- from the np.longdouble statement
    where that type is wider than float64, else from forward against reversed summation of the float64 statement."""
    args = (blocks, params, freq, A, sigma_min, induc_scale)
    if LONGDOUBLE:
        Zh, sg = hn.transformed(*args)
        ref, how = hn.transformed(*args, dtype=np.longdouble), 'longdouble'
    else:
        Zh, sg = hn.transformed(*args, reverse=False)
        ref, how = hn.transformed(*args, reverse=True), 'reversed summation'
    e = [float(np.max(np.abs(a.astype(r.dtype) - r)) / np.max(np.abs(r))) for a, r in zip((Zh, sg), ref)]
    return Zh, sg, e[0], e[1], how


def calibrate(name, params, freq, A):
    """`statement_error` of a family's problem."""
    kw = family(name)['kw']
    return statement_error(kw['blocks'], params, freq, A, kw['sigma_min'], kw['induc_scale'])
