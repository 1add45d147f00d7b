"""Problems, points and evaluator cases of the per-class tests of the log-posterior evaluators: tests/test_logp_reference_host.py
measures the float64 references on them on the CPU, tests/test_gpu_logp_classes.py holds every evaluator to the longdouble statement
(tests/logp_numpy.py) on the same ones.  Test infrastructure, not the product.

Every matrix comes from the goldens or from the oracle's constructors (no GPU needed), so both files see the same bits; L is made
exactly Toeplitz before anyone reads it (exactly_toeplitz).  The shapes
are the smallest that reach each path (CASES); the points of a synthetic or `dat` problem are 19 rows (one full 16-column tile and a
ragged one) in three point sets, those of a stored fit five rows in one:
  init      13 rows uniform(-2, 2), Stan's initialisation range;
  random    tests/hessian_shapes.py::random_point;
  near_map  tests/hessian_shapes.py::near_map_point and four copies perturbed by 0.1 N(0, 1);
  map       the stored Stan MAP om.unconstrain(k['params']) and four copies perturbed by 0.1 N(0, 1)."""
import functools
import zlib

import numpy as np

from tests import hessian_shapes as hs
from tests.helpers import kat_to_model, load
from tests.logp_numpy import class_slices, reference

POINT_SETS = ('init', 'random', 'near_map', 'map')
SO_KW = ('outlier_mode', 'so_lambda', 'so_alpha', 'so_beta')


def _orc():
    from oracle import oracle as orc
    return orc


def _orc_A(f, part, tau, eps):
    return _orc().construct_A(f, part, tau=tau, epsilon=eps)


def _orc_L(bf, tau, eps, order):
    return _orc().construct_L(tau, eps, order)


def _pack(name, A, L, Z, f, pos, kw):
    A = np.ascontiguousarray(A, dtype=float); L = tuple(np.ascontiguousarray(Li, dtype=float) for Li in L)
    f = np.ascontiguousarray(f, dtype=float)
    kw = dict(dict(induc_scale=1.0, outlier_mode=0, so_lambda=10.0, so_alpha=5.0, so_beta=1.0), **kw)
    return dict(name=name, A=A, L=L, Z=np.ascontiguousarray(Z, dtype=float), f=f, w=2 * np.pi * f, pos=pos, K=A.shape[1], nf=len(f), kw=kw,
                blk=dict(A=A, L0=L[0], L1=L[1], L2=L[2], nonneg=pos))


def _outlier_kw(mode):
    if not mode:
        return {}
    so = load('dat_sample_outlier_scalars')
    return dict(outlier_mode=mode, so_lambda=float(so['sigma_out_lambda']), so_alpha=float(so['sigma_out_alpha']),
                so_beta=float(so['sigma_out_beta']))


def _dat(name, mode, tag, pos, outlier=0):
    d = load('dat_%s_2ZARC_uniform_0.25_%s' % (mode, tag))
    kw = dict(sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']), ups_beta=float(d['ups_beta']),
              induc_scale=float(d['induc_scale']), **_outlier_kw(outlier))
    return _pack(name, d['A'], (d['L0'], d['L1'], d['L2']), d['Z'], d['freq'], pos, kw)


def _log_uniform(name, nf, K, pos=True, outlier=0):
    """tests/test_gpu_model.py::_log_uniform_problem with the oracle's constructors: log-uniform grids of equal spacing, A exactly
    Toeplitz, the basis bracketing the measured range."""
    orc = _orc()
    ppd = 10.0
    f = 10.0 ** (6.0 - np.arange(nf) / ppd)
    bf = 10.0 ** (6.0 + ((K - nf) // 2) / ppd - np.arange(K) / ppd)
    tau = 1 / (2 * np.pi * bf); eps = 1 / np.mean(np.diff(np.log(tau)))
    A = np.vstack([orc.construct_A(f, 'real', tau=tau, epsilon=eps), orc.construct_A(f, 'imag', tau=tau, epsilon=eps)])
    L = [orc.construct_L(tau, eps, o) for o in (0, 1, 2)]
    rng = np.random.default_rng(nf * 1000 + K)
    Z = np.concatenate([1.0 + rng.random(nf), -rng.random(nf)]) + 0.01 * rng.standard_normal(2 * nf)
    return _pack(name, A, (L[0], L[1], 0.75 * L[2]), Z, f, pos, dict(sigma_min=0.002, ups_alpha=1.0, ups_beta=0.1, **_outlier_kw(outlier)))


def _shape(name, nf, K, pos, irregular):
    A, L, Z, f = hs.make_shape(nf, K, irregular, _orc_A, _orc_L)
    return _pack(name, A, L, Z, f, pos, dict(hs.KW))


def _kat(name):
    k = kat_to_model(name)
    kw = k['kw']
    assert len(kw['blocks']) == 1 and not kw['blocks'][0]['parallel'] and not kw['use_x_sum'] and not kw['outlier_mode'] and k['has_Z']
    b = kw['blocks'][0]
    P = _pack(name, b['A'], (b['L0'], b['L1'], b['L2']), kw['Z'], kw['freq'], bool(b['nonneg']),
              dict(sigma_min=kw['sigma_min'], ups_alpha=kw['ups_alpha'], ups_beta=kw['ups_beta'], induc_scale=kw['induc_scale']))
    P['params'] = np.asarray(k['params'], dtype=float)
    return P


_BUILDERS = {
    'dat_sample_K81': lambda n: _dat(n, 'sample', 'K81', True),
    'dat_optimize_K81': lambda n: _dat(n, 'optimize', 'K81', True),
    'dat_sample_K81_free': lambda n: _dat(n, 'sample', 'K81', False),
    'dat_sample_K101': lambda n: _dat(n, 'sample', 'K101', True),
    'dat_sample_K101_free': lambda n: _dat(n, 'sample', 'K101', False),
    'dat_sample_K81_so1': lambda n: _dat(n, 'sample', 'K81', True, 1),
    'dat_sample_K81_so2': lambda n: _dat(n, 'sample', 'K81', True, 2),
    'lu80x80': lambda n: _log_uniform(n, 80, 80),
    'lu82x162': lambda n: _log_uniform(n, 82, 162),
    'lu33x47': lambda n: _log_uniform(n, 33, 47),
    'lu16x16': lambda n: _log_uniform(n, 16, 16),
    'lu33x47_so1': lambda n: _log_uniform(n, 33, 47, outlier=1),
    'lu33x47_so2': lambda n: _log_uniform(n, 33, 47, outlier=2),
    'hs33x90': lambda n: _shape(n, 33, 90, True, False),
    'hs37x61_irr': lambda n: _shape(n, 37, 61, True, True),
    'RC-ZARC_uniform_0.25': _kat,           # 41 x 51, x >= 0
    'trunc_uniform_0.25': _kat,             # 53 x 81, free x
    'LIB_data': _kat,                       # 107 x 91, free x, irregular frequencies
}
KAT = ('RC-ZARC_uniform_0.25', 'trunc_uniform_0.25', 'LIB_data')


def exactly_toeplitz(L):
    """L with every diagonal made constant: the entry of that diagonal nearest the middle row.  On a log-uniform tau grid L is
    Toeplitz by construction, but the constructors' entries vary along a diagonal by 1e-14 .. 4e-14 of the largest (rounding of
    ln(tau_m / tau_n)), and the structured L path of the library reads each diagonal as ONE number (csrc/bdrt_model.hip, admitted up
    to 1e-12 of the largest entry) where the dense path, the oracle and the statement read every entry.  With constant diagonals
    every reader evaluates the same matrix, whichever row it takes a diagonal from, and the comparison is about arithmetic alone;
    what the reading costs against L as constructed is measured on the CPU (tests/test_logp_reference_host.py)."""
    K = L.shape[0]
    out = np.empty_like(L)
    for d in range(-(K - 1), K):
        r = np.arange(max(0, -d), min(K, K - d))
        mid = r[np.argmin(np.abs(r - K // 2))]
        out[r, r + d] = L[mid, mid + d]
    return out


@functools.lru_cache(maxsize=None)
def problem(name, as_constructed=False):
    """the problem every side is given: L made exactly Toeplitz (as_constructed: the constructors' / goldens' L untouched)"""
    P = _BUILDERS[name](name)
    if not as_constructed:
        L = tuple(exactly_toeplitz(Li) for Li in P['L'])
        P = dict(P, L=L, blk=dict(P['blk'], L0=L[0], L1=L[1], L2=L[2]))
    return P


def _with_outlier_rows(y, K, nf, mode):
    """a point of the plain layout with the 2 nf outlier parameters put in: small and smooth, as at a fit without outliers"""
    if not mode:
        return y
    n = np.arange(nf) / max(nf - 1.0, 1.0)
    if mode == 1:
        so = np.concatenate([0.3 + 0.2 * np.sin(2 * np.pi * n + 0.7), 0.25 + 0.1 * np.cos(2 * np.pi * n)])     # raw, scale
    else:
        so = np.concatenate([0.10 + 0.05 * np.sin(2 * np.pi * n + 0.7), 0.12 + 0.05 * np.cos(2 * np.pi * n)])  # re rows, im rows
    return np.concatenate([y[:6 + K], np.log(so), y[6 + K:]])


@functools.lru_cache(maxsize=None)
def points(name):
    """(thetas [n, D], point set of every row)"""
    P = problem(name)
    K, nf, mode = P['K'], P['nf'], P['kw']['outlier_mode']
    D = class_slices(K, nf, mode)['d'].stop
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name in KAT:
        th0 = np.where(_is_pos(P), np.log(np.where(_is_pos(P), P['params'], 1.0)), P['params'])
        rows = [th0] + [th0 + 0.1 * rng.standard_normal(D) for _ in range(4)]
        sets = ['map'] * 5
    else:
        nm = _with_outlier_rows(hs.near_map_point(K, P['pos']), K, nf, mode)
        rows = list(rng.uniform(-2, 2, (13, D))) + [hs.random_point(D), nm] + [nm + 0.1 * rng.standard_normal(D) for _ in range(4)]
        sets = ['init'] * 13 + ['random'] + ['near_map'] * 5
    th = np.ascontiguousarray(np.stack(rows))
    th.setflags(write=False)
    return th, tuple(sets)


def _is_pos(P):
    sl = class_slices(P['K'], P['nf'], P['kw']['outlier_mode'])
    pos = np.ones(sl['d'].stop, dtype=bool)
    if not P['pos']:
        pos[sl['x']] = False
    return pos


@functools.lru_cache(maxsize=None)
def references(name, jacobian, as_constructed=False):
    """the longdouble statement at every point of the problem, computed once and shared"""
    P = problem(name, as_constructed)
    return tuple(reference(P, y, jacobian) for y in points(name)[0])


def oracle_model(name):
    P = problem(name)
    return _orc().OracleModel([P['blk']], P['Z'], P['f'], **P['kw'])


# ---- the evaluator cases of tests/test_gpu_logp_classes.py ---------------------------------------------------------------------------
# (path, problem, environment at Problem(...), expected bdrt_problem_evaluator code, entry, rows)
#   entry: 'tile' Problem.logp_grad with BDRT_FEW_POINTS=0; 'few' Problem.logp_grad with BDRT_FEW_POINTS unset; 'solo' / 'wave' the
#   debug entries of the one-chain evaluators.  rows: indices into points(problem) making the batch (None: all of them).
FEW_1 = (14,)                                    # B = 1: the near-MAP point
FEW_5 = (0, 13, 14, 15, 18)                      # B = 5: an init row, the random point, near-MAP and two perturbed copies
FEW_300 = tuple(int(i) for i in np.arange(300) % 19)    # B = 300; rows 0, 150 and 299 are compared (points 0, 17 and 14)
FEW_300_COMPARED = (0, 150, 299)
STREAM, GENERIC, DENSE, BIG = dict(BDRT_STREAM_A='1'), dict(BDRT_GENERIC_TILE='1'), dict(BDRT_GENERIC_TILE='1', BDRT_DENSE_L='1'), dict(BDRT_BIG='1')
CASES = [
    ('table default', 'dat_sample_K81', {}, 4, 'tile', None),
    ('table default', 'dat_optimize_K81', {}, 4, 'tile', None),
    ('table default', 'lu80x80', {}, 4, 'tile', None),
    ('table default', 'lu82x162', {}, 4, 'tile', None),
    ('table general', 'RC-ZARC_uniform_0.25', {}, 4, 'tile', None),
    ('table general', 'lu33x47', {}, 4, 'tile', None),
    ('table general', 'trunc_uniform_0.25', {}, 4, 'tile', None),
    ('streamed fragments', 'dat_sample_K81', STREAM, 2, 'tile', None),
    ('streamed fragments', 'lu16x16', {}, 2, 'tile', None),
    ('generic banded L', 'hs33x90', GENERIC, 1, 'tile', None),
    ('generic dense L', 'hs33x90', DENSE, 0, 'tile', None),
    ('irregular', 'hs37x61_irr', {}, 2, 'tile', None),
    ('irregular', 'LIB_data', {}, 2, 'tile', None),
    ('streamed evaluator', 'hs33x90', BIG, 5, 'tile', None),
    ('workgroup per point B=1', 'dat_sample_K81', {}, 4, 'few', FEW_1),
    ('workgroup per point B=5', 'dat_sample_K81', {}, 4, 'few', FEW_5),
    ('workgroup per point B=300', 'dat_sample_K81', {}, 4, 'few', FEW_300),
    ('solo', 'dat_sample_K81', {}, None, 'solo', None),
    ('solo', 'dat_sample_K81_free', {}, None, 'solo', None),
    ('solo', 'dat_sample_K101', {}, None, 'solo', None),
    ('solo', 'dat_sample_K101_free', {}, None, 'solo', None),
]
for _occ in ('1', '2'):
    CASES += [('wave occ %s' % _occ, n, dict(BDRT_WAVE_OCC=_occ), None, 'wave', None)
              for n in ('dat_sample_K81', 'dat_sample_K81_free', 'dat_sample_K101', 'dat_sample_K101_free')]
CASES += [
    ('outliers 1 fast tile', 'dat_sample_K81_so1', {}, 4, 'tile', None),
    ('outliers 2 fast tile', 'dat_sample_K81_so2', {}, 4, 'tile', None),
    ('outliers 1 generic tile', 'lu33x47_so1', GENERIC, 1, 'tile', None),
    ('outliers 2 generic tile', 'lu33x47_so2', GENERIC, 1, 'tile', None),
    ('outliers 1 wave', 'dat_sample_K81_so1', {}, None, 'wave', None),
    ('outliers 2 wave', 'dat_sample_K81_so2', {}, None, 'wave', None),
]
PROBLEMS = tuple(dict.fromkeys(c[1] for c in CASES))           # every problem a case uses, once


def has_outlier_model(name):
    return name.endswith(('_so1', '_so2'))


def case_id(case):
    return '%s-%s' % (case[0].replace(' ', '_'), case[1])


# ---- the references' ratios and the tolerances (measured and explained in tests/test_logp_reference_host.py) ------------------------
U = 2.0 ** -53
REF = {
    'init': {'lp': 4.6e-15, 'R': 1.2e-15, 'I': 3.4e-16, 'x': 7.6e-15, 'err': 1.3e-15, 'so': 1.1e-15, 'ups': 1.3e-14, 'd': 1.5e-15},
    'random': {'lp': 2.7e-15, 'R': 4.9e-16, 'I': 1.1e-16, 'x': 1.7e-15, 'err': 1.1e-15, 'so': 1.3e-15, 'ups': 4.1e-15, 'd': 1.1e-15},
    'near_map': {'lp': 7.9e-15, 'R': 1.5e-15, 'I': 3.5e-16, 'x': 5.2e-15, 'err': 2.0e-15, 'so': 5.5e-15, 'ups': 6.7e-15, 'd': 1.2e-15},
    'map': {'lp': 5.7e-15, 'R': 3.3e-14, 'I': 2.1e-14, 'x': 5.3e-14, 'err': 4.2e-14, 'ups': 2.3e-15, 'd': 1.1e-15},
}


def tol(point_set, cls, nf, K):
    """max(8 REF, twice the worst-case bound of a float64 sum of the longest top-level reduction in any order)"""
    n = 4 * nf + 4 * K if cls == 'lp' else nf + K
    return max(8 * REF[point_set][cls], 2 * n * U)
