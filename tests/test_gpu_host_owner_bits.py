"""GPU test (-m gpu) that the entry points of the model object and of the ridge / QP / MAP-fit path keep their bits: every output
of bdrt_gram, bdrt_gram_batch, bdrt_qp_box_batch, bdrt_ridge_ex, bdrt_logp_grad, bdrt_transformed, bdrt_debug_hessian(_lin),
bdrt_optimize, bdrt_debug_sum_by_lane, bdrt_debug_lean_math and bdrt_build_A / _L / _M against the recorded fixture
tests/golden/host_owner_bits.npz, at the smallest shapes at which their host code takes another branch.

The fixture holds what the library answered before its host code was moved onto one owner per device buffer (DevBuf, upload,
download of bdrt_host.h; Problem owning its memory by members); it holds outputs only.  It was recorded twice from that library
and every output below came out the same both times, so every output is held to its bits.  The synthetic inputs are rebuilt
here from the integer recurrence of tests/test_gpu_post_stats_bits.py; the model problems are the stored ones (tests/golden) and
the smallest problem of tests/test_gpu_big.py.  BDRT_RECORD_HOST_OWNER=<file> writes the answers there instead of comparing them.

Rows of the ridge history beyond a fit's last iteration are never written by the entry (tests/test_gpu_ridge_many.py): they are
zeroed here before they are recorded or compared.

A failure prints the largest ulp distance of every output that differs."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tests.test_gpu_post_stats_bits import _uniform, _ulps

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'host_owner_bits.npz')
RECORD = os.environ.get('BDRT_RECORD_HOST_OWNER')
QP_NVEC = 14                                     # bdrt_qp.hip
LDS_LIMIT = (160 * 1024 - 2560) // 8             # doubles: what bdrt_qp_box_batch / bdrt_ridge_ex may take of the LDS


def _check(case, outs, fixture=FIXTURE, record=RECORD):
    """outs: {name: array} of one case, compared with (or recorded as) the fixture's '<case>/<name>'"""
    outs = {'%s/%s' % (case, k): np.asarray(v) for k, v in outs.items()}
    if record:
        table = dict(np.load(record)) if os.path.exists(record) else {}
        table.update(outs)
        np.savez_compressed(record, **table)
        return
    want = np.load(fixture)
    wrong = []
    for k, got in outs.items():
        ref = want[k]
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        if not np.array_equal(got, ref, equal_nan=got.dtype.kind == 'f'):
            d = _ulps(got, ref) if got.dtype.kind == 'f' else float(np.max(np.abs(got.astype(np.int64) - ref)))
            print('%s: largest distance %g ulp' % (k, d))
            wrong.append(k)
    assert not wrong, wrong


@pytest.fixture(scope='module')
def lib():
    from bayes_drt_amd import _lib
    return _lib.require_gpu()


def _call(lib, name, *args):
    from bayes_drt_amd import _lib
    return _lib.check(getattr(lib, name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]), name)


def _spd(seed, m, n):
    """[m, n, n]: M^T M + n I of uniform M [n + 3, n]"""
    M = _uniform(seed, (m, n + 3, n)) * 2.0
    return np.ascontiguousarray(np.einsum('mri,mrj->mij', M, M) + n * np.eye(n))


# ------------------------------------------------------------------------------------------------ gram
@pytest.mark.parametrize('what', ['P_L2', 'q_L1', 'both_plain'])
def test_gram_bits(lib, what):
    nrows, n = 5, 17                             # two 16-wide tiles
    WA, WZ = _uniform(101, (nrows, n)) * 3.0, _uniform(102, (nrows,))
    L2, L1 = _spd(103, 1, n)[0], _uniform(104, (n,)) + 0.5
    P, q = np.full((n, n), -7.0), np.full(n, -7.0)
    if what == 'P_L2':
        _call(lib, 'bdrt_gram', WA, None, nrows, n, L2, None, P, None)
        outs = {'P': P}
    elif what == 'q_L1':
        _call(lib, 'bdrt_gram', WA, WZ, nrows, n, None, L1, None, q)
        outs = {'q': q}
    else:
        _call(lib, 'bdrt_gram', WA, WZ, nrows, n, None, None, P, q)
        outs = {'P': P, 'q': q}
    _check('gram_' + what, outs)


@pytest.mark.parametrize('what', ['G', 'q_L1', 'both'])
def test_gram_batch_bits(lib, what):
    R, n, ng = 5, 17, 2
    A, w, t = _uniform(111, (R, n)) * 3.0, _uniform(112, (ng, R)) + 1.0, _uniform(113, (ng, R))
    L1 = _uniform(114, (n,)) + 0.5
    G, q = np.full((ng, n, n), -7.0), np.full((ng, n), -7.0)
    if what == 'G':
        _call(lib, 'bdrt_gram_batch', A, R, n, w, None, ng, None, G, None)
        outs = {'G': G}
    elif what == 'q_L1':
        _call(lib, 'bdrt_gram_batch', A, R, n, w, t, ng, L1, None, q)
        outs = {'q': q}
    else:
        _call(lib, 'bdrt_gram_batch', A, R, n, w, t, ng, None, G, q)
        outs = {'G': G, 'q': q}
    _check('gram_batch_' + what, outs)


# ------------------------------------------------------------------------------------------------ qp / ridge
def _qp_first_n_beyond_lds():
    n = 1
    while (QP_NVEC + 1) * ((n + 1) & ~1) + 32 + n * (n + 1) // 2 <= LDS_LIMIT:
        n += 1
    return n


def _ridge_first_n_beyond_lds():
    n = 1
    while (QP_NVEC + 1) * ((n + 1) & ~1) + 32 + n * (n + 1) // 2 + 6 * ((n + 1) & ~1) + 34 <= LDS_LIMIT:
        n += 1
    return n


@pytest.mark.parametrize('what', ['lo', 'nolo', 'beyond_lds'])
def test_qp_box_batch_bits(lib, what):
    n, nb = (_qp_first_n_beyond_lds(), 2) if what == 'beyond_lds' else (9, 3)
    assert what != 'beyond_lds' or n == 186
    P, q = _spd(121, nb, n), _uniform(122, (nb, n)) * 4.0
    lo = None if what == 'nolo' else np.concatenate([np.full(2, -10.0), np.zeros(n - 2)])
    x, obj, its = np.full((nb, n), -7.0), np.full(nb, -7.0), np.full(nb, -7, dtype=np.int32)
    _call(lib, 'bdrt_qp_box_batch', P, q, lo, n, nb, x, obj, its)
    _check('qp_' + what, {'x': x, 'obj': obj, 'its': its})


RIDGE_CASES = {
    # n, K, nb, ng, penalty, hyper_lambda, Ls, history, x0, max_iter
    'discrete_hist': (9, 7, 3, 2, 0, 1, True, True, False, 6),
    'discrete_x0_nohist': (9, 7, 3, 2, 0, 1, True, False, True, 6),
    'integral_noLs': (9, 7, 3, 2, 1, 1, False, True, True, 6),
    'single_qp_noLs': (9, 7, 3, 2, 0, 0, False, False, False, 6),
    'beyond_lds': (None, None, 2, 1, 1, 1, False, True, False, 2),
}


@pytest.mark.parametrize('case', list(RIDGE_CASES))
def test_ridge_ex_bits(lib, case):
    from bayes_drt_amd import _lib
    from bayes_drt_amd.inversion import Inverter
    n, K, nb, ng, penalty, hyper, with_Ls, hist, with_x0, mi = RIDGE_CASES[case]
    if n is None:
        n = _ridge_first_n_beyond_lds()
        K = n - 2
    off = n - K
    o = _lib.RidgeOptions()
    o.n, o.K, o.off, o.penalty, o.max_iter, o.hyper_lambda, o.xtol = n, K, off, penalty, mi, hyper, 1e-3
    for i in range(3):
        o.reg_ord[i] = (0.0, 1.0, 0.5)[i]
    G, qbase = _spd(131, ng, n), _uniform(132, (ng, n)) * 4.0
    gsel = np.ascontiguousarray(np.arange(nb) % ng, dtype=np.int32)
    zd = np.ascontiguousarray(np.arange(ng) % 2, dtype=np.uint8)
    fb = np.ascontiguousarray([0.0, 0.5, 0.0][:nb])
    base = _spd(133, 3, n) * 0.01
    Ls = np.ascontiguousarray(_uniform(134, (3, K, n))) if with_Ls else None
    lo = np.concatenate([np.full(2, -10.0), np.zeros(n - 2)])
    lam0 = np.ascontiguousarray([1e-2, 1e-1, 1e-2][:nb])
    terms = [Inverter._hyper_prior_terms('integral' if penalty else 'discrete', 5.0 if penalty else 2.5, l) for l in lam0]
    lam0s, betas = np.ascontiguousarray(np.stack([t[2] for t in terms])), np.ascontiguousarray(np.stack([t[3] for t in terms]))
    x0 = np.ascontiguousarray(_uniform(135, (nb, n)) + 0.6) if with_x0 else None
    out = dict(coef=np.full((nb, n), -7.0), lam=np.full((nb, 3, n), -7.0), cost=np.full(nb, -7.0), fun=np.full(nb, -7.0),
               iters=np.full(nb, -7, dtype=np.int32), flags=np.full(nb, -7, dtype=np.int32))
    h = dict(hc=np.zeros((nb, mi, n)), hl=np.zeros((nb, mi, 3, n)), hf=np.zeros((nb, mi)), hk=np.zeros((nb, mi))) if hist else {}
    _call(lib, 'bdrt_ridge_ex', C.byref(o), zd, fb, nb, ng, G, qbase, gsel, base, Ls, lo, lam0, lam0s, betas, x0,
          *([out[k] for k in ('coef', 'lam', 'cost', 'fun', 'iters', 'flags')] + [h.get(k) for k in ('hc', 'hl', 'hf', 'hk')]))
    for b in range(nb):                          # (the rows no iteration wrote)
        for k in h:
            h[k][b, out['iters'][b]:] = 0.0
    out.update(h)
    _check('ridge_' + case, out)


# ------------------------------------------------------------------------------------------------ the model object
def _points(seed, B, D):
    return np.ascontiguousarray(_uniform(seed, (B, D)) * 3.0)


def _logp(prob, th, spec, case, tag):
    lp, g = prob.logp_grad(th, jacobian=True, spec=spec)
    return {'%s_lp' % tag: lp, '%s_grad' % tag: g}


def test_problem_bits(lib):
    """One problem object through every regrowth of its buffers, a second one used after the first is gone."""
    from tests.test_gpu_hessian import _dat_problem
    name = 'dat_optimize_2ZARC_uniform_0.25_K81'
    first, d, _ = _dat_problem(name, True, n_spectra=2)
    second, _, _ = _dat_problem(name, True, n_spectra=2)
    D = first.D
    outs = {}
    outs.update(_logp(first, _points(141, 1, D), None, 'problem', 'B1'))
    outs.update(_logp(first, _points(142, 17, D), np.arange(17) % 2, 'problem', 'B17'))
    outs.update(_logp(first, _points(143, 65, D), None, 'problem', 'B65'))          # scratch regrows from its 64-row floor
    first.set_Z(np.vstack([d['Z'] * (1.0 + 0.1 * i) for i in range(5)]))           # d_Z regrows
    outs.update(_logp(first, _points(144, 3, D), np.array([0, 2, 4]), 'problem', 'B3_5spectra'))
    first.close()
    th = _points(145, 3, D)
    spec = np.array([1, 0, 1], dtype=np.int32)
    outs.update(_logp(second, th, spec, 'problem', 'second_B3'))
    par, Zh, sg = second.transformed(th, spec=spec)
    outs.update(tr_params=par, tr_Zhat=Zh, tr_sigma=sg)
    Zh1 = np.full((3, 2 * second.nf), -7.0)
    _call(lib, 'bdrt_transformed', second.handle, th, spec, 3, None, Zh1, None)
    outs['tr_Zhat_alone'] = Zh1
    y = np.ascontiguousarray(_points(146, 1, D)[0] * 0.5)
    H, Hl, held = np.full((D, D), -7.0), np.full((D, D), -7.0), np.full(D, -7.0)
    assert _call(lib, 'bdrt_debug_hessian', second.handle, y, 1, H) == 0
    assert _call(lib, 'bdrt_debug_hessian_lin', second.handle, y, 1, 1, Hl, held) == 0
    outs.update(H=H, H_lin=Hl, held=held)
    second.close()
    _check('problem', outs)


def test_optimize_bits(lib):
    from bayes_drt_amd.engine import optimize_batch
    from tests.test_gpu_hessian import _dat_problem
    prob, _, _ = _dat_problem('dat_optimize_2ZARC_uniform_0.25_K81', True, n_spectra=2)
    th0 = np.ascontiguousarray(_uniform(151, (3, prob.D)) * 4.0)
    outs = {}
    for tag, before in (('newton', 0), ('lbfgs20_newton', 20)):
        theta, rep = optimize_batch(prob, th0, spec=[0, 1, 0], lbfgs_before_newton=before)
        outs[tag + '_theta'] = theta
        for k in ('lp', 'grad_norm', 'grad_inf'):
            outs['%s_%s' % (tag, k)] = np.array([r[k] for r in rep], dtype=np.float64)
        for k in ('iterations', 'n_evals', 'return_code', 'newton_iterations'):
            outs['%s_%s' % (tag, k)] = np.array([r[k] for r in rep], dtype=np.int32)
    prob.close()
    _check('optimize', outs)


def test_streamed_problem_bits(lib):
    """the streamed evaluator's workspace: first use, then a batch that makes it grow"""
    from tests.test_gpu_big import _big_problem
    prob, _, _ = _big_problem(nf=150, K=221)
    assert prob.evaluator() == 5
    outs = {}
    outs.update(_logp(prob, _points(161, 2, prob.D), None, 'big', 'B2'))
    outs.update(_logp(prob, _points(162, 5, prob.D), None, 'big', 'B5'))
    prob.close()
    _check('big', outs)


# ------------------------------------------------------------------------------------------------ debug entries, matrices
def test_debug_entries_bits(lib):
    x8 = np.ascontiguousarray(_uniform(171, (64, 8)) * 16.0)
    s = np.full((2, 64), -7.0)
    fn = lib.bdrt_debug_sum_by_lane
    fn.argtypes = [C.c_void_p, C.c_void_p]; fn.restype = C.c_int
    assert fn(x8.ctypes.data, s.ctypes.data) == 0
    x = np.ascontiguousarray(_uniform(172, (5,)) * 8.0 + 4.5)
    m = np.full((3, 5), -7.0)
    fn = lib.bdrt_debug_lean_math
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p]; fn.restype = C.c_int
    assert fn(x.ctypes.data, 5, m.ctypes.data) == 0
    _check('debug', {'sum_by_lane': s, 'lean_math': m})


def test_build_matrices_bits(lib):
    nf, k = 5, 7
    freq = np.ascontiguousarray(10.0 ** (2.0 - 0.5 * np.arange(nf)))
    tau = np.ascontiguousarray(1.0 / (2.0 * np.pi * 10.0 ** (3.0 - 0.5 * np.arange(k))))
    eps = 1.0 / np.mean(np.diff(np.log(tau[::-1])))
    outs = {}
    for part in (0, 1):
        for toep in (0, 1):
            A = np.full((nf, k), -7.0)
            _call(lib, 'bdrt_build_A', freq, nf, tau, k, C.c_double(eps), 0, part, 1, 0, C.c_double(0.0), toep, A)
            outs['A_part%d_toep%d' % (part, toep)] = A
    L = np.full((k, k), -7.0)
    _call(lib, 'bdrt_build_L', tau, k, C.c_double(eps), np.array([1.0, 0.5, 0.25, 0.125]), L)
    Lr = np.full((nf, k), -7.0)
    _call(lib, 'bdrt_build_L_rect', freq, nf, tau, k, C.c_double(eps), np.array([1.0, 0.0, 0.0, 0.0]), 0, Lr)
    outs.update(L=L, L_rect=Lr)
    for toep in (0, 1):
        M = np.full((k, k), -7.0)
        _call(lib, 'bdrt_build_M', tau, k, C.c_double(eps), np.array([0.25, 0.5, 1.0]), toep, M)
        outs['M_toep%d' % toep] = M
    _check('build', outs)
