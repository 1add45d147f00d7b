"""GPU tests (-m gpu) of the closed-form Hessian behind the MAP's Newton iteration (csrc/bdrt_newton_hess.h; StanModel.optimizing,
reference bayes_drt/inversion.py:1216; density stan_model_files/Series_pos_modelcode.txt:24-69): the HIP kernels against the numpy
statement of the same formulas (itself held to central differences of the oracle's gradient by tests/test_oracle_hessian.py) and
against central differences of the HIP gradient; the Newton iteration on it against the finite-difference iteration of rounds 1-5.

The comparison with the numpy statement is tests/hessian_numpy.py::hessian_mismatch: every block of index classes against its own
largest entry, the dense product A^T C A column by column and entry by entry, the diagonal entry by entry, on the log scale and on the
linear scale of the coefficients (with the mask of the coefficients held at their floor).  The tolerances in force, and the
measurement of the reference's own rounding error they rest on, are in the docstring of tests/test_oracle_hessian.py.

Shapes (tests/hessian_shapes.py): the golden problems (K = 81 .. 161: NH <= 192, NG >= 2) and the regimes of hess_fill's column and
frequency ownership they do not reach -- nf < NG, nf not divisible by NG, NH = 256 with NG = 2, the same from plain copies of A.
The largest K with a closed form is 192 (K_ADMITTED, found at nf = 33 by test_..._ownership[nf33_Kmax]): beyond it L leaves the band
path and the debug entry returns 1, so D <= 393 / Dp <= 400 and the one-group regimes NH = 320 .. 512 are not reachable today."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import hessian_shapes as hs
from tests.helpers import load, rel_l2
from tests.hessian_numpy import hessian_mismatch, series_hessian
from tests.test_oracle_hessian import failures, held_margin

pytestmark = pytest.mark.gpu

K_ADMITTED = 192        # the largest K with a closed form (found at nf = 33; beyond it the debug entry returns 1)


def _dat_problem(name, pos=True, n_spectra=1):
    from bayes_drt_amd.model import Problem
    d = load(name)
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=pos)
    kw = dict(sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']), ups_beta=float(d['ups_beta']), induc_scale=float(d['induc_scale']))
    Z = d['Z'] if n_spectra == 1 else np.vstack([d['Z'] * (1.0 + 0.1 * i) for i in range(n_spectra)])
    return Problem([blk], Z, d['freq'], **kw), d, kw


def _hip_hessian(prob, y, spec=0):
    H = np.empty((prob.D, prob.D))
    rc = prob._lib.bdrt_debug_hessian(C.c_void_p(prob.handle), y.ctypes.data_as(C.c_void_p), int(spec), H.ctypes.data_as(C.c_void_p))
    return rc, H


def _hip_hessian_lin(prob, y, lin, spec=0):
    H = np.empty((prob.D, prob.D)); held = np.full(prob.D, np.nan)
    rc = prob._lib.bdrt_debug_hessian_lin(C.c_void_p(prob.handle), y.ctypes.data_as(C.c_void_p), int(spec), int(lin), H.ctypes.data_as(C.c_void_p),
                                          held.ctypes.data_as(C.c_void_p))
    return rc, H, held


def _assert_equals_the_statement(prob, y, P, lin, spec=0, label=''):
    """one debug call against one numpy evaluation: every check of hessian_mismatch within its tolerance, the held mask exactly.
    P: the arguments of the statement (tests/test_oracle_hessian.py::statement)."""
    rc, H, held = _hip_hessian_lin(prob, y, lin, spec)
    assert rc == 0
    out = series_hessian(y, P['A'], P['L'], P['Z'], P['w'], pos=P['pos'], lin=bool(lin), parts=True, **P['kw'])
    Href = out[2]
    mm = hessian_mismatch(H, Href, P['K'], parts=out[-2:])
    print('%s lin %d: %s' % (label, lin, ', '.join('%s %.1e' % kv for kv in sorted(mm.items(), key=lambda kv: -kv[1])[:5])))
    assert not failures(mm, P['nf']), (label, lin, failures(mm, P['nf']))
    assert np.array_equal(held != 0, out[3] if lin else np.zeros(prob.D, dtype=bool))
    sc = np.max(np.abs(Href))                          # the whole matrix relative to its largest entry, as before
    assert np.max(np.abs(H - Href)) <= 1e-11 * sc, np.max(np.abs(H - Href)) / sc
    assert np.max(np.abs(H - H.T)) <= 1e-12 * sc
    return H, Href


@pytest.mark.parametrize('name,pos', [('dat_optimize_2ZARC_uniform_0.25_K81', True), ('dat_optimize_2ZARC_uniform_0.25_K161', True),
                                      ('dat_optimize_2ZARC_uniform_0.25_K101', False), ('dat_sample_2ZARC_uniform_0.25_K161', True)])
def test_hip_hessian_equals_the_numpy_statement(name, pos):
    """Every entry of the D x D matrix, relative to its largest entry: <= 1e-11 (both sum the same terms in another order); and
    block by block, column by column of the dense product and entry by entry of the diagonal (hessian_mismatch), on the log scale
    and, for nonnegative coefficients, on the linear scale."""
    prob, d, kw = _dat_problem(name, pos, n_spectra=3)
    rs = np.random.RandomState(5)
    for spec in (0, 2):
        y = np.ascontiguousarray(rs.uniform(-1.5, 1.5, prob.D))
        rc, H = _hip_hessian(prob, y, spec)
        assert rc == 0
        Z = d['Z'] * (1.0 + 0.1 * spec)
        kw2 = {k: v for k, v in kw.items() if k != 'induc_scale'}
        _, _, Href = series_hessian(y, d['A'], (d['L0'], d['L1'], d['L2']), Z, 2 * np.pi * d['freq'], pos=pos, induc_scale=kw['induc_scale'], **kw2)
        sc = np.max(np.abs(Href))
        low = np.tril(np.ones_like(H, dtype=bool))          # (the factorisation reads the lower triangle)
        assert np.max(np.abs(H - Href)[low]) <= 1e-11 * sc, np.max(np.abs(H - Href)) / sc
        assert np.max(np.abs(H - H.T)) <= 1e-12 * sc
        P = dict(A=d['A'], L=(d['L0'], d['L1'], d['L2']), Z=Z, w=2 * np.pi * d['freq'], pos=pos, K=prob.Ks[0], nf=len(d['freq']), kw=kw)
        for lin in ((0, 1) if pos else (0,)):
            Hl, _ = _assert_equals_the_statement(prob, y, P, lin, spec, '%s spec %d' % (name, spec))
            if not lin:
                assert np.array_equal(Hl, H)                # the wrapper is the lin = 0 entry
    if not pos:                                             # the linear scale is for <lower=0> coefficients
        assert _hip_hessian_lin(prob, y, 1)[0] == 1
    prob.close()


def _gm_A(f, part, tau, eps):
    from bayes_drt_amd import matrices as gm
    return gm.construct_A(f, part, tau=tau, epsilon=eps)


def _gm_L(bf, tau, eps, order):
    from bayes_drt_amd import matrices as gm
    return gm.construct_L(bf, tau=tau, epsilon=eps, order=order)


_shapes = {}


def _shape(nf, K, pos, irregular):
    """(Problem, arguments of the statement) of a synthetic shape; the matrices built once per session by the product's constructors"""
    from bayes_drt_amd.model import Problem
    key = (nf, K, pos, irregular)
    if key not in _shapes:
        A, L, Z, f = hs.make_shape(nf, K, irregular, _gm_A, _gm_L)
        _shapes[key] = dict(A=A, L=L, Z=Z, w=2 * np.pi * f, f=f, pos=pos, K=K, nf=nf, kw=dict(hs.KW))
    P = _shapes[key]
    return Problem([dict(A=P['A'], L0=P['L'][0], L1=P['L'][1], L2=P['L'][2], nonneg=pos)], P['Z'], P['f'], **hs.KW), P


def _has_closed_form(nf, K):
    """whether the library builds the closed-form Hessian of the nf x K synthetic problem (not streamed: evaluator != 5, and rc == 0)"""
    prob, P = _shape(nf, K, True, False)
    ok = prob.evaluator() != 5 and _hip_hessian(prob, hs.random_point(prob.D))[0] == 0
    streamed = prob.evaluator() == 5
    prob.close()
    return ok, streamed


def _largest_admitted_K(nf=33, K_hi=352, K_lo=35):
    """The largest K with a closed form at nf frequencies, between K_lo (admitted) and K_hi (not admitted).  Every condition of
    admission is an upper bound on K (the band path's K <= 192, LDS sizes that grow with K), so bisection finds the step; the test
    then confirms K is admitted and K + 1 is not."""
    assert _has_closed_form(nf, K_lo)[0] and not _has_closed_form(nf, K_hi)[0]
    lo, hi = K_lo, K_hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _has_closed_form(nf, mid)[0]:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize('key', list(hs.SHAPES) + ['nf33_Kmax'])
def test_hip_hessian_in_every_regime_of_column_and_frequency_ownership(key):
    """Per shape: the random point and the near-MAP point (coefficients at the floor, some of them held), on the log scale and on
    the linear scale: four debug calls (two where the coefficients are free), each against one numpy evaluation."""
    if key == 'nf33_Kmax':
        # asked for as the NH = 384 regime, K stepped down from 352 until the problem is not streamed (evaluator != 5).  Not being
        # streamed is not enough: between K_ADMITTED and the first streamed K the problem has no closed form either (rc == 1: L is
        # not on the band path), so the helper looks for the closed form itself.  K_ADMITTED = 192 is NH = 256 again.
        K = _largest_admitted_K()
        print('largest K with a closed form at nf = 33:', K, '; streamed at 352:', _has_closed_form(33, 352)[1])
        assert K == K_ADMITTED and not _has_closed_form(33, K + 1)[0]
        nf, pos, irr = 33, True, False
    else:
        nf, K, pos, irr = hs.SHAPES[key]
    prob, P = _shape(nf, K, pos, irr)
    assert prob.evaluator() != 5 and prob.D == 2 * K + 9
    assert _hip_hessian(prob, hs.random_point(prob.D))[0] == 0
    for pname, y in (('random', hs.random_point(prob.D)), ('near-MAP', hs.near_map_point(K, pos))):
        if pos and pname == 'near-MAP':
            at_floor, held, margin = held_margin(P, y)       # (of the reference alone: no sign on a knife edge)
            assert at_floor.any() and margin >= 1e-6, margin
        for lin in ((0, 1) if pos else (0,)):
            _assert_equals_the_statement(prob, y, P, lin, 0, '%s %s' % (key, pname))
    prob.close()


def test_hip_hessian_on_a_general_frequency_grid_equals_central_differences_of_the_hip_gradient():
    """A measured spectrum on its own irregular frequency list: A is a general matrix (plain copies instead of Toeplitz generators).
    Against the numpy statement as well."""
    from bayes_drt_amd import matrices as gm
    from bayes_drt_amd.model import Problem
    rs = np.random.RandomState(3)
    nf, K = 37, 61
    f = np.sort(10 ** rs.uniform(-1.5, 5, nf))[::-1].copy()
    bf = np.logspace(6, -2.5, K)
    tau = 1 / (2 * np.pi * bf); eps = 1 / np.mean(np.diff(np.log(tau)))
    A = np.vstack([gm.construct_A(f, 'real', tau=tau, epsilon=eps), gm.construct_A(f, 'imag', tau=tau, epsilon=eps)])
    L = [gm.construct_L(bf, tau=tau, epsilon=eps, order=o) for o in (0, 1, 2)]
    w = 2 * np.pi * f
    z = 1.0 + 1.2 / (1 + (1j * w * 3e-3) ** 0.8) + 0.003 * (rs.normal(size=nf) + 1j * rs.normal(size=nf))
    z = z / (np.std(np.abs(z)) / np.sqrt(nf / 81))
    blk = dict(A=A, L0=0.36 * L[0], L1=0.24 * L[1], L2=0.12 * L[2], nonneg=True)
    prob = Problem([blk], np.concatenate([z.real, z.imag]), f, sigma_min=0.002, ups_alpha=0.05, ups_beta=0.1)
    y = np.ascontiguousarray(rs.uniform(-1, 1, prob.D))
    rc, H = _hip_hessian(prob, y)
    assert rc == 0
    Hfd = np.zeros_like(H)
    for j in range(prob.D):
        h = 1e-6 * max(1.0, abs(y[j]))
        P_ = np.vstack([y, y]); P_[0, j] += h; P_[1, j] -= h
        _, g = prob.logp_grad(P_, jacobian=False)
        Hfd[j] = (g[0] - g[1]) / (2 * h)
    Hfd = 0.5 * (Hfd + Hfd.T)
    assert np.max(np.abs(H - Hfd)) <= 1e-7 * np.max(np.abs(Hfd))
    P = dict(A=A, L=(blk['L0'], blk['L1'], blk['L2']), Z=np.concatenate([z.real, z.imag]), w=w, pos=True, K=K, nf=nf,
             kw=dict(sigma_min=0.002, ups_alpha=0.05, ups_beta=0.1))
    assert A[1, 1] != A[0, 0]                               # (not Toeplitz: the plain-copy path)
    for lin in (0, 1):
        _assert_equals_the_statement(prob, y, P, lin, 0, 'general grid 37 x 61')
    prob.close()


def test_models_without_a_closed_form_say_so():
    from tests.test_gpu_engine import _small_problem
    from bayes_drt_amd.model import Problem
    blk, Z, f, kw = _small_problem()                      # 12 x 9: L is not banded at this size
    prob = Problem([blk], Z, f, **kw)
    rc, _ = _hip_hessian(prob, np.zeros(prob.D))
    assert rc == 1
    prob.close()


@pytest.mark.parametrize('tag', ['K81', 'K161'])
def test_newton_iteration_on_the_closed_form_hessian(tag, monkeypatch):
    """The same stationary point as the finite-difference iteration (gamma to 1e-6), with a handful of evaluations per round
    instead of 2 D + 4: VERDICT r05's bound of 2000 gradient evaluations per K = 161 fit."""
    from bayes_drt_amd.engine import optimize_batch
    prob, d, kw = _dat_problem('dat_optimize_2ZARC_uniform_0.25_%s' % tag)
    th0 = np.random.RandomState(1234).uniform(-2, 2, (1, prob.D))
    t0 = time.time(); out, rep = optimize_batch(prob, th0); t_an = time.time() - t0
    monkeypatch.setenv('BDRT_NEWTON_FD', '1')
    t0 = time.time(); out_fd, rep_fd = optimize_batch(prob, th0); t_fd = time.time() - t0
    K = prob.Ks[0]
    print('%s: closed form %d Newton rounds, %d evaluations, %.1f ms; finite differences %d rounds, %d evaluations, %.1f ms; lp %.6f / %.6f'
          % (tag, rep[0]['newton_iterations'], rep[0]['n_evals'], 1e3 * t_an, rep_fd[0]['newton_iterations'], rep_fd[0]['n_evals'], 1e3 * t_fd,
             rep[0]['lp'], rep_fd[0]['lp']))
    assert rep[0]['return_code'] == 0 and rep[0]['grad_inf'] < 1e-8
    assert rep[0]['n_evals'] <= 2000 and rep_fd[0]['n_evals'] > 20000
    assert abs(rep[0]['lp'] - rep_fd[0]['lp']) <= 1e-8 * abs(rep_fd[0]['lp'])
    assert rel_l2(np.exp(out[0][2:2 + K]), np.exp(out_fd[0][2:2 + K])) < 1e-6
    prob.close()


def test_newton_iteration_at_the_wide_shape_on_both_scales(monkeypatch):
    """40 x 192 (D = 393, the widest admitted problem; asked for at 40 x 260, which has no closed form): the iteration on the default
    scale (linear once the damping has dropped) and on the log scale throughout reach the same stationary point."""
    from bayes_drt_amd.engine import optimize_batch
    nf, K, pos, irr = hs.SHAPES[hs.WIDE]
    prob, P = _shape(nf, K, pos, irr)
    th0 = np.random.RandomState(1234).uniform(-2, 2, (1, prob.D))
    out, rep = optimize_batch(prob, th0)
    monkeypatch.setenv('BDRT_NEWTON_LINEAR', '0')
    out_log, rep_log = optimize_batch(prob, th0)
    print('40 x 192: linear scale %d Newton rounds, lp %.9f, |g| %.2e; log scale %d rounds, lp %.9f, |g| %.2e'
          % (rep[0]['newton_iterations'], rep[0]['lp'], rep[0]['grad_inf'], rep_log[0]['newton_iterations'], rep_log[0]['lp'], rep_log[0]['grad_inf']))
    for r in (rep[0], rep_log[0]):
        assert r['return_code'] == 0 and r['grad_inf'] < 1e-8
    assert abs(rep[0]['lp'] - rep_log[0]['lp']) <= 1e-8 * abs(rep_log[0]['lp'])
    prob.close()
