"""GPU tests (-m gpu) of the Newton iteration's damped Cholesky solve and of its verdict on the trial points (csrc/bdrt_newton.hip:
newton_build_kernel, newton_solve_kernel with chol_blocked / chol_blocked_solve, newton_gather_kernel, newton_accept_kernel), one
launch at a time on supplied data through bdrt_debug_newton_solve and bdrt_debug_newton_accept, against the plain statement and the
measures of tests/newton_numpy.py.  tests/test_newton_reference_host.py runs the same measures on LAPACK's factor without a GPU.

With u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Thms 10.3 and 10.4), each bound
twice the textbook's because the kernel multiplies by reciprocals and takes its square roots from an rsq estimate with two Newton steps:
  factor   |M - L L^T| <= 2 gamma_{Dp+1} |L||L^T| componentwise (np.longdouble up to D = 544, float64 + gamma_Dp above); padding = identity
  solve    |g - M s| <= 2 gamma_{3Dp+1} |L||L^T||s| componentwise, the residual in np.longdouble
  parity   omega = max componentwise ratio of the factor / u: the kernel's at most 4 x LAPACK's on the same matrix (above D = 544 both on
           the rows of newton_numpy.sample_rows, in np.longdouble)
  pred     |pred - (g.s + 1/2 s^T H s)| <= 1/2 |s|^T 2 gamma_{3Dp+1} |L||L^T||s| + gamma_Dp (|g|^T|s| + lam s^T s); gs, ss to gamma_Dp of their
           absolute sums
  ladder   an accepted rung has lam_min(M) >= -Dp gamma_{Dp+1} |M|_2, a refused one lam_min(M) <= +Dp gamma_{Dp+1} |M|_2; with a planted
           eigenvalue a factor 2 away from every rung the committed damping is the statement's
  natt     1, 2 and 6 attempts side by side: the same damping, and s, pred, gs, ss, the factor's lower block triangle and the four
           trial points bit for bit
  verdict  lam, iters, rc, done, need_hess and the committed x, g exactly the statement's, every input 1e-9 away from its thresholds
Each line of measurements is appended to the file BDRT_NEWTON_PARITY_OUT names, when set (profiles/newton_solve/parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

from bayes_drt_amd import _lib
from tests import hessian_shapes as hs
from tests import newton_cases as nc
from tests import newton_numpy as nn

pytestmark = pytest.mark.gpu


def _record(line):
    print(line)
    path = os.environ.get('BDRT_NEWTON_PARITY_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _lin_args(lin, D):
    if lin is None:
        return None, None, 0.0, 0, 0, []
    tz, held = _lib.f64(lin['tz']), _lib.f64(lin['held'])
    assert tz.shape == (D,) and held.shape == (D,)
    return _lib.ptr(tz), _lib.ptr(held), float(lin['floor']), int(lin['o_x']), int(lin['Kx']), [tz, held]


def hip_solve(c, natt=1, expect_rc=0):
    """one launch of the damped solve on the case's data: dict(L [Dp, Dp], s, trial [4, D], and the record's fields)"""
    lib = _lib.require_gpu()
    H, g, x = _lib.f64(c['H']), _lib.f64(c['g']), _lib.f64(c['x'])
    D = len(g); Dp = nn.padded(D)
    assert H.shape == (D, D) and x.shape == (D,)
    L = np.full((Dp, Dp), np.nan); s = np.full(D, np.nan); trial = np.full((4, D), np.nan)
    rec = _lib.NewtonSolveRecord()
    tz, held, floor, o_x, Kx, keep = _lin_args(c['lin'], D)
    rc = lib.bdrt_debug_newton_solve(_lib.ptr(H), _lib.ptr(g), _lib.ptr(x), D, float(c['lam']), int(natt), tz, held, floor, o_x, Kx,
                                     _lib.ptr(L), _lib.ptr(s), _lib.ptr(trial), C.byref(rec))
    assert rc == expect_rc, (rc, lib.bdrt_last_error())
    return dict(L=L, s=s, trial=trial, ok=rec.ok, attempt=rec.attempt, rc=rec.rc, done=rec.done, lam=rec.lam, pred=rec.pred, gs=rec.gs, ss=rec.ss)


def _rung_of(lam, lam0):
    j = int(round(np.log(lam / lam0) / np.log(4.0)))
    assert lam == lam0 * 4.0 ** j and j >= 0, (lam, lam0)          # (multiplications by 4 are exact)
    return j


def check_solve(c, out, label, rung=None):
    """every bound on one launch's results; returns the measures"""
    D = len(c['g']); Dp = nn.padded(D)
    assert out['ok'] == 1 and out['rc'] == 1 and out['done'] == 0, (label, out['ok'], out['rc'], out['done'])
    # the ladder
    j = _rung_of(out['lam'], c['lam'])
    R = nn.ladder(c['H'], c['g'], c['x'], c['lam'], c['lin'])
    for jj in range(j):
        assert nn.rung_margin_ok(c['H'], c['lam'] * 4.0 ** jj, Dp, accepted=False), (label, 'refused rung', jj)
    assert nn.rung_margin_ok(c['H'], out['lam'], Dp, accepted=True), (label, 'accepted rung', j)
    if rung is not None:
        assert j == rung == R['rung'] and out['lam'] == R['lam'], (label, j, rung, R['rung'])
    assert out['attempt'] <= j
    # the factor
    M = nn.damped(c['H'], out['lam'])
    Mp, Lp = nn.pad_identity(M, Dp), np.tril(out['L'])
    assert np.all(np.isfinite(Lp))
    assert np.array_equal(Lp[D:], np.eye(Dp)[D:]), label                       # padding rows (and with them the padding columns): identity
    ext = D <= nn.LD_MAX_D
    omega = nn.factor_omega(Mp, Lp, extended=ext)
    Lref = nn.lapack_factor(M)
    assert Lref is not None, label
    if ext:
        omega_k, omega_ref = omega, nn.factor_omega(M, Lref)
    else:
        rows = nn.sample_rows(Dp)
        omega_k, omega_ref = nn.factor_omega(Mp, Lp, rows=rows), nn.factor_omega(M, Lref, rows=rows[rows < D])
    # the solve and the predicted increase
    b = nn.rhs(c['g'], c['lin'])
    bp, sp = np.zeros(Dp), np.zeros(Dp)
    bp[:D], sp[:D] = b, out['s']
    sr = nn.solve_ratio(Mp, Lp, bp, sp)
    pc = nn.pred_check(c['H'], b, out['s'], out['lam'], Lp[:D, :D], Dp, out['pred'], out['gs'], out['ss'])
    ratio = omega_k / omega_ref if omega_ref > 0 else (0.0 if omega_k == 0 else np.inf)
    _record('%-34s D %4d Dp %4d rung %2d | omega kernel %7.2f lapack %6.2f ratio %5.2f (bound %6.0f%s) | solve %.4f of its bound | '
            'pred %.2e of %.2e, gs %.2e of %.2e, ss %.2e of %.2e' % (label, D, Dp, j, omega_k, omega_ref, ratio, nn.factor_bound_omega(Dp, ext),
                                                                     '' if ext else ', float64: %.2f' % omega, sr, *pc['pred'], *pc['gs'], *pc['ss']))
    assert omega <= nn.factor_bound_omega(Dp, ext), (label, omega)
    assert omega_k <= 4.0 * omega_ref, (label, omega_k, omega_ref)
    assert sr <= 1.0, (label, sr)
    for k, (err, bound) in pc.items():
        assert err <= bound, (label, k, err, bound)
    # the trial points, from the kernel's own step
    tp = nn.trial_points(c['x'], out['s'], c['lin'])
    exact = np.ones(D, dtype=bool)
    if c['lin'] is not None:
        exact[c['lin']['o_x']:c['lin']['o_x'] + c['lin']['Kx']] = False
    assert np.array_equal(out['trial'][:, exact], tp[:, exact]), label
    if not np.all(exact):
        err = np.abs(out['trial'][:, ~exact] - tp[:, ~exact]) / np.spacing(np.abs(tp[:, ~exact]))
        assert np.max(err) <= 4.0, (label, np.max(err))                        # device exp and log
    return dict(omega=omega_k, omega_ref=omega_ref, solve=sr, pred=pc, rung=j)


@pytest.mark.parametrize('cond', nc.CONDS)
@pytest.mark.parametrize('D', sorted(nc.SHAPES))
def test_factor_solve_and_prediction_stay_inside_their_bounds(D, cond):
    """SPD with the spectrum [1 / cond, 1] at every size where chol_blocked's schedule changes (tests/newton_cases.py::SHAPES)"""
    c = nc.spd_case(D, cond)
    check_solve(c, hip_solve(c), 'spectrum 1 .. %.0e' % (1.0 / cond), rung=0)


def test_one_past_the_lds_limit_is_refused_without_a_launch():
    D = nc.D_TOO_WIDE
    c = dict(H=-np.eye(D), g=np.ones(D), x=np.zeros(D), lam=1e-3, lin=None)
    out = hip_solve(c, expect_rc=-2)
    assert np.all(np.isnan(out['s'])) and np.all(np.isnan(out['L'])) and b'LDS' in _lib.load_library().bdrt_last_error()


def _gpu_problem(name):
    from tests.test_gpu_hessian import _shape
    return _shape(*hs.SHAPES[name])


@pytest.mark.parametrize('point', sorted(nc.PROJECT_POINTS))
@pytest.mark.parametrize('lin', (0, 1))
@pytest.mark.parametrize('name', nc.PROJECT_SHAPES)
def test_the_projects_own_hessian_through_the_ladder(name, lin, point):
    """-H + lam I from bdrt_debug_hessian_lin, both scales.  At the near-MAP point H is indefinite, the ladder climbs ten rungs and
    more from 1e-3 (six attempts side by side, the last one going on by itself), and the committed rung is the statement's; at the
    MAP the first rung factors a matrix whose diagonal spans twelve orders of magnitude."""
    from tests.test_gpu_hessian import _hip_hessian_lin
    prob, P = _gpu_problem(name)

    def hessian(P_, y, lin_):
        rc, H, held = _hip_hessian_lin(prob, y, lin_)
        assert rc == 0
        return H, held

    def gradient(P_, y):
        return np.ascontiguousarray(prob.logp_grad(y[None, :], jacobian=False)[1][0])

    y, lam = nc.project_point(name, point)
    c = nc.project_case(P, y, lin, hessian, gradient, lam)
    prob.close()
    label = '%s %s lin %d' % (name, point, lin)
    R = nn.ladder(c['H'], c['g'], c['x'], c['lam'], c['lin'])
    outs = [hip_solve(c, natt) for natt in (1, 6)]
    check_solve(c, outs[0], label, rung=R['rung'])
    _assert_same_bits(outs, label)
    if point == 'MAP':
        d = np.abs(np.diag(nn.damped(c['H'], outs[0]['lam'])))
        assert R['rung'] == 0 and d.max() / d.min() >= 1e8
    elif lin:
        held = c['lin']['held'] != 0
        assert held.any() and np.all(outs[0]['s'][held] == 0.0)       # (a held coefficient's row of H is -1 on the diagonal, its right-hand side zero)


def test_the_linear_scale_holds_coefficients_and_projects_steps_onto_the_floor():
    c = nc.lin_synthetic_case()
    out = hip_solve(c)
    check_solve(c, out, 'linear scale, synthetic', rung=0)
    k5, k6 = c['below']
    lf = np.log(c['lin']['floor'])
    # (the projected points: log of the floor itself, to the device's log)
    assert np.all(np.abs(out['trial'][:, k5] - lf) <= 4 * np.spacing(abs(lf))) and np.all(np.abs(out['trial'][:2, k6] - lf) <= 4 * np.spacing(abs(lf)))
    assert np.all(out['trial'][2:, k6] > lf + 0.1)
    # the right-hand side is zero where held: with the gradient's entries there kept, g.s would be another number altogether
    held = c['lin']['held'] != 0
    b_wrong = c['g'] * c['lin']['tz']
    assert abs(b_wrong @ out['s'] - out['gs']) > 1e3 * nn.gamma(48) * (np.abs(b_wrong) @ np.abs(out['s'])) and np.all(b_wrong[held] != 0)


def _block_lower(L):
    n = len(L)
    blk = np.arange(n) // 16
    return np.where(blk[None, :] <= blk[:, None], L, 0.0)


def _assert_same_bits(outs, label):
    a = outs[0]
    for o in outs[1:]:
        assert o['lam'] == a['lam'] and o['ok'] == a['ok'], label
        for k in ('pred', 'gs', 'ss'):
            assert np.float64(o[k]).tobytes() == np.float64(a[k]).tobytes(), (label, k)
        assert np.array_equal(o['s'], a['s']) and np.array_equal(o['trial'], a['trial']), label
        assert np.array_equal(_block_lower(o['L']), _block_lower(a['L'])), label


@pytest.mark.parametrize('D,rung', nc.PLANTED)
def test_speculative_attempts_commit_the_same_damping_and_the_same_numbers(D, rung):
    """attempts side by side give "the same sequence of dampings and the same numbers as the one-workgroup loop".  The
    largest eigenvalue of H is planted a factor 2 from the nearest rungs, so the rung is not a matter of rounding."""
    c = nc.planted_case(D, rung)
    assert nc.least_rung_distance(c['mu']) >= 2.0
    outs = [hip_solve(c, natt) for natt in nc.NATTS]
    for natt, o in zip(nc.NATTS, outs):
        assert o['attempt'] == min(rung, natt - 1), (natt, o['attempt'])
    check_solve(c, outs[0], 'planted mu %.3g' % c['mu'], rung=rung)
    assert outs[0]['lam'] == 2.0 * c['mu']
    _assert_same_bits(outs, 'planted D %d' % D)


def test_damping_exhausted_returns_normally():
    """mu = 1e13: no rung up to 1e12 factors -- ok 0, rc 2 (done), the damping beyond 1e12, whatever the number of attempts"""
    c = nc.planted_case(33, mu=nc.MU_HOPELESS)
    R = nn.ladder(c['H'], c['g'], c['x'], c['lam'])
    assert not R['ok']
    for natt in nc.NATTS:
        o = hip_solve(c, natt)
        assert (o['ok'], o['rc'], o['done']) == (0, 2, 1) and o['lam'] > 1e12 and o['lam'] == R['lam'], (natt, o['ok'], o['rc'], o['done'], o['lam'])
        assert o['attempt'] == natt - 1


# ---- the verdict ------------------------------------------------------------------------------------------------------------

_ACCEPT = nc.accept_cases()
_STATE_FIELDS = ('lp', 'lam', 'pred', 'gs', 'ss', 'grad_inf', 'tol', 'lp_trial', 'iters', 'max_iter', 'lin', 'rc', 'done', 'need_hess', 'n_evals')


def hip_accept(c):
    lib = _lib.require_gpu()
    st = _lib.NewtonState()
    for k in _STATE_FIELDS:
        setattr(st, k, c['st'][k])
    D = len(c['x'])
    x, g = _lib.f64(c['x']).copy(), _lib.f64(c['g']).copy()
    trial, lp_t, gt = _lib.f64(c['trial']), _lib.f64(c['lp_t']), _lib.f64(c['gt'])
    assert trial.shape == (4, D) and gt.shape == (4, D) and lp_t.shape == (4,)
    tz, held, floor, o_x, Kx, keep = _lin_args(c['lin'], D)
    rc = lib.bdrt_debug_newton_accept(C.byref(st), _lib.ptr(x), _lib.ptr(g), D, _lib.ptr(trial), _lib.ptr(lp_t), _lib.ptr(gt), tz, held, floor, o_x, Kx)
    assert rc == 0, lib.bdrt_last_error()
    return {k: getattr(st, k) for k in _STATE_FIELDS}, x, g


@pytest.mark.parametrize('name', sorted(_ACCEPT))
def test_the_verdict_is_the_statements(name):
    c, exp = _ACCEPT[name]
    ref, xr, gr, mg = nn.accept(c['st'], c['x'], c['g'], c['trial'], c['lp_t'], c['gt'], c['lin'])
    assert mg.least >= 1e-9, sorted(mg.log, key=lambda r: r[3])[:3]
    st, x, g = hip_accept(c)
    got = tuple(st[k] for k in ('lam', 'iters', 'rc', 'done', 'need_hess'))
    print('%s: lam %r iters %d rc %d done %d need_hess %d (statement: lam %r)' % ((name,) + got + (ref['lam'],)))
    assert got == tuple(ref[k] for k in ('lam', 'iters', 'rc', 'done', 'need_hess')) == tuple(exp[k] for k in ('lam', 'iters', 'rc', 'done', 'need_hess'))
    assert np.array_equal(x, xr, equal_nan=True) and np.array_equal(g, gr, equal_nan=True)
    assert st['lp'] == ref['lp'] and st['n_evals'] == ref['n_evals']
    assert st['lp_trial'] == ref['lp_trial'] or (np.isnan(st['lp_trial']) and np.isnan(ref['lp_trial']))
