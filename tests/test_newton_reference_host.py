"""The checking code of tests/test_gpu_newton_solve.py, run on LAPACK's Cholesky factor (no GPU): for every input of the GPU test the
reference alone stays inside every bound of tests/newton_numpy.py -- factor, solve, predicted increase, g.s, s.s --, the damping
ladder commits the rung the planted eigenvalue asks for, accepted and refused rungs keep their eigenvalue margins, and every input
of the verdict is at least 1e-9 (relative) away from each of its thresholds and takes the branch it was made for.

The project's own Hessians come from the numpy statement here (tests/hessian_numpy.py on the oracle's matrices) and from
bdrt_debug_hessian_lin on the GPU: the same matrices to 1e-11 of their largest entry (tests/test_gpu_hessian.py)."""
import numpy as np
import pytest

from tests import hessian_shapes as hs
from tests import newton_cases as nc
from tests import newton_numpy as nn
from tests.test_oracle_hessian import shape_problem, statement


def check_reference(c, label, rung=None):
    """LAPACK's ladder, factor and solve on one input through every measure; returns the measures"""
    D = len(c['g']); Dp = nn.padded(D)
    R = nn.ladder(c['H'], c['g'], c['x'], c['lam'], c['lin'])
    assert R['ok'], label
    if rung is not None:
        assert R['rung'] == rung, (label, R['rung'])
    for lam in R['refused']:
        assert nn.rung_margin_ok(c['H'], lam, Dp, accepted=False), (label, lam)
    assert nn.rung_margin_ok(c['H'], R['lam'], Dp, accepted=True), label
    M = nn.damped(c['H'], R['lam'])
    ext = D <= nn.LD_MAX_D
    omega = nn.factor_omega(M, R['L'], extended=ext)
    assert omega <= nn.factor_bound_omega(Dp, ext), (label, omega)
    sr = nn.solve_ratio(M, R['L'], R['rhs'], R['s'])
    assert sr <= 1.0, (label, sr)
    # pred, gs, ss as a float64 implementation would form them
    s, b = R['s'], R['rhs']
    gs, ss = float(b @ s), float(s @ s)
    pc = nn.pred_check(c['H'], b, s, R['lam'], R['L'], Dp, 0.5 * (gs + R['lam'] * ss), gs, ss)
    for k, (err, bound) in pc.items():
        assert err <= bound, (label, k, err, bound)
    return dict(omega=omega, solve=sr, pred=pc, R=R)


@pytest.mark.parametrize('D', sorted(nc.SHAPES))
def test_lapack_stays_inside_the_bounds_at_every_shape_and_condition(D):
    for cond in nc.CONDS:
        m = check_reference(nc.spd_case(D, cond), 'D %d cond %.0e' % (D, cond), rung=0)
        print('D %4d cond %.0e: omega %.2f (bound %.0f), solve %.3f of its bound, pred %.1e of %.1e' % (
            D, cond, m['omega'], nn.factor_bound_omega(nn.padded(D), D <= nn.LD_MAX_D), m['solve'], *m['pred']['pred']))
        assert m['omega'] > 0 or D == 1


def test_the_sampled_rows_see_what_the_whole_factor_shows():
    """the parity measure of a wide factor is taken on tests/newton_numpy.py::sample_rows: on a factor small enough to evaluate in
    full, an error planted in the last trailing update is seen on the sample as on the whole"""
    c = nc.spd_case(130, 1e8)
    M = nn.damped(c['H'], c['lam'])
    L = nn.lapack_factor(M)
    rows = nn.sample_rows(len(M))
    full, part = nn.factor_omega(M, L), nn.factor_omega(M, L, rows=rows)
    assert 0 < part <= full
    Lbad = L.copy(); Lbad[-1, :] *= 1.0 + 2.0 ** -40          # 2^-39 of the last diagonal entry's sum: 2^14 u
    assert nn.factor_omega(M, Lbad, rows=rows) > 1000 and nn.factor_omega(M, Lbad) > 1000


def _hess(P, y, lin):
    out = statement(P, y, lin=bool(lin))
    return out[2], (out[3] if lin else np.zeros(len(y)))


def _grad(P, y):
    return statement(P, y)[1]


@pytest.mark.parametrize('point', sorted(nc.PROJECT_POINTS))
@pytest.mark.parametrize('name', nc.PROJECT_SHAPES)
@pytest.mark.parametrize('lin', (0, 1))
def test_lapack_stays_inside_the_bounds_on_the_projects_hessian(name, lin, point):
    nf, K, pos, irr = hs.SHAPES[name]
    P = shape_problem(nf, K, pos, irr)
    y, lam = nc.project_point(name, point)
    c = nc.project_case(P, y, lin, _hess, _grad, lam)
    m = check_reference(c, '%s %s lin %d' % (name, point, lin))
    M = nn.damped(c['H'], m['R']['lam'])
    d = np.abs(np.diag(M))
    print('%s %s lin %d: rung %d, diagonal of M over %.1e .. %.1e, omega %.2f, solve %.3f' % (name, point, lin, m['R']['rung'], d.min(), d.max(), m['omega'], m['solve']))
    if point == 'MAP':
        assert m['R']['rung'] == 0 and d.max() / d.min() >= 1e8       # the dynamic range the kernel really sees
    else:
        assert m['R']['rung'] >= 6                                    # beyond what six attempts side by side reach at once


@pytest.mark.parametrize('D,rung', nc.PLANTED)
def test_the_ladder_commits_the_rung_after_the_planted_eigenvalue(D, rung):
    c = nc.planted_case(D, rung)
    assert nc.least_rung_distance(c['mu']) >= 2.0
    m = check_reference(c, 'planted D %d' % D, rung=rung)
    assert m['R']['lam'] == nc.LAM0 * 4.0 ** rung == 2.0 * c['mu']


def test_no_damping_up_to_1e12_lifts_the_hopeless_eigenvalue():
    c = nc.planted_case(33, mu=nc.MU_HOPELESS)
    R = nn.ladder(c['H'], c['g'], c['x'], c['lam'])
    assert not R['ok'] and R['lam'] > 1e12 and R['lam'] == nc.LAM0 * 4.0 ** len(nc.rungs()) and len(R['refused']) == len(nc.rungs())


def test_the_linear_scale_case_crosses_the_floor_and_holds_coefficients():
    c = nc.lin_synthetic_case()
    m = check_reference(c, 'linear scale, synthetic', rung=0)
    s, lin = m['R']['s'], c['lin']
    held = lin['held'] != 0
    assert held.sum() == 2 and np.all(m['R']['rhs'][held] == 0) and np.all(c['g'][held] != 0)
    tp = nn.trial_points(c['x'], s, lin)
    k5, k6 = c['below']
    lf = np.log(lin['floor'])
    assert np.all(tp[:, k5] == lf) and tp[0, k6] == lf and tp[1, k6] == lf and tp[2, k6] > lf and tp[3, k6] > lf
    other = np.ones(len(s), dtype=bool); other[lin['o_x']:lin['o_x'] + lin['Kx']] = False
    for t in range(4):
        assert np.array_equal(tp[t, other], (c['x'] + 2.0 ** -t * s)[other])


_ACCEPT = nc.accept_cases()


@pytest.mark.parametrize('name', sorted(_ACCEPT))
def test_every_input_of_the_verdict_is_away_from_its_thresholds_and_takes_its_branch(name):
    c, exp = _ACCEPT[name]
    st, x, g, mg = nn.accept(c['st'], c['x'], c['g'], c['trial'], c['lp_t'], c['gt'], c['lin'])
    assert mg.least >= 1e-9, sorted(mg.log, key=lambda r: r[3])[:3]
    assert (st['lam'], st['iters'], st['rc'], st['done'], st['need_hess']) == (exp['lam'], exp['iters'], exp['rc'], exp['done'], exp['need_hess'])
    t = exp['taken']
    assert np.array_equal(x, c['x'] if t is None else c['trial'][t]) and np.array_equal(g, c['g'] if t is None else c['gt'][t], equal_nan=True)
    assert st['n_evals'] == c['st']['n_evals'] + 4
    # the state's pred is the shortcut's: the statement's form of the scaled prediction and the state's (gs, ss, lam) form agree
    for tt in range(1, 4):
        sc = 2.0 ** -tt
        assert abs(sc * c['st']['gs'] + sc * sc * (c['st']['pred'] - c['st']['gs']) - nc.pred_of(c['st'], tt)) <= 1e-15 * abs(c['st']['gs'])


def test_the_verdicts_cover_every_branch():
    taken = [e['taken'] for _, e in _ACCEPT.values()]
    assert set(taken) == {None, 0, 1, 2, 3}
    assert {(e['rc'], e['done']) for _, e in _ACCEPT.values()} == {(1, 0), (0, 1), (1, 1)}
