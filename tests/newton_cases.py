"""Inputs of the tests of the Newton iteration's damped solve and verdict (tests/test_newton_reference_host.py on the CPU with
LAPACK's factor, tests/test_gpu_newton_solve.py on the GPU with csrc/bdrt_newton.hip's): the sizes at which chol_blocked changes its
schedule, matrices with a prescribed spectrum, planted indefinite directions for the damping ladder, and one input per branch of
the verdict.  Test infrastructure, not the product."""
import functools

import numpy as np

from tests import hessian_shapes as hs

# D: what changes there (Dp = D rounded up to 16; 512 threads, 16-row blocks, 28 trailing tiles per trip of the seven updating waves)
SHAPES = {
    1: 'one block, 15 rows of padding', 15: 'one block, 1 row of padding', 16: 'one block, no padding', 17: 'two blocks, 15 rows of padding',
    33: 'three blocks', 113: "the panel's four-pass load loop at m = 96 .. 112", 130: 'more than 28 trailing tiles: a second trip',
    331: 'the headline size', 400: 'the largest banded size', 530: 'panel rows and backward columns take a second pass of 512 threads',
    818: 'the wide model', 1104: 'the LDS limit',
}
D_TOO_WIDE = 1105          # Dp = 1120: more LDS than a workgroup can have
CONDS = (1e2, 1e8, 1e14)
LAM0 = 1e-3                # the iteration's first damping


@functools.lru_cache(maxsize=2)
def _orthogonal(D, seed=11):
    q, r = np.linalg.qr(np.random.RandomState(seed + D).normal(size=(D, D)))
    return q * np.sign(np.diag(r))


def _sym(Q, d):
    A = (Q * d) @ Q.T
    return 0.5 * (A + A.T)


def spd_case(D, cond):
    """H, g, x, lam with M = -H + lam I of spectrum [1 / cond, 1], log-spaced; lam is half of the smallest eigenvalue.
    D = 1 is M = 1 at every condition: the case is there for its 15 rows of padding, and a ratio of two one-entry residuals, each
    zero or one rounding, would say nothing (the square root's accuracy shows from D = 15 on)."""
    rs = np.random.RandomState(1000 + D)
    d = np.logspace(-np.log10(cond), 0.0, D) if D > 1 else np.array([1.0])
    lam = 0.5 * d[0]
    H = -_sym(_orthogonal(D), d - lam)
    return dict(H=H, g=rs.normal(size=D), x=rs.uniform(-1, 1, D), lam=lam, lin=None)


def rungs(lam0=LAM0):
    out, lam = [], lam0
    while lam <= 1e12:
        out.append(lam); lam *= 4.0
    return out


# (D, the rung that has to be committed): one rung up, three up (inside a six-attempt launch), seven up (beyond attempt 5: the last
# attempt goes on by itself)
PLANTED = [(17, 1), (130, 3), (331, 7)]
NATTS = (1, 2, 6)


def planted_case(D, rung=None, mu=None):
    """indefinite H: eigenvalues -[1e-6, 1] and one planted largest eigenvalue mu = twice the damping of rung - 1, so that -H + lam I is
    positive definite from rung `rung` on and no rung is within a factor 2 of mu"""
    rs = np.random.RandomState(2000 + D)
    mu = 2.0 * LAM0 * 4.0 ** (rung - 1) if mu is None else mu
    h = -np.logspace(-6, 0, D)
    h[0] = mu
    return dict(H=_sym(_orthogonal(D), h), g=rs.normal(size=D), x=rs.uniform(-1, 1, D), lam=LAM0, lin=None, mu=mu)


def least_rung_distance(mu):
    return min(max(mu / r, r / mu) for r in rungs())


MU_HOPELESS = 1e13         # no damping up to 1e12 makes -H + lam I positive definite


def lin_synthetic_case(D=33, o_x=2, Kx=20):
    """the linear scale on made-up data: held coefficients, and a step that takes coefficients below the floor at t = 0 (some of them at
    every length, some at the longer ones only)"""
    rs = np.random.RandomState(77)
    Q = _orthogonal(D)
    lam = 1e-3
    H = -_sym(Q, np.logspace(-3, 0, D))
    x = rs.uniform(-1, 1, D)
    k = np.arange(o_x, o_x + Kx)
    x[k] = np.log(10.0 ** rs.uniform(-6, 0, Kx))
    x[k[0]] = 0.0                                           # the largest coefficient, 1: the floor is 1e-14
    floor = 1e-14
    x[k[3]] = x[k[4]] = np.log(1.5 * floor)                 # at the floor
    held = np.zeros(D); held[k[3]] = 1.0; held[k[7]] = 1.0
    tz = np.ones(D); tz[k] = np.exp(-x[k])
    # a wanted step: coefficient 5 far below zero (below the floor at every length), coefficient 6 below the floor at t = 0 and 1 only
    s = rs.normal(size=D) * 0.1
    s[k] = rs.normal(size=Kx) * 0.1 * np.exp(x[k])
    s[k[5]] = -40.0 * np.exp(x[k[5]])
    s[k[6]] = -3.0 * np.exp(x[k[6]])
    M = -H + lam * np.eye(D)
    gz = M @ s
    # (the held coefficients' right-hand side is dropped: the two entries at `below` are set so that the step there stays the wanted one)
    idx = [k[5], k[6]]
    Minv = np.linalg.inv(M)
    gz[idx] += np.linalg.solve(Minv[np.ix_(idx, idx)], s[idx] - (Minv @ np.where(held != 0, 0.0, gz))[idx])
    g = gz / tz
    return dict(H=H, g=g, x=x, lam=lam, lin=dict(tz=tz, held=held, floor=floor, o_x=o_x, Kx=Kx), wanted=s, below=(k[5], k[6]))


PROJECT_SHAPES = ('nf7_K35', 'nf33_K90')     # the two smallest problems of tests/hessian_shapes.py


def project_case(P, y, lin, hessian, gradient, lam=LAM0):
    """-H + lam I from the project's own Hessian at the point y of problem P.  hessian(P, y, lin) -> (H, held [D]) and
    gradient(P, y) -> g_y are the caller's: the debug entry on the GPU, the numpy statement on the CPU."""
    K = P['K']
    H, held = hessian(P, y, lin)
    g = gradient(P, y)
    spec = None
    if lin:
        xk = np.exp(y[2:2 + K])
        tz = np.ones(len(y)); tz[2:2 + K] = 1.0 / xk
        spec = dict(tz=tz, held=np.asarray(held, dtype=float), floor=1e-14 * float(np.max(xk)), o_x=2, Kx=K)
    return dict(H=np.ascontiguousarray(H), g=g, x=np.ascontiguousarray(y), lam=lam, lin=spec)


# the points: 'near-MAP' (tests/hessian_shapes.py; H is indefinite there and the ladder climbs ten rungs and more from 1e-3) and 'MAP',
# the stationary point bdrt_optimize reaches from it (tests/golden/newton_map_points.npz, |g|inf < 1e-8): -H is positive definite
# there and with the small damping the iteration has at its end the diagonal of M spans 1e-6 .. 1e6, its condition is 1e12 .. 1e13
PROJECT_POINTS = {'near-MAP': LAM0, 'MAP': 1e-6}


def project_point(name, point):
    """(y, the damping the ladder starts from)"""
    nf, K, pos, irr = hs.SHAPES[name]
    if point == 'MAP':
        from tests.helpers import load
        return np.ascontiguousarray(load('newton_map_points')[name]), PROJECT_POINTS[point]
    return hs.near_map_point(K, pos), PROJECT_POINTS[point]


# ---- the verdict ------------------------------------------------------------------------------------------------------------

ACC_D, ACC_OX, ACC_KX = 37, 2, 12


def _accept_base(lp=-1234.5):
    rs = np.random.RandomState(9)
    D = ACC_D
    x, s = rs.uniform(-1, 1, D), rs.normal(size=D)
    lam, gs, ss = 1e-2, 3.0, 50.0
    st = dict(lp=lp, lam=lam, pred=0.5 * (gs + lam * ss), gs=gs, ss=ss, grad_inf=10.0, tol=1e-8, iters=3, max_iter=300, rc=1, done=0,
              need_hess=0, n_evals=17, lin=0, lp_trial=0.0)
    trial = np.array([x + 2.0 ** -t * s for t in range(4)])
    gt = rs.normal(size=(4, D))
    gt *= np.array([5.0, 6.0, 7.0, 8.0])[:, None] / np.max(np.abs(gt), axis=1)[:, None]       # |g|inf 5, 6, 7, 8 at t = 0 .. 3
    return dict(st=st, x=x, g=rs.normal(size=D), trial=trial, lp_t=np.full(4, lp - 1.0), gt=gt, lin=None)


def pred_of(st, t):
    """predicted increase of the step 2^-t s from the state's gs, ss, lam (with (-H + lam I) s = g: s^T H s = lam s.s - g.s)"""
    sc = 2.0 ** -t
    return sc * st['gs'] + 0.5 * sc * sc * (st['lam'] * st['ss'] - st['gs'])


def accept_cases():
    """name -> (inputs, expected: taken step t or None, and the state fields lam, iters, rc, done, need_hess)"""
    out = {}

    def add(name, c, taken, lam, iters, rc, done, need_hess):
        out[name] = (c, dict(taken=taken, lam=lam, iters=iters, rc=rc, done=done, need_hess=need_hess))

    lam = 1e-2
    for name, frac, newlam in (('full step, rho above 0.75', 0.9, lam / 5.0), ('full step, rho between', 0.5, lam), ('full step, rho below 0.25', 0.1, lam * 2.0)):
        c = _accept_base(); c['lp_t'][0] = c['st']['lp'] + frac * c['st']['pred']
        add(name, c, 0, newlam, 4, 1, 0, 1)
    c = _accept_base(); c['st']['lam'] = 2e-12; c['st']['pred'] = 0.5 * (3.0 + 2e-12 * 50.0); c['lp_t'][0] = c['st']['lp'] + 0.9 * c['st']['pred']
    add('full step, damping at its floor 1e-12', c, 0, 1e-12, 4, 1, 0, 1)
    for t in (1, 2, 3):
        c = _accept_base(); c['lp_t'][t] = c['st']['lp'] + 0.5 * pred_of(c['st'], t)
        add('shortened step t = %d' % t, c, t, lam * 2.0 ** t, 4, 1, 0, 1)
        # an increase between the shortened step's bound 1e-4 pred(t) and what the bound would be without the - g.s term of s^T H s:
        # passes, and a verdict that leaves the term out refuses it (at t = 3 it then takes nothing: 16 lam)
        c = _accept_base(); st = c['st']; sc = 2.0 ** -t
        wrong = sc * st['gs'] + 0.5 * sc * sc * st['lam'] * st['ss']
        c['lp_t'][t] = st['lp'] + 1e-4 * 0.5 * (pred_of(st, t) + wrong)
        add('shortened step t = %d just above its bound' % t, c, t, lam * 2.0 ** t, 4, 1, 0, 1)
        c = _accept_base(); c['lp_t'][t] = c['st']['lp'] + 1e-4 * 0.9 * pred_of(c['st'], t)
        add('shortened step t = %d just below its bound' % t, c, None, lam * 16.0, 3, 1, 0, 0)
    add('no step', _accept_base(), None, lam * 16.0, 3, 1, 0, 0)
    for name, bad in (('lp_t[0] nan', np.nan), ('lp_t[0] +inf', np.inf), ('lp_t[0] -inf', -np.inf)):
        c = _accept_base(); c['lp_t'][0] = bad; c['lp_t'][1] = c['st']['lp'] + 0.5 * pred_of(c['st'], 1)
        add(name, c, 1, lam * 2.0, 4, 1, 0, 1)
    for name, bad, at in (('gradient nan at t = 0', np.nan, 36), ('gradient inf at t = 0', np.inf, 0)):
        c = _accept_base(); c['lp_t'][0] = c['st']['lp'] + 0.9 * c['st']['pred']; c['gt'][0, at] = bad
        c['lp_t'][1] = c['st']['lp'] + 0.5 * pred_of(c['st'], 1)
        add(name, c, 1, lam * 2.0, 4, 1, 0, 1)
    # the noise rule: the predicted increase far below 64 eps |lp| (77 ulp of lp here), lp_t 16 ulp lower, the gradient lower
    for name, ginf_scale, taken in (('noise rule', 1.0, 0), ('noise rule, gradient not lower', 4.0, None)):
        c = _accept_base(); st = c['st']
        st['gs'], st['ss'] = 1e-14, 1e-12; st['pred'] = 0.5 * (st['gs'] + st['lam'] * st['ss'])
        c['lp_t'][:] = st['lp'] - 16 * np.spacing(abs(st['lp']))
        c['gt'] *= ginf_scale                                   # |g|inf 5 .. 8 against the state's 10, or 20 .. 32
        if taken is None:
            add(name, c, None, lam * 16.0, 3, 1, 0, 0)
        else:
            add(name, c, 0, lam * 2.0, 4, 1, 0, 1)              # rho < 0
    c = _accept_base(-0.75); st = c['st']                       # |lp| < 1: noise = 64 eps; lp_t 16 ulp of lp (= 8 eps) lower
    st['gs'], st['ss'] = 1e-17, 1e-15; st['pred'] = 0.5 * (st['gs'] + st['lam'] * st['ss'])
    c['lp_t'][:] = st['lp'] - 16 * np.spacing(abs(st['lp']))
    add('noise rule, |lp| below 1', c, 0, lam * 2.0, 4, 1, 0, 1)
    c = _accept_base(); c['lp_t'][0] = c['st']['lp'] + 0.5 * c['st']['pred']; c['gt'][0] *= 1e-9 / 5.0
    add('converged', c, 0, lam, 4, 0, 1, 0)
    c = _accept_base(); c['st']['iters'] = 299; c['lp_t'][0] = c['st']['lp'] + 0.5 * c['st']['pred']
    add('iteration cap', c, 0, lam, 300, 1, 1, 0)
    c = _accept_base(); c['st']['iters'] = 299; c['lp_t'][0] = c['st']['lp'] + 0.5 * c['st']['pred']; c['gt'][0] *= 1e-9 / 5.0
    add('converged at the iteration cap', c, 0, lam, 300, 0, 1, 0)
    # the floor rule (linear scale): every |g_y| is 1e-9 < tol, but a coefficient within 4 floors of the floor has g_y > 0: it counts as
    # g_y / x * 1e14 floor = 5e3, so the fit is NOT converged; a negative g_y there, or a coefficient 8 floors up, leaves it converged
    floor = 1e-14
    for name, xj, sign, conv in (('floor rule', 2.0 * floor, 1.0, False), ('floor rule, gradient pointing below the floor', 2.0 * floor, -1.0, True),
                                 ('floor rule, coefficient 8 floors up', 8.0 * floor, 1.0, True)):
        c = _accept_base(); c['st']['lin'] = 1
        j = ACC_OX + 5
        c['lin'] = dict(tz=np.ones(ACC_D), held=np.zeros(ACC_D), floor=floor, o_x=ACC_OX, Kx=ACC_KX)
        c['lp_t'][0] = c['st']['lp'] + 0.5 * c['st']['pred']; c['gt'][0] *= 1e-10 / 5.0
        c['trial'][0, j] = np.log(xj); c['gt'][0, j] = sign * 1e-9
        if conv:
            add(name, c, 0, lam, 4, 0, 1, 0)
        else:
            add(name, c, 0, lam, 4, 1, 0, 1)
    # the same coefficient index outside the coefficient slots is an ordinary parameter: no floor rule
    c = _accept_base(); c['st']['lin'] = 1
    c['lin'] = dict(tz=np.ones(ACC_D), held=np.zeros(ACC_D), floor=floor, o_x=ACC_OX, Kx=ACC_KX)
    c['lp_t'][0] = c['st']['lp'] + 0.5 * c['st']['pred']; c['gt'][0] *= 1e-10 / 5.0
    for j in (ACC_OX - 1, ACC_OX + ACC_KX):
        c['trial'][0, j] = np.log(2.0 * floor); c['gt'][0, j] = 1e-9
    add('floor rule, slots next to the coefficients', c, 0, lam, 4, 0, 1, 0)
    return out
