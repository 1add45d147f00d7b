"""The Newton iteration's damped solve and its verdict on the trial points, stated plainly in numpy -- written from DESIGN.md 3.3 and
the host state machine csrc/bdrt_newton.h (NewtonFit::make_trial, ::consume), not from the kernels of csrc/bdrt_newton.hip -- and the
backward-error measures that hold a Cholesky factor, a solve and the predicted increase to Higham's bounds (Accuracy and Stability of
Numerical Algorithms, 2nd ed., Thms 10.3 and 10.4).  Shared by tests/test_newton_reference_host.py (LAPACK's factor through the same
measures, no GPU) and tests/test_gpu_newton_solve.py (the kernels' factor).  Test infrastructure, not the product.

One round, with H the Hessian of the log-posterior, g its gradient, x the point, lam the damping:
  ladder   M = -H + lam 4^j I for j = 0, 1, ... while lam 4^j <= 1e12: the first rung with a Cholesky factor and a finite step
  step     s = M^-1 g;  predicted increase of the quadratic model  pred = g.s + 1/2 s^T H s
  trial    x + 2^-t s for t = 0 .. 3; a coefficient on the linear scale: log(max(exp(x) + 2^-t s, floor)), with the right-hand side
           g_z = g tz there and zero for a coefficient held at its floor
  verdict  the longest step that passes the sufficient-increase test (or the noise rule) is taken: accept()."""
import numpy as np
import scipy.linalg as sla

U = 2.0 ** -53
LAM_MAX = 1e12
N_TRY = 4
LD = np.longdouble


def gamma(k):
    return k * U / (1.0 - k * U)


def padded(D):
    return (D + 15) & ~15


# ---- the statement ----------------------------------------------------------------------------------------------------------

def rhs(g, lin=None):
    """the gradient in the iteration's coordinates.  lin: None (log scale) or dict(tz, held, floor, o_x, Kx)"""
    if lin is None:
        return np.array(g, dtype=float)
    return np.where(np.asarray(lin['held']) != 0, 0.0, np.asarray(g, dtype=float) * np.asarray(lin['tz'], dtype=float))


def damped(H, lam):
    return -np.asarray(H, dtype=float) + lam * np.eye(len(H))


def lapack_factor(M):
    """lower Cholesky factor by LAPACK (dpotrf), None when it reports a non-positive pivot"""
    try:
        return np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None


def lapack_solve(L, b):
    y = sla.solve_triangular(L, b, lower=True, check_finite=False)
    return sla.solve_triangular(L, y, lower=True, trans='T', check_finite=False)


def ladder(H, g, x, lam0, lin=None):
    """dict(ok, lam, rung, refused, L, s, rhs): the first rung lam0 4^j <= 1e12 that factors and gives a finite trial point; refused: the
    dampings that did not.  ok False: no rung did, lam is the first damping beyond 1e12 (the iteration ends with rc 2)."""
    b = rhs(g, lin)
    lam, j, refused = float(lam0), 0, []
    while lam <= LAM_MAX:
        L = lapack_factor(damped(H, lam))
        if L is not None:
            s = lapack_solve(L, b)
            if np.all(np.isfinite(np.asarray(x) + s)):
                return dict(ok=True, lam=lam, rung=j, refused=refused, L=L, s=s, rhs=b)
        refused.append(lam)
        lam *= 4.0
        j += 1
    return dict(ok=False, lam=lam, rung=j, refused=refused, L=None, s=None, rhs=b)


def predicted_increase(H, b, s):
    """g.s + 1/2 s^T H s in extended precision (b: the right-hand side rhs(g))"""
    Hl, bl, sl = np.asarray(H, dtype=LD), np.asarray(b, dtype=LD), np.asarray(s, dtype=LD)
    return bl @ sl + LD(0.5) * (sl @ (Hl @ sl))


def trial_points(x, s, lin=None):
    """[4][D]: x + 2^-t s; the coefficient slots of the linear scale log(max(exp(x) + 2^-t s, floor))"""
    x, s = np.asarray(x, dtype=float), np.asarray(s, dtype=float)
    out = np.empty((N_TRY, len(x)))
    for t in range(N_TRY):
        sc = 2.0 ** -t
        out[t] = x + sc * s
        if lin is not None:
            k = slice(lin['o_x'], lin['o_x'] + lin['Kx'])
            out[t, k] = np.log(np.maximum(np.exp(x[k]) + sc * s[k], lin['floor']))
    return out


class _Margins:
    """every comparison the verdict makes, with its distance from equality relative to the larger side.  Comparisons of lp_t with lp
    less an allowance are taken between the difference lp_t - lp and the allowance: that is the scale on which they are decided."""

    def __init__(self):
        self.least = np.inf
        self.log = []

    def _note(self, what, a, b):
        if np.isfinite(a) and np.isfinite(b):
            den = max(abs(a), abs(b))
            m = abs(a - b) / den if den > 0 else np.inf
            self.log.append((what, a, b, m))
            self.least = min(self.least, m)

    def ge(self, what, a, b):
        self._note(what, a, b); return a >= b

    def gt(self, what, a, b):
        self._note(what, a, b); return a > b

    def lt(self, what, a, b):
        self._note(what, a, b); return a < b

    def le(self, what, a, b):
        self._note(what, a, b); return a <= b


def accept(st, x, g, trial, lp_t, gt, lin=None):
    """The verdict on the trial points t = 0 .. 3 (steps s, s/2, s/4, s/8), the first that passes is taken.
    st: dict(lp, lam, pred, gs, ss, grad_inf, tol, iters, max_iter, rc, done, need_hess, n_evals); pred, gs = g.s and ss = s.s belong to
    the full step.  Returns (new state, x, g, margins).

    The quadratic model along the direction: pred(t) = 2^-t g.s + 1/2 4^-t s^T H s, and with the full step's pred = g.s + 1/2 s^T H s
    that is 2^-t g.s + 4^-t (pred - g.s).
    sufficient increase:  lp_t - lp >= 1e-4 pred(t)  and  lp_t >= lp - 1e-12 |lp|,  all of lp_t, gt finite;
    noise rule: where pred(t) is below noise = 64 eps max(1, |lp|), a step that does not lower lp by more than noise and lowers |g|inf passes;
    |g|inf of a trial point: max |gt|, except that a coefficient on the linear scale within 4 floors of its floor with a positive
    gradient counts as gt / x * 1e14 floor (the floor rule: g_y = x g_x vanishes at the floor whatever g_x is);
    accepted at t = 0: rho = (lp_t - lp) / pred (0 when pred <= 0); rho > 0.75: lam / 5, not below 1e-12; rho < 0.25: 2 lam;
    accepted at t > 0: 2^t lam;  none accepted: 16 lam, same point;
    after an accepted step: iters + 1; |g|inf < tol: converged (rc 0); else iters >= max_iter: rc 1; else a new Hessian is needed."""
    st = dict(st)
    mg = _Margins()
    x, g = np.array(x, dtype=float), np.array(g, dtype=float)
    lp, lam0, pred0, gs = st['lp'], st['lam'], st['pred'], st['gs']
    st['n_evals'] = st.get('n_evals', 0) + N_TRY
    st['lp_trial'] = float(lp_t[0])
    noise = 64.0 * 2.0 ** -52 * max(1.0, abs(lp))
    for t in range(N_TRY):
        sc = 2.0 ** -t
        lpn, gtt = float(lp_t[t]), np.asarray(gt[t], dtype=float)
        fin = bool(np.isfinite(lpn) and np.all(np.isfinite(gtt)))
        v = gtt.copy()
        if lin is not None and fin:
            for j in range(lin['o_x'], lin['o_x'] + lin['Kx']):
                xj = np.exp(trial[t][j])
                if v[j] > 0.0 and mg.le('floor rule t=%d j=%d' % (t, j), xj, 4.0 * lin['floor']):
                    v[j] = v[j] / xj * (1e14 * lin['floor'])
        ginf = float(np.max(np.abs(v))) if fin else np.nan
        pred = pred0 if t == 0 else sc * gs + sc * sc * (pred0 - gs)
        acc = False
        if fin:
            inc = mg.ge('increase t=%d' % t, lpn - lp, 1e-4 * pred)
            nodrop = mg.ge('no drop t=%d' % t, lpn - lp, -1e-12 * abs(lp))
            acc = inc and nodrop
            if not acc:
                small = mg.lt('pred below noise t=%d' % t, pred, noise)
                flat = mg.ge('lp within noise t=%d' % t, lpn - lp, -noise)
                lower = mg.lt('gradient lower t=%d' % t, ginf, st['grad_inf'])
                acc = small and flat and lower
        if not acc:
            continue
        rho = (lpn - lp) / pred if pred > 0.0 else 0.0
        st['lp'] = lpn
        if t == 0:
            if mg.gt('rho > 0.75', rho, 0.75):
                st['lam'] = max(lam0 / 5.0, 1e-12)
            elif mg.lt('rho < 0.25', rho, 0.25):
                st['lam'] = lam0 * 2.0
        else:
            st['lam'] = lam0 * 2.0 ** t
        st['iters'] += 1
        st['grad_inf'] = ginf
        if mg.lt('converged', ginf, st['tol']):
            st['rc'], st['done'] = 0, 1
        elif st['iters'] >= st['max_iter']:
            st['rc'], st['done'] = 1, 1
        else:
            st['need_hess'] = 1
        return st, np.array(trial[t], dtype=float), gtt.copy(), mg
    st['lam'] = lam0 * 16.0
    return st, x, g, mg


# ---- the measures -----------------------------------------------------------------------------------------------------------

LD_MAX_D = 544          # the factor's residual is evaluated in extended precision up to here, in float64 (+ gamma_Dp) above


def pad_identity(M, Dp):
    out = np.eye(Dp)
    D = len(M)
    out[:D, :D] = M
    return out


UNDERFLOW = 2.0 ** -1022 / U     # below this a bound u |..| is itself subnormal: the rounding model says nothing relative there


def _ratio_max(num, den):
    """max num / den over den >= UNDERFLOW; inf when num is that large somewhere den is not"""
    num, den = np.asarray(num, dtype=float), np.asarray(den, dtype=float)
    if np.any((den < UNDERFLOW) & (num >= UNDERFLOW)) or not np.all(np.isfinite(num)):
        return np.inf
    nz = den >= UNDERFLOW
    return float(np.max(num[nz] / den[nz])) if np.any(nz) else 0.0


def factor_omega(M, L, rows=None, extended=True):
    """max over the lower triangle (of `rows`, default all) of |M - L L^T| / (|L| |L|^T), in units of u.  M, L [n x n], L lower
    triangular.  extended: the product in np.longdouble (its own error, 2^-64 n, is 1/2048 of a unit per term of the sum)."""
    n = len(M)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    dt = LD if extended else float
    Lt = np.tril(L)
    Lr, La = Lt[rows].astype(dt), Lt.astype(dt)
    R = np.abs(np.asarray(M)[rows].astype(dt) - Lr @ La.T)
    B = np.abs(Lt[rows]) @ np.abs(Lt).T              # (float64: a sum of nonnegative terms, good to n u relative)
    low = np.arange(n)[None, :] <= rows[:, None]
    return _ratio_max(np.where(low, R, 0), np.where(low, B, 0)) / U


def factor_bound_omega(Dp, extended=True):
    """Higham Thm 10.3, |M - L L^T| <= gamma_{n+1} |L||L^T|, twice (reciprocal pivots, a sqrt that is not correctly rounded); evaluated
    in float64, gamma_n more for the evaluation of the product itself.  In units of u."""
    return (2.0 * gamma(Dp + 1) + (0.0 if extended else gamma(Dp))) / U


def sample_rows(Dp):
    """rows at which the parity measure of a wide factor is taken in extended precision: one row of every 16-row block, moving through
    the block, and every row of the last two blocks (the end of the trailing updates)"""
    r = set(16 * b + (5 * b) % 16 for b in range(Dp // 16)) | set(range(max(0, Dp - 32), Dp))
    return np.array(sorted(r))


def absLLt_s(L, s):
    Lt = np.abs(np.tril(L)).astype(LD)
    return Lt @ (Lt.T @ np.abs(np.asarray(s, dtype=LD)))


def solve_ratio(M, L, b, s):
    """max_i |b - M s|_i / (2 gamma_{3n+1} (|L||L^T||s|)_i)  (Higham Thm 10.4; the residual in extended precision): <= 1 holds the solve"""
    n = len(M)
    r = np.abs(np.asarray(b, dtype=LD) - np.asarray(M, dtype=LD) @ np.asarray(s, dtype=LD))
    return _ratio_max(r, 2.0 * gamma(3 * n + 1) * absLLt_s(L, s))


def pred_check(H, b, s, lam, L, Dp, pred, gs, ss):
    """(error, bound) of pred, gs and ss.  pred is formed as 1/2 (g.s + lam s.s), which equals g.s + 1/2 s^T H s up to
    1/2 s^T (residual of the solve): |pred - (g.s + 1/2 s^T H s)| <= 1/2 |s|^T 2 gamma_{3Dp+1} |L||L^T||s| + gamma_Dp (|g|^T|s| + lam s^T s);
    gs and ss to gamma_Dp of their absolute sums."""
    bl, sl = np.asarray(b, dtype=LD), np.asarray(s, dtype=LD)
    ags, ass = np.abs(bl) @ np.abs(sl), sl @ sl
    ref = predicted_increase(H, b, s)
    bound = 0.5 * (np.abs(sl) @ (2.0 * gamma(3 * Dp + 1) * absLLt_s(L, s))) + gamma(Dp) * (ags + lam * ass)
    return dict(pred=(float(abs(LD(pred) - ref)), float(bound)), gs=(float(abs(LD(gs) - bl @ sl)), float(gamma(Dp) * ags)),
                ss=(float(abs(LD(ss) - ass)), float(gamma(Dp) * ass)))


def rung_margin_ok(H, lam, Dp, accepted):
    """an accepted rung has lam_min(M) >= -Dp gamma_{Dp+1} |M|_2, a refused one lam_min(M) <= +Dp gamma_{Dp+1} |M|_2 (a factorisation
    that runs to completion has a nearby positive semidefinite matrix; one that breaks down has a nearby singular one)"""
    w = np.linalg.eigvalsh(damped(H, lam))
    tol = Dp * gamma(Dp + 1) * max(abs(w[0]), abs(w[-1]))
    return (w[0] >= -tol) if accepted else (w[0] <= tol)
