"""GPU tests (-m gpu) of the ridge path's dense linear algebra, each against a reference of its own operation: the box-QP solver's
form-KKT loop, regularisation ladder, blocked Cholesky of the packed triangle (chol_packed) and blocked substitutions
(chol_solve_blocked) of csrc/bdrt_qp.hip, one launch on supplied data through bdrt_debug_qp_factor_solve; and the Gram kernels of
csrc/bdrt_ridge.hip through bdrt_gram and bdrt_gram_batch.  The statement, the measures and the shared checks are
tests/qp_numpy.py (on tests/newton_numpy.py's), the inputs tests/qp_cases.py; tests/test_qp_linear_algebra_host.py runs the same
inputs through LAPACK and numpy without a GPU.

With u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, Thms 10.3 and 10.4), the bounds
of the factor and the solve twice the textbook's because the kernel multiplies by reciprocal pivots and takes its square roots from
an rsq estimate with two Newton steps:
  factor   |M - L L^T| <= 2 gamma_{n+1} |L||L^T| componentwise in np.longdouble; diag^2 within 4 ulp of the kept pivot
  parity   omega = the factor's largest componentwise ratio / u: the kernel's at most 4 x LAPACK's on the same matrix
  solve    |b - M s| <= 2 gamma_{3n+1} |L||L^T||s| componentwise; for a unit vector also |s - x| <= |M^-1| (r(s) + r(x)) against the
           column x of LAPACK's inverse, r the residual bound
  sym      P and P + S, S antisymmetric, give the same bits (a strict upper triangle read where the lower one belongs would not)
  place    the triangle in LDS and in the global work buffer: the same L, pivots, reg and solutions bit for bit
  ladder   an eigenvalue planted between two rungs commits the upper one, reg bit-equal to the statement's; every refused and every
           accepted rung of every case has the margin of newton_numpy.rung_margin_ok; an exhausted ladder returns -3
  Gram     |G - (A^T A + L2)| <= gamma_{R+1} (|A|^T|A| + |L2|), |q - (-A^T z + L1)| <= gamma_{R+1} (|A|^T|z| + |L1|), the references in
           np.longdouble; G = G^T bit for bit
Each line of measurements is appended to the file BDRT_QP_PARITY_OUT names, when set (profiles/qp_solve/parity.txt)."""
import os

import numpy as np
import pytest

from bayes_drt_amd import _lib
from tests import newton_numpy as nn
from tests import qp_cases as qc
from tests import qp_numpy as qn

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _record(line):
    print(line)
    path = os.environ.get('BDRT_QP_PARITY_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def hip_factor_solve(P, dg, rhs, place, expect_rc=0):
    """one launch on nb problems (P [nb, n, n] or [n, n]; rhs [nb, nrhs, n], or [nrhs, n] for every problem): a list of
    dict(ok, rungs, reg, L, piv, sol) per problem.  The output arrays go in filled with SENTINEL."""
    lib = _lib.require_gpu()
    P, dg = _lib.f64(P), _lib.f64(dg)
    if P.ndim == 2:
        P, dg = P[None], dg[None]
    nb, n = dg.shape
    rhs = _lib.f64(rhs)
    if rhs.ndim == 2:
        rhs = np.ascontiguousarray(np.broadcast_to(rhs, (nb,) + rhs.shape))
    nrhs = rhs.shape[1]
    assert P.shape == (nb, n, n) and rhs.shape == (nb, nrhs, n)
    rec = (_lib.QpFactorRecord * nb)()
    L, piv, sol = np.full((nb, n, n), SENTINEL), np.full((nb, n), SENTINEL), np.full((nb, nrhs, n), SENTINEL)
    rc = lib.bdrt_debug_qp_factor_solve(_lib.ptr(P), _lib.ptr(dg), n, nb, int(place), _lib.ptr(rhs), nrhs, rec, _lib.ptr(L), _lib.ptr(piv),
                                        _lib.ptr(sol))
    if rc == -10:
        pytest.exit('bdrt_debug_qp_factor_solve: device error, nothing more is launched: %r' % lib.bdrt_last_error(), returncode=3)
    assert rc == expect_rc, (rc, lib.bdrt_last_error())
    return [dict(ok=rec[b].ok, rungs=rec[b].rungs, reg=rec[b].reg, L=L[b], piv=piv[b], sol=sol[b]) for b in range(nb)]


def _same_bits(a, b):
    return (a['ok'] == b['ok'] and a['rungs'] == b['rungs'] and np.float64(a['reg']).tobytes() == np.float64(b['reg']).tobytes() and
            all(a[k].tobytes() == b[k].tobytes() for k in ('L', 'piv', 'sol')))


def _untouched(o):
    return all(np.all(o[k] == SENTINEL) for k in ('L', 'piv', 'sol'))


def _places(n):
    return (0, 1) if n <= qc.N_LAST_LDS else (1,)


def _line(label, n, place, m):
    _record('%-40s n %3d %s rung %2d | omega kernel %7.2f lapack %6.2f ratio %5.2f (bound %6.0f) | pivots %.2f ulp | solve %.4f, inverse column '
            '%.4f of their bounds' % (label, n, 'lds   ' if place == 0 else 'global', m['rung'], m['omega'], m['omega_ref'], m['ratio'],
                                      nn.factor_bound_omega(n), m['pivot_ulps'], m['solve'], m['inverse']))


def _check_parity(m, label):
    # If this fails inside the Higham bound: find the reason in the arithmetic (order of the MFMA accumulation, for instance) first.
    assert m['omega'] <= 4.0 * m['omega_ref'], (label, m['omega'], m['omega_ref'])


# ---- factor and solve -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', qc.KINDS)
@pytest.mark.parametrize('n', sorted(qc.SIZES))
def test_factor_and_solves_stay_inside_their_bounds(n, kind):
    """Every size at which chol_packed / chol_solve_blocked change their schedule (tests/qp_cases.py::SIZES) times every matrix kind,
    in LDS and in the global work buffer; in the same launch the quantised matrix and its unsymmetric partner."""
    P, dg = qc.kkt_case(n, kind)
    rhs, cols = qc.rhs_case(n, kind)
    Pq = qc.quantised(P)
    batch = np.stack([P, Pq, qc.antisymmetric_partner(Pq, n, kind)])
    outs = {}
    for place in _places(n):
        o = hip_factor_solve(batch, np.stack([dg] * 3), rhs, place)
        outs[place] = o
        label = '%s' % kind
        m = qn.check_factor_solve(P, dg, rhs, cols, o[0], label)
        _line(label, n, place, m)
        _check_parity(m, label)
        qn.check_factor_solve(Pq, dg, rhs, cols, o[1], label + ' quantised')
        assert _same_bits(o[1], o[2]), (label, 'P + S differs from P')
    if len(outs) == 2:
        for b in range(3):
            assert _same_bits(outs[0][b], outs[1][b]), (kind, n, b, 'LDS and global work buffer differ')
        _record('%-40s n %3d lds == global bit for bit (L, pivots, reg, %d solutions)' % (kind, n, len(rhs)))


def test_lds_placement_is_refused_beyond_its_limit_without_a_launch():
    n = qc.N_BEYOND_LDS
    o = hip_factor_solve(np.eye(n), np.zeros(n), np.ones((1, n)), 0, expect_rc=-2)[0]
    assert _untouched(o) and b'LDS' in _lib.load_library().bdrt_last_error()


# ---- the ladder -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', qc.PLANTED_N)
def test_a_planted_eigenvalue_commits_the_rung_above_it(n):
    """all pinnable rungs of one size in one launch; smallest eigenvalue -sqrt(reg_j reg_{j+1}), the rest of the spectrum 1 .. 4"""
    rungs = qc.planted_rungs(n)
    cases = [qc.planted_case(n, j) for j in rungs]
    rhs, cols = qc.rhs_case(n, 'full')
    for place in _places(n):
        outs = hip_factor_solve(np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), rhs, place)
        for (P, dg, lam, rung, reg), o in zip(cases, outs):
            label = 'planted %.3e' % lam
            assert o['ok'] == 1 and o['rungs'] == rung + 1 and np.float64(o['reg']).tobytes() == np.float64(reg).tobytes(), (label, o['rungs'], o['reg'])
            m = qn.check_factor_solve(P, dg, rhs, cols, o, label, expect_rung=rung)
            _line(label, n, place, m)
            _check_parity(m, label)


def test_an_exhausted_ladder_returns_the_productions_verdict():
    P, dg = qc.hopeless_case()
    R = qn.ladder(P, dg)
    for place in (0, 1):
        o = hip_factor_solve(P, dg, np.ones((1, len(dg))), place, expect_rc=-3)[0]
        assert o['ok'] == 0 and o['rungs'] == R['rungs'] and o['reg'] == R['reg'] > 1e6 and _untouched(o)
        _record('hopeless (eigenvalue -4e7)               n %3d %s ok 0 after %d factorisations, reg left at %.3e' % (len(dg), 'lds   ' if place == 0 else 'global', o['rungs'], o['reg']))


@pytest.mark.parametrize('n', qc.BREAK_N)
def test_breakdown_in_a_chosen_column(n):
    """M = L0 D L0^T with one negative D_c, c in the first block, on its edges and in the last column: D_c = -1e7 is refused at every
    rung and writes nothing; D_c between two rungs is accepted at the statement's rung."""
    cols_c = qc.break_columns(n)
    rhs, cols = qc.rhs_case(n, 'full')
    for place in _places(n):
        bad = [qc.breakdown_case(n, c, hopeless=True) for c in cols_c]
        outs = hip_factor_solve(np.stack([b[0] for b in bad]), np.stack([b[1] for b in bad]), rhs, place, expect_rc=-3)
        for c, (P, dg, vals), o in zip(cols_c, bad, outs):
            assert o['ok'] == 0 and o['rungs'] == len(vals) and o['reg'] == qn.ladder(P, dg)['reg'] and _untouched(o), (c, o['ok'], o['rungs'], o['reg'])
        good = [qc.breakdown_case(n, c, hopeless=False) for c in cols_c]
        outs = hip_factor_solve(np.stack([g[0] for g in good]), np.stack([g[1] for g in good]), rhs, place)
        for c, (P, dg, vals), o in zip(cols_c, good, outs):
            label = 'breakdown column %d' % c
            m = qn.check_factor_solve(P, dg, rhs, cols, o, label, expect_rung=qn.ladder(P, dg)['rung'])
            _line(label, n, place, m)
            _check_parity(m, label)


@pytest.mark.timeout(60)
@pytest.mark.parametrize('cell', qc.NAN_CELLS)
def test_a_nan_in_P_is_refused(cell):
    """(0,0): reg itself becomes NaN and the ladder is left at once; a panel cell and the last pivot: every rung breaks down.  The
    ladder is bounded by construction (`!(reg <= 1e6)` leaves it)."""
    P, dg = qc.nan_case(cell)
    R = qn.ladder(P, dg)
    for place in (0, 1):
        o = hip_factor_solve(P, dg, np.ones((1, len(dg))), place, expect_rc=-3)[0]
        assert o['ok'] == 0 and o['rungs'] == R['rungs'] and _untouched(o), (cell, o['ok'], o['rungs'])
        assert np.isnan(o['reg']) if np.isnan(R['reg']) else o['reg'] == R['reg'], (cell, o['reg'], R['reg'])


@pytest.mark.parametrize('place', (0, 1))
def test_problems_of_one_launch_do_not_disturb_each_other(place):
    """accepted at reg = 0, accepted at a planted rung and refused, side by side: each equals its own launch bit for bit"""
    P, dg, rung = qc.isolation_case()
    rhs, _ = qc.rhs_case(P.shape[1], 'full')
    together = hip_factor_solve(P, dg, rhs, place, expect_rc=-3)
    assert [o['ok'] for o in together] == [1, 1, 0] and together[0]['rungs'] == 1 and together[1]['rungs'] == rung + 1
    for b in range(3):
        alone = hip_factor_solve(P[b], dg[b], rhs, place, expect_rc=0 if b < 2 else -3)[0]
        assert _same_bits(together[b], alone), b
    assert _untouched(together[2])


# ---- Gram -------------------------------------------------------------------------------------------------------------------

def _call(name, *args):
    lib = _lib.require_gpu()
    return _lib.check(getattr(lib, name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]), name)


@pytest.mark.parametrize('nrows,n', qc.GRAM_SHAPES)
def test_gram_against_the_extended_precision_product(nrows, n):
    c = qc.gram_case(nrows, n)
    A, z, L2, L1 = c['A'], _lib.f64(c['z']), c['L2'], _lib.f64(c['L1'])
    worst_P, worst_q = 0.0, 0.0
    for with_L in (False, True):
        l2, l1 = (L2, L1) if with_L else (None, None)
        P, q, P2, q2 = np.full((n, n), SENTINEL), np.full(n, SENTINEL), np.full((n, n), SENTINEL), np.full(n, SENTINEL)
        _call('bdrt_gram', A, None, nrows, n, l2, None, P, None)              # P only
        _call('bdrt_gram', A, z, nrows, n, None, l1, None, q)                 # q only
        _call('bdrt_gram', A, z, nrows, n, l2, l1, P2, q2)                    # both
        assert P.tobytes() == P2.tobytes() and q.tobytes() == q2.tobytes()
        assert np.array_equal(P, P.T), 'G is not symmetric bit for bit'
        rP, rq = qn.gram_ratio(P, A, l2), qn.gram_q_ratio(q, A, z, l1)
        worst_P, worst_q = max(worst_P, rP), max(worst_q, rq)
        assert rP <= 1.0 and rq <= 1.0, (with_L, rP, rq)
    _record('gram        nrows %3d n %3d | P %.4f, q %.4f of gamma_%d' % (nrows, n, worst_P, worst_q, nrows + 1))


@pytest.mark.parametrize('nrows,n', qc.GRAM_SHAPES)
def test_gram_batch_against_the_extended_precision_product_of_the_rounded_rows(nrows, n):
    c = qc.gram_case(nrows, n)
    A, w, t, L1 = c['A'], c['w'], c['t'], _lib.f64(c['L1'])
    ng = qc.GRAM_NG
    worst_G, worst_q = 0.0, 0.0
    for with_L in (False, True):
        l1 = L1 if with_L else None
        G, q, G2, q2 = np.full((ng, n, n), SENTINEL), np.full((ng, n), SENTINEL), np.full((ng, n, n), SENTINEL), np.full((ng, n), SENTINEL)
        _call('bdrt_gram_batch', A, nrows, n, w, None, ng, None, G, None)     # G only
        _call('bdrt_gram_batch', A, nrows, n, w, t, ng, l1, None, q)          # q only
        _call('bdrt_gram_batch', A, nrows, n, w, t, ng, l1, G2, q2)           # both
        assert G.tobytes() == G2.tobytes() and q.tobytes() == q2.tobytes()
        for g in range(ng):
            WA, wz = qn.batch_rows(A, w[g], t[g])
            assert np.array_equal(G[g], G[g].T), 'G is not symmetric bit for bit'
            rG, rq = qn.gram_ratio(G[g], WA), qn.gram_q_ratio(q[g], WA, wz, l1)
            worst_G, worst_q = max(worst_G, rG), max(worst_q, rq)
            assert rG <= 1.0 and rq <= 1.0, (with_L, g, rG, rq)
    _record('gram batch  nrows %3d n %3d | G %.4f, q %.4f of gamma_%d' % (nrows, n, worst_G, worst_q, nrows + 1))
