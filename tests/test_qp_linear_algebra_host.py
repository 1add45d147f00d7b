"""The inputs and measures of tests/test_gpu_qp_linear_algebra.py without a GPU: every case of tests/qp_cases.py through LAPACK's
factor and solves, numpy's Gram products and the numpy ladder of tests/qp_numpy.py, held to the same bounds -- so every input the GPU
tests use is one that a correct implementation passes, and every planted rung is the one the statement commits.  And the debug
entry is part of the bound ABI."""
import numpy as np
import pytest

from bayes_drt_amd import _lib
from tests import newton_numpy as nn
from tests import qp_cases as qc
from tests import qp_numpy as qn


def lapack_outputs(P, dg, rhs):
    """the statement's ladder with LAPACK's factor and solves, in the shape of the debug entry's outputs"""
    R = qn.ladder(P, dg)
    if not R['ok']:
        return dict(ok=0, rungs=R['rungs'], reg=R['reg'], L=None, piv=None, sol=None)
    L = R['L']
    return dict(ok=1, rungs=R['rungs'], reg=R['reg'], L=L, piv=np.diag(L) ** 2, sol=np.stack([nn.lapack_solve(L, b) for b in rhs]))


def test_the_lds_limit_is_the_documented_one():
    assert (qc.N_LAST_LDS, qc.N_BEYOND_LDS) == (185, 186)


@pytest.mark.parametrize('kind', qc.KINDS)
@pytest.mark.parametrize('n', sorted(qc.SIZES))
def test_lapack_passes_every_factor_and_solve_case(n, kind):
    P, dg = qc.kkt_case(n, kind)
    rhs, cols = qc.rhs_case(n, kind)
    m = qn.check_factor_solve(P, dg, rhs, cols, lapack_outputs(P, dg, rhs), 'n %d %s' % (n, kind), expect_rung=0)
    assert m['ratio'] in (0.0, 1.0)
    # the unsymmetric partner symmetrises to the quantised matrix exactly, and that one factors at reg = 0 too
    Pq = qc.quantised(P)
    assert np.array_equal(qn.kkt(qc.antisymmetric_partner(Pq, n, kind), dg), qn.kkt(Pq, dg)) and qn.ladder(Pq, dg)['rung'] == 0
    if n > 1:
        assert not np.array_equal(qc.antisymmetric_partner(Pq, n, kind), Pq)


@pytest.mark.parametrize('n', qc.PLANTED_N)
def test_every_planted_rung_is_the_one_the_statement_commits(n):
    rungs = qc.planted_rungs(n)
    assert len(rungs) >= 6, rungs
    for j in rungs:
        P, dg, lam, rung, reg = qc.planted_case(n, j)
        w = np.linalg.eigvalsh(qn.kkt(P, dg))
        assert abs(w[0] / lam - 1.0) < 1e-6 and w[1] >= 1.0 - 1e-9, (j, w[0], lam)
        rhs, cols = qc.rhs_case(n, 'full')
        out = lapack_outputs(P, dg, rhs)
        assert out['reg'] == reg
        qn.check_factor_solve(P, dg, rhs, cols, out, 'planted n %d rung %d' % (n, rung), expect_rung=rung)


def test_the_hopeless_matrix_exhausts_the_ladder():
    P, dg = qc.hopeless_case()
    R = qn.ladder(P, dg)
    assert not R['ok'] and R['reg'] > 1e6 and R['rungs'] == len(qn.regs(P[0, 0])[0])
    assert all(qn.rung_margin_ok(P, dg, reg, accepted=False) for reg in R['refused'])


@pytest.mark.parametrize('n', qc.BREAK_N)
def test_breakdown_cases_break_down_and_their_planted_twins_factor(n):
    for c in qc.break_columns(n):
        P, dg, vals = qc.breakdown_case(n, c, hopeless=True)
        assert not qn.ladder(P, dg)['ok']
        P, dg, vals = qc.breakdown_case(n, c, hopeless=False)
        R = qn.ladder(P, dg)
        # the least eigenvalue lies between two rungs, a factor 3 and more from either: the verdict is not a matter of rounding
        w0 = -np.linalg.eigvalsh(qn.kkt(P, dg))[0]
        assert R['ok'] and vals[R['rung'] - 1] * 3.0 <= w0 <= vals[R['rung']] / 3.0, (c, w0, R['rung'])
        assert qn.pinnable(vals[R['rung'] - 1], n, np.linalg.norm(P, 2))
        rhs, cols = qc.rhs_case(n, 'full')
        qn.check_factor_solve(P, dg, rhs, cols, lapack_outputs(P, dg, rhs), 'breakdown n %d c %d' % (n, c), expect_rung=R['rung'])


@pytest.mark.parametrize('cell', qc.NAN_CELLS)
def test_a_nan_is_refused_by_the_statement(cell):
    P, dg = qc.nan_case(cell)
    assert not qn.ladder(P, dg)['ok']


def test_the_isolation_batch_is_one_of_each():
    P, dg, rung = qc.isolation_case()
    R = [qn.ladder(P[b], dg[b]) for b in range(3)]
    assert [r['ok'] for r in R] == [True, True, False] and R[0]['rung'] == 0 and R[1]['rung'] == rung > 1


@pytest.mark.parametrize('nrows,n', qc.GRAM_SHAPES)
def test_numpy_passes_every_gram_case(nrows, n):
    c = qc.gram_case(nrows, n)
    A, z = c['A'], c['z']
    assert np.array_equal(c['L2'], c['L2'].T)
    assert qn.gram_ratio(A.T @ A, A) <= 1.0 and qn.gram_ratio(A.T @ A + c['L2'], A, c['L2']) <= 1.0
    assert qn.gram_q_ratio(-(A.T @ z), A, z) <= 1.0 and qn.gram_q_ratio(-(A.T @ z) + c['L1'], A, z, c['L1']) <= 1.0
    for g in range(qc.GRAM_NG):
        WA, wz = qn.batch_rows(A, c['w'][g], c['t'][g])
        assert qn.gram_ratio(WA.T @ WA, WA) <= 1.0 and qn.gram_q_ratio(-(WA.T @ wz) + c['L1'], WA, wz, c['L1']) <= 1.0
    # the measure notices a dropped last row
    if nrows > 1:
        assert qn.gram_ratio(A[:-1].T @ A[:-1], A) > 1.0


def test_the_measures_notice_a_wrong_factor_and_a_wrong_solve():
    P, dg = qc.kkt_case(33, 'barrier6')
    rhs, cols = qc.rhs_case(33, 'barrier6')
    out = lapack_outputs(P, dg, rhs)
    bad = dict(out, L=out['L'].copy())
    bad['L'][32, 31] *= 1.0 + 1e-13
    with pytest.raises(AssertionError):
        qn.check_factor_solve(P, dg, rhs, cols, bad, 'wrong factor')
    bad = dict(out, sol=out['sol'].copy())
    bad['sol'][0, 5] *= 1.0 + 1e-9
    with pytest.raises(AssertionError):
        qn.check_factor_solve(P, dg, rhs, cols, bad, 'wrong solve')


def test_the_debug_entry_is_bound():
    assert 'bdrt_debug_qp_factor_solve' in _lib.SYMBOLS
    lib = _lib.load_library()
    assert hasattr(lib, 'bdrt_debug_qp_factor_solve') and len(lib.bdrt_debug_qp_factor_solve.argtypes) == 11
    assert [f[0] for f in _lib.QpFactorRecord._fields_] == ['ok', 'rungs', 'reg']
