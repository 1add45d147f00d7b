"""GPU tests (-m gpu): every log-posterior evaluator of the single-distribution family against the LONGDOUBLE statement
(tests/logp_numpy.py), lp and the gradient class by class, each component relative to the sum of the absolute values of its own
terms (logp_mismatch), within the tolerances of tests/logp_cases.py (measured by tests/test_logp_reference_host.py on the float64
references at these same problems and points, never on a kernel).  The cases -- path, problem, switches of DESIGN.md 7b, expected evaluator code, entry -- are
tests/logp_cases.py::CASES; each is evaluated once, with the Jacobian on and off, and every class is a test of its own.

Every side reads the same matrices: the cases' L are exactly Toeplitz (tests/logp_cases.py::exactly_toeplitz), so the structured L
path, which keeps one number per diagonal, the dense path, the oracle and the statement evaluate one matrix and the comparison is
about arithmetic alone.  (What one number per diagonal costs against L as the constructors round it -- up to 10.5 tolerances in
ups, the same for every structured reader -- is measured on the CPU, tests/test_logp_reference_host.py.)  No case is excepted.

Which kernel ran.  bdrt_problem_evaluator reports the tile evaluator's code and is asserted where a switch selects one.  The
one-workgroup-per-point rows have no such report: bdrt_logp_grad chooses them by the batch size alone when BDRT_FEW_POINTS is unset
(up to one point per CU the plain variant, beyond it the register-tight one), so those rows are what that entry
does at B = 1, 5 and 300, whichever kernel that is; the solo and wave rows call their debug entries directly.

Every comparison prints one line: path, problem, shape, batch, Jacobian, point set, then per class the
kernel's worst ratio / the references' recorded ratio / the tolerance.  The lines are appended to the file BDRT_LOGP_PARITY_OUT
names, when set (profiles/logp_classes/parity.txt)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import logp_cases as lc
from tests.logp_cases import REF, tol
from tests.logp_numpy import CLASSES, logp_mismatch

pytestmark = pytest.mark.gpu

SWITCHES = ('BDRT_STREAM_A', 'BDRT_GENERIC_TILE', 'BDRT_DENSE_L', 'BDRT_BIG', 'BDRT_TOEP_GEN', 'BDRT_WAVE_OCC', 'BDRT_FEW_POINTS')


def _record(line):
    print(line)
    path = os.environ.get('BDRT_LOGP_PARITY_OUT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _debug_logp_grad(prob, entry, theta, jac):
    fn = getattr(prob._lib, 'bdrt_debug_%s_logp_grad' % entry)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lp = np.empty(len(theta)); g = np.empty_like(theta)
    rc = fn(prob.handle, theta.ctypes.data, None, len(theta), int(jac), lp.ctypes.data, g.ctypes.data)
    assert rc == 0, prob._lib.bdrt_last_error().decode()
    return lp, g


_results = {}


def _evaluate(case):
    """the case's evaluator at its batch, once: {'rows', 'compared', jac: (lp [B], g [B, D])}"""
    key = lc.case_id(case)
    if key in _results:
        return _results[key]
    from bayes_drt_amd.model import Problem
    path, name, env, code, entry, rows = case
    P = lc.problem(name)
    th_all = lc.points(name)[0]
    rows = list(range(len(th_all))) if rows is None else list(rows)
    theta = np.ascontiguousarray(th_all[rows])
    out = dict(rows=rows, compared=list(lc.FEW_300_COMPARED) if len(rows) == 300 else list(range(len(rows))))
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        if entry != 'few':
            mp.setenv('BDRT_FEW_POINTS', '0')
        prob = Problem([P['blk']], P['Z'], P['f'], **P['kw'])
        try:
            assert prob.D == theta.shape[1]
            if code is not None:
                assert prob.evaluator() == code, (path, name, prob.evaluator())            # the switch did switch
            for jac in (True, False):
                if entry in ('solo', 'wave'):
                    out[jac] = _debug_logp_grad(prob, entry, theta, jac)
                else:
                    out[jac] = prob.logp_grad(theta, jacobian=jac)
        finally:
            prob.close()
    _results[key] = out
    return out


_compared = {}


def _compare(case):
    """{class: [(ratio, tolerance, Jacobian, batch row, point set) beyond the tolerance]} of the case against the longdouble
    statement; prints the parity lines the first time"""
    key = lc.case_id(case)
    if key in _compared:
        return _compared[key]
    path, name = case[0], case[1]
    P = lc.problem(name)
    nf, K = P['nf'], P['K']
    sets = lc.points(name)[1]
    out = _evaluate(case)
    rows = out['rows']
    bad = {cls: [] for cls in ('lp',) + CLASSES}
    for jac in (True, False):
        lp, g = out[jac]
        refs = lc.references(name, jac)
        worst = {}
        for b in out['compared']:
            i = rows[b]
            for cls, v in logp_mismatch(lp[b], g[b], refs[i]).items():
                t = tol(sets[i], cls, nf, K)
                if v / t >= worst.get((sets[i], cls), (-1.0,))[0]:
                    worst[(sets[i], cls)] = (v / t, v, t)
                if not v <= t:
                    bad[cls].append((v, t, jac, b, sets[i]))
        for s in dict.fromkeys(sets[rows[b]] for b in out['compared']):
            _record('%-26s %-22s %3d x %-3d B %3d jac %d %-8s | %s' % (
                path, name, nf, K, len(rows), jac, s,
                '  '.join('%s %.1e / %.1e / %.1e' % (cls, worst[(s, cls)][1], REF[s][cls], worst[(s, cls)][2])
                          for cls in ('lp',) + CLASSES if (s, cls) in worst)))
    _compared[key] = bad
    return bad


def _params():
    for case in lc.CASES:
        for cls in ('lp',) + CLASSES:
            if cls != 'so' or lc.has_outlier_model(case[1]):
                yield pytest.param(case, cls, id='%s-%s' % (lc.case_id(case), cls))


@pytest.mark.parametrize('case,cls', list(_params()))
def test_evaluator_holds_the_class_to_the_longdouble_statement(case, cls):
    bad = _compare(case)[cls]
    assert not bad, (max(v / t for v, t, *_ in bad), bad[:4])
