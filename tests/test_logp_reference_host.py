"""CPU tests of the yardstick the log-posterior evaluators are held to per index class (tests/test_gpu_logp_classes.py): the numpy
statement of lp and its gradient (tests/logp_numpy.py) in np.longdouble, the measure logp_mismatch, and the tolerances.

Why per class.  The suite's other comparisons of an evaluator with the fp64 oracle are normwise (old_criterion below): at a point of
Stan's initialisation range the largest |g| is 1e5 .. 1e7 (an x, ups or d component) and the components of Rinf_raw, induc_raw and
the four error parameters are 1 .. 100, so 1e-10 of the largest leaves them four or five digits; near a MAP the whole ups block is
below 2 against a largest |g| of 1e4.  logp_mismatch holds every component to the sum of the absolute values of ITS OWN additive
terms (gabs_j, tests/logp_numpy.py), class by class, and lp to the same sum of its terms (test_the_criterion_has_teeth shows what
the normwise criterion lets through).

Tolerances.  REF[point set][class] is the worst logp_mismatch of three float64 references -- the C oracle, the float64 statement and
the float64 statement with every reduction reversed -- against the longdouble statement, over every problem and point of
tests/logp_cases.py, where the constants live beside the cases (`python -m tests.test_logp_reference_host` prints the table; the
recorded value is 1.5 x the measured one, two digits, so that the repeated measurement may land a little to either side).  tol = max(8 REF, 2 n 2^-53): the 8 is the factor
tests/test_oracle_hessian.py uses over a measured reference ratio (the kernels' other summation orders); the floor is twice the
worst-case bound of a float64 sum of the longest top-level reduction in any order, n = nf + K terms for a gradient component (a
column of A in both parts, or a frequency sum beside a band) and 4 nf + 4 K for lp.  No tolerance comes from a kernel's output.
The largest entries are those of the stored MAPs (x 3.6e-14, err 2.8e-14, R 2.2e-14: the cancellation inside Z - Z_hat at a good
fit, which every float64 evaluation shares); none reaches the cap 8 REF <= 1e-12."""
import numpy as np
import pytest

from tests import logp_cases as lc
from tests.logp_cases import REF, tol
from tests.hessian_numpy import series_hessian
from tests.logp_numpy import CLASSES, class_slices, logp_mismatch, reference, series_logp

def failures(mm, point_set, nf, K):
    """the entries of logp_mismatch's result beyond their tolerance: {class: (ratio, tolerance)}"""
    return {k: (v, tol(point_set, k, nf, K)) for k, v in mm.items() if not v <= tol(point_set, k, nf, K)}


def old_criterion(lp, g, lp_ref, g_ref, gtol=1e-10):
    """the normwise criterion of tests/test_gpu_model.py::_compare"""
    return abs(lp - lp_ref) <= 1e-10 * max(1.0, abs(lp_ref)) and np.max(np.abs(g - g_ref)) <= gtol * max(1.0, np.max(np.abs(g_ref)))


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63


# ---- the gradient statement is the derivative of the lp statement ------------------------------------------------------------------
H_STEP = 1e-4


def _fd_problem(shape, pos, mode):
    if shape == '7x35':
        P = dict(lc._shape('fd7x35', 7, 35, pos, False))
        P['kw'] = dict(P['kw'], **lc._outlier_kw(mode))
    else:
        P = lc._log_uniform('fd33x47', 33, 47, pos, mode)
    return P


@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('jac', [False, True])
@pytest.mark.parametrize('pos', [True, False])
@pytest.mark.parametrize('shape', ['7x35', '33x47'])
def test_gradient_statement_equals_central_differences_of_the_lp_statement(shape, pos, jac, mode):
    """Every component, in longdouble, within 1e-6 gabs_j (a wrong or missing term, not rounding); the step is small enough when the
    differences at h and h / 2 agree to 1e-7 gabs_j."""
    ld = np.longdouble
    P = _fd_problem(shape, pos, mode)
    D = class_slices(P['K'], P['nf'], mode)['d'].stop
    y = np.random.RandomState(7).uniform(-1, 1, D).astype(ld)
    ref = reference(P, y, jac)

    def lp(yy):
        return reference(P, yy, jac)['lp']

    def central(h):
        out = np.empty(D, dtype=ld)
        for j in range(D):
            yp, ym = y.copy(), y.copy()
            yp[j] += h; ym[j] -= h
            out[j] = (lp(yp) - lp(ym)) / (yp[j] - ym[j])
        return out
    g1, g2 = central(ld(H_STEP)), central(ld(H_STEP) / 2)
    step = np.max(np.abs(g1 - g2) / ref['gabs'])
    err = np.max(np.abs(g2 - ref['g']) / ref['gabs'])
    print('%s pos %d jac %d mode %d: h vs h/2 %.1e, statement vs differences %.1e' % (shape, pos, jac, mode, step, err))
    assert step < 1e-7, (step, int(np.argmax(np.abs(g1 - g2) / ref['gabs'])))
    assert err <= 1e-6, (err, int(np.argmax(np.abs(g2 - ref['g']) / ref['gabs'])))


# ---- the new statement agrees with the old one --------------------------------------------------------------------------------------
def test_statement_equals_the_hessian_file_s_lp_and_gradient():
    """float64, no outlier model, no Jacobian: lp and g of tests/hessian_numpy.py::series_hessian to 1e-13 of lp_abs and gabs, at an
    init row, the random point and the near-MAP point (or the stored MAP) of every such problem."""
    n = 0
    for name in lc.PROBLEMS:
        P = lc.problem(name)
        if P['kw']['outlier_mode']:
            continue
        th, sets = lc.points(name)
        for i in sorted({0, len(th) - 6, len(th) - 5}):
            lp, lp_abs, g, gabs = series_logp(th[i], P['A'], P['L'], P['Z'], P['w'], pos=P['pos'], **P['kw'])
            kw = {k: v for k, v in P['kw'].items() if k not in lc.SO_KW}
            lp0, g0, _ = series_hessian(th[i], P['A'], P['L'], P['Z'], P['w'], pos=P['pos'], **kw)
            assert abs(lp - lp0) <= 1e-13 * lp_abs, (name, i)
            assert np.all(np.abs(g - g0) <= 1e-13 * gabs), (name, i, float(np.max(np.abs(g - g0) / gabs)))
            n += 1
    assert n >= 30


# ---- the references' own ratios ------------------------------------------------------------------------------------------------------
_measured = {}


def measure():
    """{point set: {class: worst logp_mismatch of the oracle, the float64 statement and the reversed float64 statement against the
    longdouble statement}} over every problem, point and Jacobian setting of tests/logp_cases.py; also asserts the coverage: every
    point has a finite reference lp and gabs > 0 in every component."""
    if _measured:
        return _measured
    seen = 0
    for name in lc.PROBLEMS:
        P = lc.problem(name)
        om = lc.oracle_model(name)
        th, sets = lc.points(name)
        assert lc.has_outlier_model(name) == bool(P['kw']['outlier_mode'])
        assert om.D == th.shape[1] and len(sets) == len(th) == (5 if name in lc.KAT else 19)
        for jac in (False, True):
            for y, s, ref in zip(th, sets, lc.references(name, jac)):
                assert np.isfinite(float(ref['lp'])) and np.isfinite(float(ref['lp_abs'])), (name, s)
                assert np.all(np.isfinite(ref['g'].astype(float))) and np.all(ref['gabs'] > 0), (name, s)
                assert sum(sl.stop - sl.start for sl in ref['slices'].values()) == om.D      # no component outside the classes
                cands = [om.logp_grad(y, jac)]
                for rev in (False, True):
                    r = reference(P, y, jac, dtype=float, reverse=rev)
                    cands.append((r['lp'], r['g']))
                for lp, g in cands:
                    for k, v in logp_mismatch(lp, g, ref).items():
                        row = _measured.setdefault(s, {})
                        row[k] = max(row.get(k, 0.0), v)
                seen += 1
    assert seen == 2 * sum(len(lc.points(n)[0]) for n in lc.PROBLEMS)
    return _measured


def test_recorded_reference_ratios_are_the_measured_ones():
    m = measure()
    assert set(m) == set(REF) == set(lc.POINT_SETS)
    for s, row in m.items():
        assert set(row) == set(REF[s]), s
        print(s, {k: '%.2e' % v for k, v in row.items()})
        for k, v in row.items():
            assert v <= REF[s][k] <= 4 * v, (s, k, v, REF[s][k])
            assert 8 * REF[s][k] <= 1e-12, (s, k)


def test_every_class_of_every_point_set_has_a_tolerance():
    """'so' with an outlier model only (the stored fits of this family have none); every other class everywhere."""
    for s in lc.POINT_SETS:
        want = set(CLASSES) | {'lp'}
        if s == 'map':
            want.discard('so')
        assert set(REF[s]) == want, s
    for case in lc.CASES:
        assert case[1] in lc.PROBLEMS and case[4] in ('tile', 'few', 'solo', 'wave')
        rows = case[5]
        assert rows is None or max(rows) < len(lc.points(case[1])[0])


# ---- what reading L as Toeplitz costs ------------------------------------------------------------------------------------------------
READING_COST = 16                                # x the tolerance; see the test


def test_what_one_number_per_diagonal_of_L_costs_against_L_as_constructed():
    """The cases hand every reader an exactly Toeplitz L (lc.exactly_toeplitz) because the library's structured L path keeps one
    number per diagonal of an L whose diagonals are constant to 1e-12 of its largest entry (csrc/bdrt_model.hip), the middle row's.
    What that costs at the L the constructors and the goldens hold, on the CPU, longdouble statement against longdouble statement:
      the diagonals within the band vary by at most 1e-13 of the largest entry (measured: 9e-15 .. 4.2e-14), a tenth of what is admitted;
      R, I, err, so do not move at all (L enters the prior alone);
      x, ups, d and lp move by up to READING_COST tolerances (measured: lp 0.33, d 4.3, x 7.5, ups 10.6, the largest at 82 x 162).
    That is beyond what the kernels are held to, and it is the price of the admission, not of any kernel: a reader of every entry
    (dense-L tile, streamed evaluator) pays nothing, every structured reader pays the same.  The bound is not a rounding bound; it
    states the measured cost with a margin of 1.5 so that a constructor or an admission that makes it grow is seen."""
    worst = {}
    for name in lc.PROBLEMS:
        P0, P = lc.problem(name, True), lc.problem(name)
        sets = lc.points(name)[1]
        for L0, L in zip(P0['L'], P['L']):
            assert np.max(np.abs(L - L0)) <= 1e-13 * np.max(np.abs(L0)), name
            assert np.array_equal(L, lc.exactly_toeplitz(L))                                  # (a fixed point: diagonals constant)
        for jac in (False, True):
            for i, (a, b) in enumerate(zip(lc.references(name, jac), lc.references(name, jac, True))):
                for cls, v in logp_mismatch(a['lp'], a['g'], b).items():
                    r = v / tol(sets[i], cls, P['nf'], P['K'])
                    if r > worst.get(cls, (0.0,))[0]:
                        worst[cls] = (r, name, sets[i])
    print({k: '%.2f (%s, %s)' % v for k, v in worst.items()})
    assert set(worst) <= {'lp', 'x', 'ups', 'd'}
    assert all(v[0] <= READING_COST for v in worst.values()), worst
    assert worst['ups'][0] > 1 and worst['x'][0] > 1                                          # (why the cases do not use L as constructed)


# ---- the criterion ---------------------------------------------------------------------------------------------------------------------
def _oracle_at(name, i, jac=False):
    P = lc.problem(name)
    th, sets = lc.points(name)
    lp, g = lc.oracle_model(name).logp_grad(th[i], jac)
    return P, th[i], sets[i], lp, g, lc.references(name, jac)[i]


def test_the_criterion_has_teeth():
    """Mutations of the ORACLE's gradient, one each.  The first four pass the normwise criterion; every one fails logp_mismatch
    against tol, and only in its own class."""
    P, y, s, lp, g, ref = _oracle_at('hs33x90', 13)                        # the random point of 33 x 90
    nf, K = P['nf'], P['K']
    sl = ref['slices']
    assert s == 'random' and not failures(logp_mismatch(lp, g, ref), s, nf, K)

    def mutated(g, j, rel):
        out = g.copy(); out[j] *= 1 + rel
        return out
    j_err = sl['err'].start + int(np.argmin(np.abs(g[sl['err']])))
    for cls, j in (('R', 0), ('I', 1), ('err', j_err)):
        gm = mutated(g, j, 1e-7)
        assert old_criterion(lp, gm, lp, g), cls
        bad = failures(logp_mismatch(lp, gm, ref), s, nf, K)
        print(cls, {k: '%.1e of %.1e' % v for k, v in bad.items()})
        assert set(bad) == {cls}
    # one frequency's likelihood term missing from one x component: the term, from the float64 statement, taken off the oracle's
    f64 = reference(P, y, False, dtype=float)
    full = reference(P, y, False)
    n_, k_ = nf // 2, int(np.argmax(np.abs(np.asarray(P['A'][nf // 2], dtype=float)) * np.exp(y[sl['x']]) / ref['gabs'][sl['x']].astype(float)))
    delta = reference(P, y, False, dtype=float, drop=(n_, k_))['g'] - f64['g']
    assert np.count_nonzero(delta) == 1 and delta[sl['x'].start + k_] != 0
    bad = failures(logp_mismatch(lp, g + delta, full), s, nf, K)
    print('dropped term', {k: '%.1e of %.1e' % v for k, v in bad.items()})
    assert set(bad) == {'x'}
    # one ups component at the near-MAP point
    P, y, s, lp, g, ref = _oracle_at('hs33x90', 14)
    sl = ref['slices']
    assert s == 'near_map' and not failures(logp_mismatch(lp, g, ref), s, nf, K)
    gu = np.abs(g[sl['ups']])
    assert np.max(gu) <= 3.0 and np.max(np.abs(g)) >= 5e3                  # the whole block is small beside the largest component
    small = gu * 1e-6 <= 0.5e-10 * np.max(np.abs(g))                       # (an error the normwise criterion cannot see)
    j = sl['ups'].start + int(np.argmax(np.where(small, gu / ref['gabs'][sl['ups']].astype(float), 0.0)))
    gm = mutated(g, j, 1e-6)
    assert old_criterion(lp, gm, lp, g)
    bad = failures(logp_mismatch(lp, gm, ref), s, nf, K)
    print('ups', {k: '%.1e of %.1e' % v for k, v in bad.items()})
    assert set(bad) == {'ups'}
    # one outlier parameter, both outlier models
    for name in ('dat_sample_K81_so1', 'lu33x47_so2'):
        P, y, s, lp, g, ref = _oracle_at(name, 13)
        sl = ref['slices']
        assert not failures(logp_mismatch(lp, g, ref), s, P['nf'], P['K'])
        j = sl['so'].start + int(np.argmax(np.abs(g[sl['so']]) / ref['gabs'][sl['so']].astype(float)))
        bad = failures(logp_mismatch(lp, mutated(g, j, 1e-6), ref), s, P['nf'], P['K'])
        print('so', name, {k: '%.1e of %.1e' % v for k, v in bad.items()})
        assert set(bad) == {'so'}
    # a non-finite value is never within a tolerance
    gm = g.copy(); gm[0] = np.nan
    assert logp_mismatch(lp, gm, ref)['R'] == np.inf and logp_mismatch(np.inf, g, ref)['lp'] == np.inf


if __name__ == '__main__':
    for s, row in measure().items():
        print("    '%s': {%s}," % (s, ', '.join("'%s': %.1e" % (k, float('%.2g' % (1.5 * row[k]))) for k in ('lp',) + CLASSES if k in row)))
        print('      measured', {k: '%.2e' % v for k, v in row.items()})
