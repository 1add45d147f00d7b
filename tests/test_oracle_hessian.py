"""CPU tests of the closed-form Hessian's numpy statement (tests/hessian_numpy.py): against central differences of the ORACLE's
gradient (the formulas the HIP kernels of csrc/bdrt_newton_hess.h restate; the GPU test holds those to this file's function), and of
the criterion the GPU test applies, hessian_mismatch, with the tolerances below.

Why per block.  The largest entry of H is a q-prior entry (4e5 .. 1.4e6 at the K = 161 points); the entries of the one dense product,
x-x beyond the prior's band, are 1e-8 .. 3e-10 of it, and whole columns of them 4e-13 .. 1e-14: `max |dH| <= 1e-11 max |H|` passes with
a column of the product missing (test_the_criterion_has_teeth shows both facts).  So every block of index classes is held to its own
largest entry, the dense product column by column and entry by entry, the diagonal entry by entry.

Tolerances (TOL, TOL_COL, babs_tol).  They come from the reference's own rounding error, never from the kernel's output: the numpy
statement in float64 against the same statement in np.longdouble (x87 extended, 64-bit mantissa) from the float64 inputs converted,
at every point the GPU test uses (reference_points(); the product's matrices replaced by the oracle's, equal to ~1e-13) -- 38
evaluations, `python -m tests.test_oracle_hessian 192` prints them.  A check whose float64-vs-longdouble ratio exceeds 1e-12 somewhere
gets 8 x that ratio (the 8: the kernel's other summation order, nf split over up to 8 groups), every other check the project's 1e-11.
Worst measured ratios:
  x-d 1.4e-13 (the near-MAP points of 48 x 190, 40 x 192 and 33 x 192), diag 4.9e-14, I-I 4.1e-14, x-ups 3.1e-14, R-I 7.4e-15,
  R-R 6.9e-15, R-x 3.5e-15, ups-d 3.2e-15, ups-ups 3.0e-15, I-err 2.9e-15, I-x 1.9e-15, R-err 1.9e-15, x-err 1.5e-15,
  err-err 8.0e-16, x-x 6.9e-16, d-d 3.5e-16; R-ups, R-d, I-ups, I-d, err-ups, err-d are identically zero in both.
None exceeds 1e-12, so every block and the diagonal are held to 1e-11 (TOL stays empty).  The per-column off-band ratio is held to
1e-9; the reference's own is at most 3.1e-14 (< 1e-10 is required of every point).  The entrywise off-band ratio against Babs is
held to 8 max(3.4e-15, nf 2.2e-16) (measured: 3.3e-15): 2.7e-14 at nf = 7, 1.4e-13 at nf = 81.

Largest admitted width: K = 192 (D = 393; the problem constructor's K <= NG * UK, asserted on the GPU at nf = 33 by
tests/test_gpu_hessian.py::K_ADMITTED): beyond it L leaves the banded path and there is no closed form, so the
shapes asked for at K = 260 and K ~ 350 (one thread group per tile, NH = 320 / 384) are run at the nearest admitted width instead (tests/hessian_shapes.py).

The held mask.  test_no_held_coefficient_sits_on_a_knife_edge states its margin on the gradient in the coordinates of the linear
scale, |g_z[k]| >= 1e-6 max |g_z|.  Stated on g_y it cannot hold anywhere: a coefficient at the floor has g_y[k] = x_k g_z[k] with
x_k = 1e-16 max(x), 1e-21 of the largest |g_y| at these points, whatever the construction."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hessian_shapes as hs
from tests.helpers import load
from tests.hessian_numpy import CLASSES, OFFBAND, class_slices, hessian_mismatch, series_hessian

TOL_DEFAULT = 1e-11                  # per block of index classes and per diagonal entry
TOL = {}                             # checks whose own float64 rounding error exceeds 1e-12: 8 x the measured ratio
TOL_COL = 1e-9                       # x-x off-band, per column
BABS_MEASURED = 3.4e-15                # worst float64-vs-longdouble |dH| / Babs over reference_points()


def babs_tol(nf):
    return 8 * max(BABS_MEASURED, nf * 2.2e-16)


def tolerances(nf):
    keys = ['%s-%s' % (a, b) for i, a in enumerate(CLASSES) for b in CLASSES[i:]] + ['diag']
    tol = {k: TOL.get(k, TOL_DEFAULT) for k in keys}
    tol['xx_offband_col'] = TOL_COL
    tol['xx_offband_abs'] = babs_tol(nf)
    return tol


def failures(mm, nf):
    """the checks of hessian_mismatch's result that exceed their tolerance: {check: (ratio, tolerance)}"""
    tol = tolerances(nf)
    return {k: (v, tol[k]) for k, v in mm.items() if not v <= tol[k]}


def old_criterion(H, Href):
    return np.max(np.abs(H - Href)) <= 1e-11 * np.max(np.abs(Href))


# ---- the points --------------------------------------------------------------------------------------------------------------
DAT_CASES = [('dat_optimize_2ZARC_uniform_0.25_K81', True), ('dat_optimize_2ZARC_uniform_0.25_K161', True),
             ('dat_optimize_2ZARC_uniform_0.25_K101', False), ('dat_sample_2ZARC_uniform_0.25_K161', True)]


def dat_problem(name, pos, spec=0):
    d = load(name)
    return dict(A=d['A'], L=(d['L0'], d['L1'], d['L2']), Z=d['Z'] * (1.0 + 0.1 * spec), w=2 * np.pi * d['freq'], pos=pos, K=d['A'].shape[1],
                nf=len(d['freq']), kw=dict(sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']), ups_beta=float(d['ups_beta']),
                                           induc_scale=float(d['induc_scale'])))


def dat_points(D):
    """the two points of the GPU test's golden-file cases: spectrum 0 and spectrum 2, drawn one after the other"""
    rs = np.random.RandomState(5)
    return [(spec, np.ascontiguousarray(rs.uniform(-1.5, 1.5, D))) for spec in (0, 2)]


def _orc_A(f, part, tau, eps):
    return orc.construct_A(f, part, tau=tau, epsilon=eps)


def _orc_L(bf, tau, eps, order):
    return orc.construct_L(tau, eps, order)


_shape_cache = {}


def shape_problem(nf, K, pos, irregular, construct_A=_orc_A, construct_L=_orc_L):
    key = (nf, K, pos, irregular, construct_A)
    if key not in _shape_cache:
        A, L, Z, f = hs.make_shape(nf, K, irregular, construct_A, construct_L)
        _shape_cache[key] = dict(A=A, L=L, Z=Z, w=2 * np.pi * f, f=f, pos=pos, K=K, nf=nf, kw=dict(hs.KW))
    return _shape_cache[key]


def statement(P, y, lin=False, parts=False, dtype=float):
    return series_hessian(y, P['A'], P['L'], P['Z'], P['w'], pos=P['pos'], lin=lin, parts=parts, dtype=dtype, **P['kw'])


def reference_points(extra_K=(), cheap=False):
    """(label, problem, y, lin) of every evaluation the GPU test compares (cheap: the ones with K <= 101)"""
    for name, pos in DAT_CASES:
        for spec, y in dat_points(2 * dat_problem(name, pos)['K'] + 9):
            P = dat_problem(name, pos, spec)
            if cheap and P['K'] > 101:
                continue
            for lin in ((False, True) if pos else (False,)):
                yield '%s spec %d' % (name, spec), P, y, lin
    # the general-grid test's problem and point (37 irregular frequencies x 61; the point follows the spectrum in its random stream)
    P = shape_problem(37, 61, True, True)
    rs = np.random.RandomState(3)
    rs.uniform(size=37); rs.normal(size=2 * 37)
    y = np.ascontiguousarray(rs.uniform(-1, 1, 2 * 61 + 9))
    for lin in (False, True):
        yield '37 x 61 irregular', P, y, lin
    shapes = list(hs.SHAPES.values()) + [(33, K, True, False) for K in extra_K]
    for nf, K, pos, irr in shapes:
        if cheap and K > 101:
            continue
        P = shape_problem(nf, K, pos, irr)
        for pname, y in (('random', hs.random_point(2 * K + 9)), ('near-MAP', hs.near_map_point(K, pos))):
            for lin in ((False, True) if pos else (False,)):
                yield '%d x %d%s %s' % (nf, K, ' irregular' if irr else '', pname), P, y, lin


def self_error(P, y, lin):
    """hessian_mismatch of the float64 statement against the longdouble one"""
    ld = np.longdouble
    out64 = statement(P, y, lin, parts=True)
    outld = statement(P, y.astype(ld), lin, parts=True, dtype=ld)
    if lin:
        assert np.array_equal(out64[3], outld[3])
    return hessian_mismatch(out64[2], outld[2], P['K'], parts=outld[-2:])


def test_the_float64_statement_is_accurate_to_a_fraction_of_the_tolerances():
    """The cheaper half of the measurement behind TOL (K <= 101), repeated: the statement's own rounding error is at most half of
    every tolerance (an eighth, where the tolerance was derived from it at these points), and below 1e-10 per off-band column."""
    assert np.finfo(np.longdouble).nmant >= 63
    for label, P, y, lin in reference_points(cheap=True):
        mm = self_error(P, y, lin)
        tol = tolerances(P['nf'])
        print(label, 'lin', int(lin), {k: '%.1e' % v for k, v in mm.items() if v > 1e-13})
        assert mm['xx_offband_col'] < 1e-10, (label, lin, mm['xx_offband_col'])
        for k, v in mm.items():
            assert v <= 0.5 * tol[k], (label, lin, k, v, tol[k])


# ---- the statement against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,pos', [('dat_optimize_2ZARC_uniform_0.25_K81', True), ('dat_optimize_2ZARC_uniform_0.25_K81', False),
                                      ('dat_sample_2ZARC_uniform_0.25_K81', True)])
def test_numpy_hessian_equals_central_differences_of_the_oracle_gradient(name, pos):
    d = load(name)
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=pos)
    kw = dict(sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']), ups_beta=float(d['ups_beta']))
    om = orc.OracleModel([blk], d['Z'], d['freq'], **kw)
    D = om.D
    y = np.random.RandomState(4).uniform(-1, 1, D)
    lp0, g0 = om.logp_grad(y, False)
    lp, g, H = series_hessian(y, d['A'], (d['L0'], d['L1'], d['L2']), d['Z'], 2 * np.pi * d['freq'], pos=pos, **kw)
    assert abs(lp - lp0) <= 1e-10 * max(1.0, abs(lp0))
    assert np.max(np.abs(g - g0)) <= 1e-12 * np.max(np.abs(g0))
    Hfd = np.zeros((D, D))
    for j in range(D):
        h = 1e-6 * max(1.0, abs(y[j]))
        yp, ym = y.copy(), y.copy()
        yp[j] += h; ym[j] -= h
        Hfd[j] = (om.logp_grad(yp, False)[1] - om.logp_grad(ym, False)[1]) / (2 * h)
    Hfd = 0.5 * (Hfd + Hfd.T)
    assert np.max(np.abs(H - H.T)) <= 1e-12 * np.max(np.abs(H))
    assert np.max(np.abs(H - Hfd)) <= 1e-8 * np.max(np.abs(Hfd))


def test_numpy_hessian_on_the_linear_scale_equals_central_differences_of_the_oracle_gradient():
    """lin=True: differences in the coordinates z (x itself for the coefficients, y elsewhere).  x_k is stepped by +-h x_k, that is
    y_k = log(x_k +- h x_k); the gradient in z is g_y / x on the coefficients.  No coefficient is held at this point.  Each block
    of index classes to 1e-8 of ITS largest entry.

    The step.  The small blocks (R-x, I-x, x-err: entries of 0.1 .. 10) are differences of a gradient whose components reach 4e4,
    known to 1e-16 of that: one central difference of step h carries 4e-12 / h of rounding noise, 4e-6 at the h = 1e-6 of the test
    above -- enough under its global bound, 1e-5 of these blocks.  So two central differences, of steps h and 2 h, combined to
    cancel the h^2 term, (4 D_h - D_2h) / 3, at h = 3e-3: noise 2e-9, truncation O(h^4)."""
    name = 'dat_optimize_2ZARC_uniform_0.25_K81'
    d = load(name)
    K = d['A'].shape[1]
    blk = dict(A=d['A'], L0=d['L0'], L1=d['L1'], L2=d['L2'], nonneg=True)
    kw = dict(sigma_min=float(d['sigma_min']), ups_alpha=float(d['ups_alpha']), ups_beta=float(d['ups_beta']))
    om = orc.OracleModel([blk], d['Z'], d['freq'], **kw)
    D = om.D
    sx = slice(2, 2 + K)
    y = np.random.RandomState(4).uniform(-1, 1, D)
    lp, g, H, held = series_hessian(y, d['A'], (d['L0'], d['L1'], d['L2']), d['Z'], 2 * np.pi * d['freq'], pos=True, lin=True, **kw)
    assert not held.any()

    def g_z(yy):
        gz = om.logp_grad(yy, False)[1].copy()
        gz[sx] /= np.exp(yy[sx])
        return gz

    def central(j, h):
        yp, ym = y.copy(), y.copy()
        if 2 <= j < 2 + K:
            xj = np.exp(y[j])
            yp[j] = np.log(xj + h * xj); ym[j] = np.log(xj - h * xj)
            dz = np.exp(yp[j]) - np.exp(ym[j])
        else:
            hj = h * max(1.0, abs(y[j]))
            yp[j] += hj; ym[j] -= hj
            dz = yp[j] - ym[j]
        return (g_z(yp) - g_z(ym)) / dz
    h = 3e-3
    Hfd = np.array([(4.0 * central(j, h) - central(j, 2 * h)) / 3.0 for j in range(D)])
    Hfd = 0.5 * (Hfd + Hfd.T)
    assert np.max(np.abs(H - H.T)) <= 1e-12 * np.max(np.abs(H))
    sl = class_slices(K)
    for i, a in enumerate(CLASSES):
        for b in CLASSES[i:]:
            blk_fd = Hfd[sl[a], sl[b]]
            assert np.max(np.abs(H[sl[a], sl[b]] - blk_fd)) <= 1e-8 * np.max(np.abs(blk_fd)), (a, b)


# ---- the held mask ---------------------------------------------------------------------------------------------------------------
def held_margin(P, y):
    """(coefficients at the floor, held mask, margin) of the reference at a point of a pos=True problem.  margin: the smallest
    |g_z[k]| of a coefficient at the floor over the largest |g_z| of all coordinates, g_z the gradient in the coordinates of the
    linear scale (g_y / x on the coefficients, g_y elsewhere).  On the log scale the same quantity is x_k g_z[k] with x_k = 1e-16
    max(x): no point can keep THAT above 1e-6 of the largest |g_y| (it is 1e-21 at the points here), and the kernel's rule only
    reads its sign, which it shares with g_z[k]; what decides whether the sign is safe is how far g_z[k] is from zero."""
    K = P['K']
    sx = slice(2, 2 + K)
    lp, g, H, held = statement(P, y, lin=True)
    x = np.exp(y[sx])
    at_floor = x <= 2 * (1e-14 * np.max(x))
    gz = g.copy(); gz[sx] /= x
    return at_floor, held[sx], (np.min(np.abs(gz[sx][at_floor])) / np.max(np.abs(gz)) if at_floor.any() else np.inf)


def test_no_held_coefficient_sits_on_a_knife_edge():
    """At the near-MAP point of every shape (and of the K = 81 golden problem) some coefficients are at the floor, and each of
    them has a gradient component at least 1e-6 of the largest: HIP's gradient and numpy's cannot disagree about a sign.  The
    random points have no coefficient at the floor."""
    mixed = 0
    cases = [(n, dat_problem('dat_optimize_2ZARC_uniform_0.25_K81', True)) for n in ['K81']]
    cases += [(k, shape_problem(*s)) for k, s in hs.SHAPES.items() if s[2]]
    for label, P in cases:
        at_floor, held, margin = held_margin(P, hs.near_map_point(P['K'], True))
        print(label, 'at the floor', at_floor.sum(), 'held', held.sum(), 'margin %.2e' % margin)
        assert at_floor.sum() >= P['K'] // 4 and not held[~at_floor].any()
        assert margin >= 1e-6, (label, margin)
        mixed += 0 < held.sum() < at_floor.sum()
        at_floor, held, _ = held_margin(P, hs.random_point(2 * P['K'] + 9))
        assert not at_floor.any() and not held.any()
    assert mixed >= 2            # held and not held among the coefficients at the floor of one point


# ---- the criterion -----------------------------------------------------------------------------------------------------------------
def test_the_criterion_has_teeth():
    """Mutations of the statement's own H at the K = 161 points of the GPU test: each exceeds a tolerance of hessian_mismatch.
    Under the criterion the GPU test used to apply alone, max |dH| <= 1e-11 max |H|:
      a column of the dense product missing (the one with the smallest off-band entries: 3.9e-13 of max |H|)      passes;
      every entry of the dense product wrong by 0.1 % (the dat_sample point: the product is 4e-10 of max |H|)      passes;
      columns 100 .. 127 of the product missing                                                                     is caught: those
    columns reach 1.6e-8 of max |H| at the dat_optimize point (4e-10 at the dat_sample point), not below 1e-11 as was hoped when
    this test was asked for -- asserted as measured."""
    P = dat_problem('dat_optimize_2ZARC_uniform_0.25_K161', True)
    K, nf = P['K'], P['nf']
    sx = slice(2, 2 + K)
    y = dat_points(2 * K + 9)[0][1]
    lp, g, Href, lik, Babs = statement(P, y, parts=True)
    parts = (lik, Babs)
    assert not failures(hessian_mismatch(Href, Href, K, parts), nf)
    s = np.exp(y[sx])                                    # (log scale: rows and columns of x carry the factor x)
    Hlik = s[:, None] * lik * s[None, :]
    m = np.arange(K)
    off = np.abs(m[:, None] - m[None, :]) > OFFBAND

    def without_product_columns(cols):
        H = Href.copy()
        for j in cols:
            H[2 + j, sx] -= Hlik[j]; H[sx, 2 + j] -= Hlik[:, j]
            H[2 + j, 2 + j] += Hlik[j, j]
        return H
    j_small = int(np.argmin(np.max(np.where(off, np.abs(Hlik), 0.0), axis=0)))
    H1 = without_product_columns([j_small])
    H2 = without_product_columns(range(100, 128))
    assert old_criterion(H1, Href) and not old_criterion(H2, Href)
    for H in (H1, H2):
        bad = failures(hessian_mismatch(H, Href, K, parts), nf)
        assert 'xx_offband_col' in bad and 'xx_offband_abs' in bad and bad['xx_offband_col'][0] >= 0.99
    H3 = Href.copy(); H3[0, sx] *= 1 + 1e-6; H3[sx, 0] *= 1 + 1e-6
    assert 'R-x' in failures(hessian_mismatch(H3, Href, K, parts), nf)
    su = np.arange(6 + K, 6 + 2 * K - 2)
    H4 = Href.copy(); H4[su, su + 2] *= 1 + 1e-6; H4[su + 2, su] *= 1 + 1e-6
    assert np.all(Href[su, su + 2] != 0)
    assert 'ups-ups' in failures(hessian_mismatch(H4, Href, K, parts), nf)
    Ps = dat_problem('dat_sample_2ZARC_uniform_0.25_K161', True)
    lp, g, Hs, lik_s, Babs_s = statement(Ps, y, parts=True)
    H5 = Hs + 1e-3 * np.pad(s[:, None] * lik_s * s[None, :], ((2, K + 7), (2, K + 7)))
    assert old_criterion(H5, Hs)
    bad = failures(hessian_mismatch(H5, Hs, K, (lik_s, Babs_s)), Ps['nf'])
    assert 'xx_offband_col' in bad and 'xx_offband_abs' in bad
    # one held coefficient released: the near-MAP point on the linear scale
    y = hs.near_map_point(K, True)
    lp, g, Href, held, lik, Babs = statement(P, y, lin=True, parts=True)
    k = int(np.argmax(held[sx]))
    assert held[2 + k]
    Hflip = series_hessian(y, P['A'], P['L'], P['Z'], P['w'], pos=True, lin=True, flip_held=k, **P['kw'])[2]
    assert Hflip[2 + k, 2 + k] != -1.0
    assert failures(hessian_mismatch(Hflip, Href, K, (lik, Babs)), nf)


if __name__ == '__main__':
    import sys
    worst = {}
    for label, P, y, lin in reference_points(extra_K=[int(a) for a in sys.argv[1:]]):
        mm = self_error(P, y, lin)
        for k, v in mm.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print('%-60s lin %d  %s' % (label, lin, {k: '%.1e' % v for k, v in mm.items() if v > 1e-13}), flush=True)
    for k, v in sorted(worst.items(), key=lambda kv: -kv[1]):
        print('  %-16s %.2e' % (k, v))
