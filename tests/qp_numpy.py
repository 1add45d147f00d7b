"""The box-QP solver's linear algebra stated plainly in numpy -- the KKT matrix and the regularisation ladder of csrc/bdrt_qp.hip
(qp_factor), written from the comments of include/bdrt.h (bdrt_debug_qp_factor_solve), with LAPACK as the verdict on each rung -- and
the rounding measures of the Gram entries (bdrt_gram, bdrt_gram_batch).  The factor's and the solves' measures are those of
tests/newton_numpy.py (gamma, factor_omega, factor_bound_omega, solve_ratio, rung_margin_ok), used as they are: the QP's factor is
n x n with no padding, so nothing is unpacked and nothing is padded here.  Shared by tests/test_qp_linear_algebra_host.py (LAPACK and
numpy through the measures, no GPU) and tests/test_gpu_qp_linear_algebra.py (the kernels).  Test infrastructure, not the product.

  KKT      M = (P + P^T) / 2 + diag(dg + reg), P not necessarily symmetric
  ladder   reg = 0, then 1e-14 (1 + |M(0,0)|) with M(0,0) of reg = 0, then x 100 per rung while reg <= 1e6: the first rung with a
           Cholesky factor is committed
  Gram     P = A^T A + L2, q = -A^T z + L1; of bdrt_gram_batch with A <- fl(w[:, None] * A), z <- fl(w * t)"""
import numpy as np

from tests import newton_numpy as nn

LD = np.longdouble
REG_MAX = 1e6


# ---- the statement ----------------------------------------------------------------------------------------------------------

def kkt(P, dg, reg=0.0):
    """sym(P) + diag(dg + reg), every operation one float64 operation in the order the kernel states it"""
    P = np.asarray(P, dtype=float)
    M = 0.5 * (P + P.T)
    i = np.arange(len(M))
    M[i, i] = M[i, i] + (np.asarray(dg, dtype=float) + float(reg))
    return M


def regs(m00):
    """the ladder's values: 0, then 1e-14 (1 + |m00|) and its multiples by 100 up to 1e6"""
    out = [0.0]
    reg = 1e-14 * (1.0 + abs(float(m00)))
    while reg <= REG_MAX:
        out.append(reg)
        reg = reg * 100.0
    return out, reg           # (reg: the first value beyond the ladder, what a refused problem reports)


def ladder(P, dg):
    """dict(ok, rung, rungs, reg, refused, M, L): the first rung that LAPACK factors.  rung: its index (0: reg = 0), rungs: the
    factorisations tried, refused: the regs that did not factor.  ok False: none did; reg is then the first value beyond 1e6 (NaN
    for a non-finite M(0,0))."""
    m00 = kkt(P, dg)[0, 0]
    if not np.isfinite(m00):
        return dict(ok=False, rung=None, rungs=1, reg=np.nan, refused=[0.0], M=None, L=None)
    vals, beyond = regs(m00)
    refused = []
    for j, reg in enumerate(vals):
        M = kkt(P, dg, reg)
        L = nn.lapack_factor(M) if np.all(np.isfinite(M)) else None
        if L is not None:
            return dict(ok=True, rung=j, rungs=j + 1, reg=reg, refused=refused, M=M, L=L)
        refused.append(reg)
    return dict(ok=False, rung=None, rungs=len(vals), reg=beyond, refused=refused, M=None, L=None)


def rung_margin_ok(P, dg, reg, accepted):
    """newton_numpy.rung_margin_ok on M = sym(P) + diag(dg) + reg I (its H is -M at reg = 0, its damping reg)"""
    return nn.rung_margin_ok(-kkt(P, dg), reg, len(dg), accepted)


def pinnable(reg, n, norm2):
    """a rung whose verdict a test may pin: reg beyond 1e3 n gamma_{n+1} |M|_2; below, it lies inside the factorisation's own rounding"""
    return reg > 1e3 * n * nn.gamma(n + 1) * norm2


# ---- the measures -----------------------------------------------------------------------------------------------------------

def pivot_ulps(diag, piv):
    """max |diag^2 - piv| in ulps of piv (the square root: rsq estimate and two Newton steps)"""
    diag, piv = np.asarray(diag, dtype=float), np.asarray(piv, dtype=float)
    return float(np.max(np.abs(diag.astype(LD) ** 2 - piv.astype(LD)) / np.spacing(np.abs(piv)).astype(LD)))


def inverse_column_ratio(M, L, Minv, c, s):
    """the solve for the unit vector e_c against column c of LAPACK's inverse: with r(y) = 2 gamma_{3n+1} |L||L^T||y| the residual bound of
    newton_numpy.solve_ratio, both s and the column x solve M y = e_c to within r(y), so |s - x| <= |M^-1| (r(s) + r(x)) componentwise.
    Returns max |s - x| / that bound."""
    n = len(M)
    x = Minv[:, c]
    r = 2.0 * nn.gamma(3 * n + 1) * (nn.absLLt_s(L, s) + nn.absLLt_s(L, x))
    bound = np.abs(Minv).astype(LD) @ r
    return nn._ratio_max(np.abs(np.asarray(s, dtype=LD) - x.astype(LD)), bound)


def gram_ratio(G, A, L2=None):
    """max |G - (A^T A + L2)| / (gamma_{R+1} (|A|^T |A| + |L2|)), the reference in np.longdouble; R = rows of A"""
    A = np.asarray(A, dtype=float)
    Al = A.astype(LD)
    ref, mag = Al.T @ Al, np.abs(Al).T @ np.abs(Al)
    if L2 is not None:
        ref, mag = ref + np.asarray(L2, dtype=LD), mag + np.abs(np.asarray(L2, dtype=LD))
    return nn._ratio_max(np.abs(np.asarray(G, dtype=LD) - ref), nn.gamma(len(A) + 1) * mag)


def gram_q_ratio(q, A, z, L1=None):
    """max |q - (-A^T z + L1)| / (gamma_{R+1} (|A|^T |z| + |L1|))"""
    A = np.asarray(A, dtype=float)
    Al, zl = A.astype(LD), np.asarray(z, dtype=LD)
    ref, mag = -(Al.T @ zl), np.abs(Al).T @ np.abs(zl)
    if L1 is not None:
        ref, mag = ref + np.asarray(L1, dtype=LD), mag + np.abs(np.asarray(L1, dtype=LD))
    return nn._ratio_max(np.abs(np.asarray(q, dtype=LD) - ref), nn.gamma(len(A) + 1) * mag)


def batch_rows(A, w, t=None):
    """what bdrt_gram_batch states it multiplies for one group: fl(w[:, None] * A) and fl(w * t)"""
    A, w = np.asarray(A, dtype=float), np.asarray(w, dtype=float)
    return w[:, None] * A, (None if t is None else w * np.asarray(t, dtype=float))


# ---- the checks both test files make on one problem's outputs ---------------------------------------------------------------

def check_factor_solve(P, dg, rhs, cols, out, label, expect_rung=None):
    """every bound on one problem's outputs `out` = dict(ok, rungs, reg, L [n, n], piv [n], sol [nrhs, n]) -- the kernel's, or LAPACK's
    through the same door; returns dict(omega, omega_ref, ratio, solve, inverse, rung).  cols: per right-hand side the column its unit
    vector stands for, or None."""
    n = len(dg)
    R = ladder(P, dg)
    assert out['ok'] == 1 and R['ok'], (label, out['ok'], R['ok'])
    vals, _ = regs(kkt(P, dg)[0, 0])
    j = out['rungs'] - 1
    assert 0 <= j < len(vals) and np.float64(out['reg']).tobytes() == np.float64(vals[j]).tobytes(), (label, j, out['reg'])
    for jj in range(j):
        assert rung_margin_ok(P, dg, vals[jj], accepted=False), (label, 'refused rung', jj)
    assert rung_margin_ok(P, dg, vals[j], accepted=True), (label, 'accepted rung', j)
    if expect_rung is not None:
        assert j == expect_rung == R['rung'], (label, j, expect_rung, R['rung'])
    # the factor
    assert n <= nn.LD_MAX_D
    M = kkt(P, dg, out['reg'])
    L = np.asarray(out['L'], dtype=float)
    assert np.all(np.isfinite(L)) and np.array_equal(L, np.tril(L)), label
    omega = nn.factor_omega(M, L)
    Lref = R['L'] if R['rung'] == j else nn.lapack_factor(M)
    assert Lref is not None, label
    omega_ref = nn.factor_omega(M, Lref)
    ratio = omega / omega_ref if omega_ref > 0 else (0.0 if omega == 0 else np.inf)
    assert omega <= nn.factor_bound_omega(n), (label, omega, nn.factor_bound_omega(n))
    pu = pivot_ulps(np.diag(L), out['piv'])
    assert pu <= 4.0, (label, 'pivots', pu)
    # the solves
    worst_solve, worst_inv = 0.0, 0.0
    Minv = None
    for b, c, s in zip(rhs, cols, out['sol']):
        assert np.all(np.isfinite(s)), label
        sr = nn.solve_ratio(M, L, b, s)
        assert sr <= 1.0, (label, 'solve', c, sr)
        worst_solve = max(worst_solve, sr)
        if c is not None:
            if Minv is None:
                Minv = nn.lapack_solve(Lref, np.eye(n))
            ir = inverse_column_ratio(M, L, Minv, c, s)
            assert ir <= 1.0, (label, 'inverse column', c, ir)
            worst_inv = max(worst_inv, ir)
    return dict(omega=omega, omega_ref=omega_ref, ratio=ratio, solve=worst_solve, inverse=worst_inv, rung=j, pivot_ulps=pu)
