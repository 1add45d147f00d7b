"""Inputs of the tests of the box-QP solver's linear algebra and of the Gram entries (tests/test_qp_linear_algebra_host.py on the CPU
with LAPACK and numpy, tests/test_gpu_qp_linear_algebra.py on the GPU with csrc/bdrt_qp.hip's chol_packed / chol_solve_blocked and
csrc/bdrt_ridge.hip's Gram kernels): every size at which the blocked factorisation changes its schedule, KKT-like matrices, planted
eigenvalues for the regularisation ladder, breakdowns at chosen columns, and the Gram shapes.  All seeded.  Test infrastructure, not
the product."""
import functools

import numpy as np

from tests import qp_numpy as qn
from tests.test_gpu_host_owner_bits import _qp_first_n_beyond_lds

N_BEYOND_LDS = _qp_first_n_beyond_lds()      # the first n whose triangle lives in the global work buffer
N_LAST_LDS = N_BEYOND_LDS - 1
# n: what changes there (16-column blocks; a trailing tile is 16 x 16)
SIZES = {
    1: 'one cell', 2: 'one block of two', 15: 'one block, one short', 16: 'one full block, no trailing part',
    17: 'the trailing tile owns one cell', 31: 'two blocks, the last one short', 32: 'two full blocks',
    33: 'three trailing tiles, the last row of tiles owns one row', 48: 'three full blocks', 49: 'six trailing tiles, one-row edge',
    163: 'the ridge problems of the stored fits', N_LAST_LDS: 'the last n in LDS', N_BEYOND_LDS: 'the first n in the global work buffer',
    257: 'more trailing tiles than two trips of the eight waves, one-row edge', 401: 'the largest: global work buffer',
}
KINDS = ('full', 'barrier6', 'barrier12')


def _rs(*key):
    """a generator seeded by the integers of `key`"""
    return np.random.RandomState(sum(1000003 ** i * (int(k) + 1) for i, k in enumerate(key)) % (2 ** 31))


def kkt_case(n, kind):
    """(P, dg): 'full': A^T A + 1e-8 I of A [n + 3, n]; 'barrier6' / 'barrier12': the rank-deficient A^T A of A [n // 2, n] with a barrier
    diagonal 10^U(-6, 6) / 10^U(-12, 12) in dg (the role of z / s)"""
    k = KINDS.index(kind)
    rs = _rs(1, n, k)
    if kind == 'full':
        A = rs.normal(size=(n + 3, n))
        return A.T @ A + 1e-8 * np.eye(n), np.zeros(n)
    span = 6.0 if kind == 'barrier6' else 12.0
    A = rs.normal(size=(n // 2, n))
    return A.T @ A, 10.0 ** rs.uniform(-span, span, n)


def quantised(P, bits=40):
    """P with every entry rounded to `bits` significant bits: P (1 + m) is then exact for small integers m"""
    m, e = np.frexp(np.asarray(P, dtype=float))
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)


def antisymmetric_partner(Pq, n, kind):
    """Pq + S, S = m * Pq above the diagonal and -m * Pq below it with integers m in 1 .. 3 (Pq symmetric, quantised): every entry
    and every sum (Pq + S)_ij + (Pq + S)_ji = 2 Pq_ij is exact, so the symmetrised matrix is Pq bit for bit -- unless the upper
    triangle is read where the lower one belongs or the other way round, when an entry comes out up to 4 times too large or of the
    other sign."""
    rs = _rs(2, n, KINDS.index(kind))
    m = np.triu(rs.randint(1, 4, size=(n, n)).astype(float), 1)
    S = (m - m.T) * Pq
    out = Pq + S
    assert np.array_equal(0.5 * (out + out.T), Pq)
    return out


def rhs_case(n, kind):
    """[nrhs, n] and the columns the unit vectors stand for (None for the others): one random vector, the unit vectors e_0, e_15,
    e_16, e_{n-1} where they exist, one vector whose entries span 1e-8 .. 1e8"""
    rs = _rs(3, n, KINDS.index(kind))
    rows, cols = [rs.normal(size=n)], [None]
    for c in sorted(set(c for c in (0, 15, 16, n - 1) if 0 <= c < n)):
        e = np.zeros(n); e[c] = 1.0
        rows.append(e); cols.append(c)
    rows.append(rs.normal(size=n) * 10.0 ** rs.uniform(-8, 8, n)); cols.append(None)
    return np.ascontiguousarray(np.stack(rows)), cols


# ---- the ladder -------------------------------------------------------------------------------------------------------------

PLANTED_N = (17, 49, N_BEYOND_LDS)


@functools.lru_cache(maxsize=4)
def _planted_basis(n):
    """(q, W): a unit vector q with q[0] = 0 and an orthonormal basis W [n, n - 1] of its complement: the planted eigenvalue then
    leaves M(0,0), and with it the ladder's values, as they are"""
    rs = _rs(4, n)
    Q, _ = np.linalg.qr(rs.normal(size=(n - 1, n - 1)))
    q = np.zeros(n); q[1:] = Q[:, 0]
    B = np.zeros((n, n - 1)); B[0, 0] = 1.0; B[1:, 1:] = Q[:, 1:]
    R, _ = np.linalg.qr(rs.normal(size=(n - 1, n - 1)))
    return q, B @ R


def _planted_matrix(n, lam):
    q, W = _planted_basis(n)
    d = np.linspace(1.0, 4.0, n - 1)
    M = (W * d) @ W.T
    M = 0.5 * (M + M.T)
    return M + lam * np.outer(q, q)                 # (q[0] = 0: row and column 0 are untouched, M(0,0) exactly as without lam)


def planted_rungs(n):
    """the rungs j (index into the ladder's values, 0: reg = 0) at which an eigenvalue can be planted between reg_j and reg_{j+1} and
    the verdict pinned: reg_j beyond qp_numpy.pinnable's threshold for the planted matrix's norm, reg_{j+1} still on the ladder"""
    vals, _ = qn.regs(_planted_matrix(n, 0.0)[0, 0])
    out = []
    for j in range(1, len(vals) - 1):
        lam = np.sqrt(vals[j] * vals[j + 1])
        if qn.pinnable(vals[j], n, max(4.0, lam)):
            out.append(j)
    return out


def planted_case(n, j):
    """(P, dg, lam, expected rung j + 1, its reg): the spectrum 1 .. 4 and the smallest eigenvalue -sqrt(reg_j reg_{j+1})"""
    vals, _ = qn.regs(_planted_matrix(n, 0.0)[0, 0])
    lam = -np.sqrt(vals[j] * vals[j + 1])
    M = _planted_matrix(n, lam)
    assert M[0, 0] == _planted_matrix(n, 0.0)[0, 0]
    return M, np.zeros(n), lam, j + 1, vals[j + 1]


def hopeless_case(n=33):
    """one eigenvalue at -1e7 |M|_2 of the rest: no reg up to 1e6 makes it positive definite"""
    return _planted_matrix(n, -4e7), np.zeros(n)


# ---- breakdown at a chosen column -------------------------------------------------------------------------------------------

BREAK_N = (49, N_BEYOND_LDS)
BREAK_RUNG = 5


def break_columns(n):
    return sorted(set((0, 7, 15, 16, 17, n - 1)))


def _ldl(n, c, dc):
    rs = _rs(5, n)
    L0 = np.eye(n) + np.tril(rs.normal(size=(n, n)) * (0.3 / np.sqrt(n)), -1)
    D = rs.uniform(1.0, 4.0, n)
    D[c] = dc
    M = (L0 * D) @ L0.T
    return 0.5 * (M + M.T)


def breakdown_case(n, c, hopeless):
    """(P, dg, reg values): M = L0 D L0^T with L0 unit lower triangular, D in [1, 4] but D_c: -1e7 (the factorisation breaks down in
    column c at every rung), or -sqrt(reg_5 reg_6) of the matrix's own ladder (c = 0 moves M(0,0): fixed point)"""
    if hopeless:
        M = _ldl(n, c, -1e7)
        return M, np.zeros(n), qn.regs(M[0, 0])[0]
    v = 1e-5
    for _ in range(6):
        M = _ldl(n, c, -v)
        vals, _ = qn.regs(M[0, 0])
        v = np.sqrt(vals[BREAK_RUNG] * vals[BREAK_RUNG + 1])
    M = _ldl(n, c, -v)
    return M, np.zeros(n), qn.regs(M[0, 0])[0]


# ---- non-finite input, batch isolation --------------------------------------------------------------------------------------

NAN_N = 33
NAN_CELLS = ((0, 0), (20, 3), (NAN_N - 1, NAN_N - 1))


def nan_case(cell):
    P, dg = kkt_case(NAN_N, 'full')
    P = P.copy()
    P[cell] = np.nan
    return P, dg


def isolation_case(n=49):
    """[3, n, n], [3, n]: accepted at reg = 0, a planted rung, refused; and the rung of the second"""
    j = planted_rungs(n)[len(planted_rungs(n)) // 2]
    Pa, da = kkt_case(n, 'barrier6')
    Pb, db, _, rung, _ = planted_case(n, j)
    Pc = _planted_matrix(n, -4e7)
    return np.ascontiguousarray(np.stack([Pa, Pb, Pc])), np.ascontiguousarray(np.stack([da, db, np.zeros(n)])), rung


# ---- Gram -------------------------------------------------------------------------------------------------------------------

GRAM_SHAPES = ((1, 1), (3, 17), (4, 16), (5, 16), (7, 33), (2, 163), (81, 5), (162, 163))
GRAM_NG = 3


def gram_case(nrows, n):
    """dict(A [nrows, n] with rows scaled by 10^U(-3, 3), z [nrows], L2 [n, n] symmetric, L1 [n], w [3, nrows] in [1, 2), t [3, nrows])"""
    rs = _rs(6, nrows, n)
    A = rs.normal(size=(nrows, n)) * 10.0 ** rs.uniform(-3, 3, (nrows, 1))
    z = rs.normal(size=nrows) * 10.0 ** rs.uniform(-3, 3, nrows)
    B = rs.normal(size=(n, n))
    return dict(A=np.ascontiguousarray(A), z=z, L2=np.ascontiguousarray(B + B.T), L1=rs.normal(size=n),
                w=np.ascontiguousarray(rs.uniform(1.0, 2.0, (GRAM_NG, nrows))), t=np.ascontiguousarray(rs.normal(size=(GRAM_NG, nrows))))
