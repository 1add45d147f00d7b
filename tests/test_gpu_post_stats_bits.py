"""GPU test (-m gpu) that the post-sampling statistics keep their bits: every output of bdrt_diagnostics, bdrt_rank_diagnostics,
bdrt_debug_rank_z, bdrt_psis_loo, bdrt_pointwise_loglik, bdrt_percentiles and bdrt_summary against the recorded fixture
tests/golden/post_stats_bits.npz, at every shape where one of their kernels takes another path.

The fixture holds what the library answered before the four files were moved onto one shared device header (bdrt_stats.h) and
one host staging path; it holds outputs only.  The inputs are rebuilt here: AR(1) series x_t = phi x_{t-1} + u_t whose
innovations come from a 64-bit integer recurrence in numpy uint64 -- additions and multiplications only, no library random
stream and no libm call, so they do not depend on the numpy version.  Ties are made by rounding to quarters.
BDRT_RECORD_POST_STATS=<file> writes the answers there instead of comparing them.

A failure prints the largest ulp distance of every output that differs: a later change of the ROCm math library (exp, log,
normcdfinv) reads as a drift of a few last bits, a changed summation order or network as much more."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'post_stats_bits.npz')
RECORD = os.environ.get('BDRT_RECORD_POST_STATS')

_MUL = np.uint64(6364136223846793005)
_INC = np.uint64(1442695040888963407)


def _uniform(seed, shape):
    """[-0.5, 0.5) of the given shape: two steps of a 64-bit linear congruential recurrence on seed + index, top 53 bits."""
    n = int(np.prod(shape))
    with np.errstate(over='ignore'):
        s = (np.arange(n, dtype=np.uint64) + np.uint64(seed * 1000003)) * _MUL + _INC
        s = s * _MUL + _INC
        s = (s ^ (s >> np.uint64(29))) * _MUL + _INC
    return ((s >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5).reshape(shape)


def _ar1(seed, n, shape, phi=0.5, scale=1.0, ties=False):
    """[n, *shape]: AR(1) along the first axis, every series started at its first innovation"""
    u = _uniform(seed, (n,) + tuple(shape))
    x = np.empty_like(u)
    x[0] = u[0]
    for t in range(1, n):
        x[t] = phi * x[t - 1] + u[t]
    x = x * scale
    return np.floor(x * 4.0 + 0.5) * 0.25 if ties else x


def _draws(seed, G, M, N, Cn, **kw):
    """[G, M * N, Cn]: every (group, chain, column) its own series over the N draws"""
    x = _ar1(seed, N, (G, M, Cn), **kw)
    return np.ascontiguousarray(x.transpose(1, 2, 0, 3).reshape(G, M * N, Cn))


def _ulps(a, b):
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i).astype(np.float64)
    both = np.isfinite(a) & np.isfinite(b)
    same = both | ((a == b) | (np.isnan(a) & np.isnan(b)))
    if not np.all(same):
        return float('inf')
    return float(np.max(np.abs(key(a[both]) - key(b[both])))) if np.any(both) else 0.0


def _check(case, outs):
    """outs: {name: array} of one case, compared with (or recorded as) the fixture's '<case>/<name>'"""
    outs = {'%s/%s' % (case, k): np.asarray(v) for k, v in outs.items()}
    if RECORD:
        table = dict(np.load(RECORD)) if os.path.exists(RECORD) else {}
        table.update(outs)
        np.savez_compressed(RECORD, **table)
        return
    want = np.load(FIXTURE)
    wrong = []
    for k, got in outs.items():
        ref = want[k]
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        if not np.array_equal(got, ref, equal_nan=got.dtype.kind == 'f'):
            d = _ulps(got, ref) if got.dtype.kind == 'f' else float(np.max(np.abs(got.astype(np.int64) - ref)))
            print('%s: largest distance %g ulp' % (k, d))
            wrong.append(k)
    assert not wrong, wrong


@pytest.fixture(scope='module')
def lib():
    from bayes_drt_amd import _lib
    return _lib.require_gpu()


def _call(lib, name, *args):
    from bayes_drt_amd import _lib
    _lib.check(getattr(lib, name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]), name)


# ------------------------------------------------------------------------------------------------ diag
def _diag_input(shape):
    G, M, N, Cn = shape
    mask = np.zeros(Cn, dtype=np.uint8)
    if shape == (2, 1, 4, 3):                    # the smallest N with an n_eff
        X = _draws(11, G, M, N, Cn)
        X[:, :, 1] = 0.75                        # a constant column
        X[1, 2, 0] = np.nan                      # a column with one NaN
        mask[2] = 1
    elif shape == (2, 2, 5, 9):                  # odd N; a tile of 8 columns and a remainder tile
        X = _draws(12, G, M, N, Cn, ties=True, scale=3.0)
        X[:, :, 5] = -1.25
        X[0, :N, 3] = 1.0                        # constant chains at different values
        X[0, N:, 3] = 2.0
        X[1, 7, 2] = np.nan
        mask[8] = 1
    elif shape == (1, 4, 200, 3):                # phi = 0.95: the pair walk crosses a 64-lag block
        X = _draws(13, G, M, N, Cn, phi=0.95)
        mask[2] = 1
    else:                                        # (1, 8, 1100, 2): 70 400 B > 64 KiB, the streamed instantiation
        X = _draws(14, G, M, N, Cn, phi=0.5)
        mask[1] = 1
    return X, mask


@pytest.mark.parametrize('shape', [(2, 1, 4, 3), (2, 2, 5, 9), (1, 4, 200, 3), (1, 8, 1100, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_diagnostics_bits(lib, shape):
    G, M, N, Cn = shape
    X, mask = _diag_input(shape)
    out = [np.full((G, Cn), -7.0) for _ in range(4)]
    _call(lib, 'bdrt_diagnostics', X, G, M, N, Cn, C.c_long(Cn), mask, *out)
    _check('diag_%dx%dx%dx%d' % shape, dict(zip(('mean', 'sd', 'n_eff', 'rhat'), out)))


# ------------------------------------------------------------------------------------------------ rank
def _rank_input(shape):
    G, M, N, Cn = shape
    mask = np.zeros(Cn, dtype=np.uint8)
    if shape == (2, 1, 2, 2):
        X = _draws(21, G, M, N, Cn)
        mask[1] = 1
    elif shape == (1, 1, 8, 1):
        X = _draws(22, G, M, N, Cn, ties=True, scale=2.0)
    elif shape == (2, 3, 7, 3):                  # S = 18: not a power of two, odd N
        X = _draws(23, G, M, N, Cn, ties=True, scale=3.0)
        X[1, N:2 * N, 0] = 0.5                   # an unmoved chain
        mask[2] = 1
    elif shape == (1, 4, 300, 2):                # S above the thread count
        X = _draws(24, G, M, N, Cn, phi=0.9, ties=True, scale=8.0)
        X[0, :N, 1] = -0.25
        mask[1] = 1
    else:                                        # (1, 4, 2048, 1): S = 8192, the limit
        X = _draws(25, G, M, N, Cn, phi=0.7)
    return X, mask


RANK_SHAPES = [(2, 1, 2, 2), (1, 1, 8, 1), (2, 3, 7, 3), (1, 4, 300, 2), (1, 4, 2048, 1)]


@pytest.mark.parametrize('tail', [(0.05, 0.95), (0.1, 0.6)], ids=['tail05_95', 'tail10_60'])
@pytest.mark.parametrize('shape', RANK_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_rank_diagnostics_bits(lib, shape, tail):
    G, M, N, Cn = shape
    X, mask = _rank_input(shape)
    out = [np.full((G, Cn), -7.0) for _ in range(5)]
    _call(lib, 'bdrt_rank_diagnostics', X, G, M, N, Cn, C.c_long(Cn), mask, C.c_double(tail[0]), C.c_double(tail[1]), *out)
    _check('rank_%dx%dx%dx%d_%g_%g' % (shape + tail), dict(zip(('rhat', 'ess_bulk', 'ess_tail', 'ess_mean', 'sd'), out)))


@pytest.mark.parametrize('is_pos', [0, 1])
def test_rank_z_bits(lib, is_pos):
    G, M, N, Cn = 2, 3, 7, 3
    X, _ = _rank_input((G, M, N, Cn))
    y = np.ascontiguousarray(X[0, :, 1].reshape(M, N))
    outs = {}
    for what in (0, 1, 2):
        z = np.full(2 * M * (N // 2), -7.0)
        _call(lib, 'bdrt_debug_rank_z', y, M, N, is_pos, what, z)
        outs['what%d' % what] = z
    _check('rank_z_pos%d' % is_pos, outs)


# ------------------------------------------------------------------------------------------------ loo
def _loo_input(S):
    N = 3
    x = _ar1(31 + S, S, (N,), phi=0.3, scale=2.0)
    ll = -1.0 - x * x                            # [S, N]
    if S >= 5:
        ll[:, 1] = -2.5                          # an all-equal column
    return np.ascontiguousarray(ll[None])        # [1, S, N]


@pytest.mark.parametrize('with_reff', [False, True], ids=['noreff', 'reff'])
@pytest.mark.parametrize('S', [2, 5, 37, 1000])
def test_psis_loo_bits(lib, S, with_reff):
    N = 3
    ll = _loo_input(S)
    reff = np.array([0.5, 1.0, 0.25]) if with_reff else None
    outs = {}
    for tag, bad in (('', False), ('_nonfinite', True)):
        x = ll.copy()
        if bad:
            x[0, S - 1, 2] = -np.inf             # a non-finite column
        out = [np.full(N, -7.0) for _ in range(4)]
        nt = np.full(N, -7, dtype=np.int32)
        _call(lib, 'bdrt_psis_loo', x, 1, S, N, reff, *out, nt)
        outs.update({k + tag: v for k, v in zip(('lpd', 'elpd_loo', 'pareto_k', 'p_waic'), out)})
        outs['n_tail' + tag] = nt
    _check('loo_%dx3_%s' % (S, 'reff' if with_reff else 'noreff'), outs)


@pytest.mark.parametrize('pair', [0, 1])
def test_pointwise_loglik_bits(lib, pair):
    G, S, N2 = 1, 5, 6
    Zhat = np.ascontiguousarray(_ar1(41, S, (N2,), scale=2.0)[None])
    sig = np.ascontiguousarray((0.5 + _ar1(42, S, (N2,)) ** 2)[None])
    sig[0, 3, 4] = 0.0                           # not a scale: NaN
    z = _uniform(43, (G, N2))
    out = np.full((G, S, N2 // 2 if pair else N2), -7.0)
    _call(lib, 'bdrt_pointwise_loglik', Zhat, sig, z, G, S, N2, pair, out)
    _check('loglik_pair%d' % pair, {'ll': out})


# ------------------------------------------------------------------------------------------------ post
Q = np.array([0.0, 2.5, 50.0, 97.5, 100.0])


@pytest.mark.parametrize('rows,K', [(1, 3), (2, 3), (7, 3), (1000, 3), (16385, 2)], ids=lambda v: str(v))
def test_percentiles_bits(lib, rows, K):
    # 16385 rows: past the 16384 a column may have in LDS, the network runs in HBM
    X = _ar1(50 + rows, rows, (K,), phi=0.6, ties=rows == 7, scale=3.0)
    out = np.full((len(Q), K), -7.0)
    _call(lib, 'bdrt_percentiles', X, rows, K, C.c_long(K), None, 0, None, Q, len(Q), out)
    _check('pct_%dx%d' % (rows, K), {'pct': out})


def test_percentiles_nan_column_bits(lib):
    rows, K = 33, 4
    X = _ar1(61, rows, (K,))
    X[5, 2] = np.nan
    out = np.full((len(Q), K), -7.0)
    _call(lib, 'bdrt_percentiles', X, rows, K, C.c_long(K), None, 0, None, Q, len(Q), out)
    _check('pct_nan', {'pct': out})


def test_projected_percentiles_bits(lib):
    rows, K, M = 33, 5, 17
    X = _ar1(62, rows, (K,))
    Phi = _uniform(63, (M, K)) * 2.0
    bias = _uniform(64, (M,))
    out = np.full((len(Q), M), -7.0)
    _call(lib, 'bdrt_percentiles', X, rows, K, C.c_long(K), Phi, M, bias, Q, len(Q), out)
    _check('pct_projected', {'pct': out})


def test_summary_bits(lib):
    rows, K = 100, 6
    X = _ar1(65, rows, (K,), phi=0.8)
    mask = np.array([0, 1, 0, 0, 1, 0], dtype=np.uint8)
    mean, pct = np.full(K, -7.0), np.full((len(Q), K), -7.0)
    _call(lib, 'bdrt_summary', X, rows, K, C.c_long(K), mask, Q, len(Q), mean, pct)
    _check('summary', {'mean': mean, 'pct': pct})
