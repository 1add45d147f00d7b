"""Problems and points for the tests of the closed-form Hessian (tests/test_oracle_hessian.py on the CPU, tests/test_gpu_hessian.py on
the GPU): the shapes at which csrc/bdrt_newton_hess.h::hess_fill changes how its threads own columns and frequencies, and two points per
shape.  Test infrastructure, not the product.

A shape is built from a constructor pair (construct_A(f, part, tau, epsilon), construct_L(basis_freq, tau, epsilon, order)): the GPU
tests pass the product's (bayes_drt_amd.matrices), the CPU tests the oracle's; grids, spectrum and points are the same for both."""
import numpy as np

# key: (nf, K, pos, irregular frequencies).  hess_fill: a 16-row tile with ncol = min(r0 + 16, Dp) columns, NH = half of ncol rounded
# up to 64, NG = 512 / NH groups share the frequencies.  The closed form needs the banded-Toeplitz L path, which the problem constructor
# gives to K <= 192 only (bdrt_model.hip: K <= NG * UK): D <= 393, Dp <= 400, so NH <= 256 and NG >= 2 in every problem that is
# admitted today -- the one-group regimes NH = 320 .. 512 of wider tiles cannot be reached through the library (hess_analytic_ok
# says "no closed form" there and the iteration differences gradients).
SHAPES = {
    'nf7_K35': (7, 35, True, False),        # D 79 / Dp 80: nf < NG (NG = 8, 4: groups with an empty frequency range); smallest banded shape
    'nf33_K90': (33, 90, True, False),      # D 189 / Dp 192: nf not divisible by NG = 8, 4, 2; a last tile of 13 rows
    'nf48_K190': (48, 190, True, False),    # D 389 / Dp 400: NH = 256, NG = 2 for the tile beyond column 384
    # asked for at 40 x 260 (NH = 320, NG = 1): not admitted (K > 192); the nearest admitted width, NH = 256 and an even nf
    'nf40_K192': (40, 192, True, False),    # D 393 / Dp 400
    # the same width from plain copies of A (irregular frequencies), free coefficients; asked for at 40 x 260 as well
    'nf40_K192_irr': (40, 192, False, True),
}
WIDE = 'nf40_K192'                           # the widest shape: the end-to-end iteration runs here
KW = dict(sigma_min=0.002, ups_alpha=0.05, ups_beta=0.1)


def make_shape(nf, K, irregular, construct_A, construct_L, seed=3):
    """(blk arrays A [2 nf, K], (L0, L1, L2), Z [2 nf], f [nf]) of one synthetic spectrum: K basis functions on a log-uniform grid,
    the frequencies a contiguous run of that grid (A is exactly Toeplitz) or an irregular list of their own."""
    rs = np.random.RandomState(seed)
    bf = np.logspace(6, -2.5, K)
    tau = 1 / (2 * np.pi * bf); eps = 1 / np.mean(np.diff(np.log(tau)))
    if irregular:
        f = np.sort(10 ** rs.uniform(-1.5, 5, nf))[::-1].copy()
    else:
        i0 = (K - nf) // 2
        f = bf[i0:i0 + nf].copy()
    A = np.vstack([construct_A(f, 'real', tau, eps), construct_A(f, 'imag', tau, eps)])
    L = [s * construct_L(bf, tau, eps, o) for s, o in ((0.36, 0), (0.24, 1), (0.12, 2))]
    w = 2 * np.pi * f
    z = 1.0 + 1.2 / (1 + (1j * w * 3e-3) ** 0.8) + 0.003 * (rs.normal(size=nf) + 1j * rs.normal(size=nf))
    z = z / (np.std(np.abs(z)) / np.sqrt(nf / 81))
    return A, L, np.concatenate([z.real, z.imag]), f


def random_point(D, seed=5):
    return np.ascontiguousarray(np.random.RandomState(seed).uniform(-1.5, 1.5, D))


def near_map_point(K, pos, scale=0.5):
    """A point shaped like a MAP: x two smooth bumps on a compact support and 1e-16 of its maximum outside it (those coefficients
    are at the floor of the linear scale; which of them are held is for the gradient to say), small error parameters (the
    likelihood is a visible share of the x-x block), smooth ups."""
    k = np.arange(K) / (K - 1.0)

    def bump(c, h):
        s = (k - c) / h
        return np.where(np.abs(s) < 1, np.exp(1.0 - 1.0 / np.maximum(1.0 - s * s, 1e-300)), 0.0)
    x = scale * (0.6 * bump(0.42, 0.16) + 0.35 * bump(0.66, 0.12))
    x = np.maximum(x, 1e-16 * np.max(x))
    D = 2 * K + 9
    y = np.empty(D)
    y[0], y[1] = np.log(0.8 * scale / 100.0), np.log(1e-7)                 # Rinf = 100 Rinf_raw, induc = induc_raw
    y[2:2 + K] = np.log(x) if pos else x
    y[2 + K:6 + K] = np.log(np.array([0.01, 0.02, 0.015, 0.012]) / 0.05)   # sigma_res, alpha_prop, alpha_re, alpha_im = 0.05 raw
    y[6 + K:6 + 2 * K] = np.log(1.0 + 0.5 * np.sin(2 * np.pi * k + 0.3))   # ups_raw
    y[6 + 2 * K:] = np.log([1.0, 0.8, 1.2])
    return np.ascontiguousarray(y)
