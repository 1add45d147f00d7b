"""Numpy statement of the HMC convergence diagnostics (the yardstick of bayes_drt_amd/csrc/bdrt_diag.hip).

Follows Stan 2.19 as pystan 2.19's `chains.ess_and_splitrhat` applies it: the NON-split effective sample size of
stan/analyze/mcmc/compute_effective_sample_size.hpp (Geyer's initial positive + initial monotone sequence, with the
antithetic bias term) and the split R-hat of compute_potential_scale_reduction.hpp.  The autocovariance is Stan's
`autocovariance` (stan/math/prim/mat/fun/autocovariance.hpp): FFT of the centred series, zero-padded, normalised by N.

What could not be pinned to pystan's output bit for bit (neither pystan nor Stan's C++ is available to compare against): the
FFT rounding (Stan uses Eigen's FFT with padding to an even length; numpy's rfft with padding to a power of two >= 2N here),
and the order of Eigen's `.sum()` reductions.  Both change results in the last bits only.

`y` is one column: [M chains, N draws].
"""
import numpy as np

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def autocovariance_fft(c):
    """acov[k] = (1/N) sum_{t=0}^{N-1-k} c[t] c[t+k] for a centred 1-D series `c`, through a zero-padded FFT."""
    N = len(c)
    nfft = 1
    while nfft < 2 * N:
        nfft <<= 1
    f = np.fft.rfft(c, nfft)
    ac = np.fft.irfft(f * np.conj(f), nfft)[:N]
    return ac / N


def autocovariance_direct(c):
    N = len(c)
    return np.array([np.dot(c[:N - k], c[k:]) for k in range(N)]) / N


def ess(y):
    """Non-split effective sample size of one column y [M, N] (Stan 2.19 compute_effective_sample_size)."""
    return ess_and_margin(y)[0]


def ess_and_margin(y):
    """(n_eff, margin) of one column: margin = the smallest |rho[s+1] + rho[s+2]| over the pairs Geyer's loop evaluated (pair 0
    included), i.e. how close a pair sum came to the sign test that ends the sequence.  The sum is rho = 1 - (mean_var -
    acov) / var_plus, so a margin below 1e-10 is a pair sum within 1e-10 var_plus of 0 in autocovariance units: another
    rounding of the lag sums may end the sequence one pair earlier or later there.  NaN columns: margin inf."""
    y = np.asarray(y, dtype=np.float64)
    M, N = y.shape
    if not np.all(np.isfinite(y)) or N < 4:
        return np.nan, np.inf
    if np.all(y == y[0, 0]):
        return np.nan, np.inf
    acov = np.array([autocovariance_fft(y[m] - y[m].mean()) for m in range(M)])   # [M, N]
    chain_mean = y.mean(axis=1)
    chain_var = acov[:, 0] * N / (N - 1.0)
    mean_var = chain_var.mean()
    var_plus = mean_var * (N - 1.0) / N
    if M > 1:
        var_plus += np.var(chain_mean, ddof=1)
    acov_mean = acov.mean(axis=0)
    rho = np.zeros(N)
    rho_even = 1.0
    rho[0] = rho_even
    rho_odd = 1.0 - (mean_var - acov_mean[1]) / var_plus
    rho[1] = rho_odd
    margin = abs(rho_even + rho_odd)
    s = 1
    while s < N - 4 and rho_even + rho_odd > 0:
        rho_even = 1.0 - (mean_var - acov_mean[s + 1]) / var_plus
        rho_odd = 1.0 - (mean_var - acov_mean[s + 2]) / var_plus
        margin = min(margin, abs(rho_even + rho_odd))
        if rho_even + rho_odd >= 0:
            rho[s + 1] = rho_even
            rho[s + 2] = rho_odd
        s += 2
    max_s = s
    if rho_even > 0:
        rho[max_s + 1] = rho_even                          # antithetic bias term
    for t in range(1, max_s - 2, 2):                       # initial monotone sequence: t = 1, 3, ..., max_s - 3
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = (rho[t - 1] + rho[t]) / 2.0
            rho[t + 2] = rho[t + 1]
    tau = -1.0 + 2.0 * np.sum(rho[:max_s]) + rho[max_s + 1]
    return M * N / tau, margin


def split_rhat(y):
    """Split R-hat of one column y [M, N] (Stan 2.19 compute_split_potential_scale_reduction)."""
    y = np.asarray(y, dtype=np.float64)
    M, N = y.shape
    if not np.all(np.isfinite(y)):
        return np.nan
    if np.all(y == y[0, 0]):
        return np.nan
    n = N // 2
    if n < 2:
        return np.nan
    halves = np.concatenate([y[:, :n], y[:, N - n:]], axis=0)    # second half starts at ceil(N/2)
    B = n * np.var(halves.mean(axis=1), ddof=1)
    W = np.mean(np.var(halves, axis=1, ddof=1))
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt((B / W + n - 1.0) / n)


def column_stats(y):
    """(mean, sd, n_eff, Rhat) of one column y [M, N]: sd over all draws with ddof = 1."""
    y = np.asarray(y, dtype=np.float64)
    flat = y.ravel()
    sd = np.std(flat, ddof=1) if flat.size > 1 else np.nan
    return flat.mean(), sd, ess(y), split_rhat(y)


def diagnostics(X):
    """X [G groups, M chains, N draws, C columns] -> mean, sd, n_eff, Rhat, each [G, C]."""
    X = np.asarray(X, dtype=np.float64)
    G, M, N, Cc = X.shape
    out = np.empty((4, G, Cc))
    for g in range(G):
        for c in range(Cc):
            out[:, g, c] = column_stats(X[g, :, :, c])
    return out[0], out[1], out[2], out[3]


def ar1(rng, phi, M, N, burn=200):
    """M chains of a stationary AR(1) series with coefficient phi and unit innovation variance: [M, N]."""
    e = rng.standard_normal((M, N + burn))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(max(1e-12, 1.0 - phi * phi))
    for t in range(1, N + burn):
        x[:, t] = phi * x[:, t - 1] + e[:, t]
    return x[:, burn:]
