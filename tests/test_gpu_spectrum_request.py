"""The 16-chain kernel's per-chain spectrum addressing on the Toeplitz-table path, at a small size.

The evaluator inside the sampler (bdrt_tile_s1.h: load_spectrum) requests a chain's measured spectrum by a lane offset that carries the
chain's spectrum index; the two chains of a wave may sit on different spectra, and the rows it reads beyond nf of the last spectrum
lie in the padding behind P.Z.  The other small-shape tests of this kernel run every chain on spectrum 0.

19 units: one full workgroup and one with three live columns.  Units w and w + 8 share wave w (columns 2 w and 2 w + 1), and are
given different spectra; the last spectrum (4) is used by unit 4 (column 8, even) and unit 8 (column 1, odd), spectrum 0 by units 0,
5, 10, 12 and 17.
  (a) every unit, draw by draw, against the recursive CPU oracle on its own spectrum;
  (b) three of the units sampled alone (other columns, other workgroup) give the same bits.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPEC = np.array([0, 1, 2, 3, 4, 0, 1, 2,   4, 3, 0, 1, 0, 4, 3, 1,   4, 0, 3], dtype=np.int32)
PICK = [4, 8, 18]


@pytest.mark.parametrize('nf,K', [(81, 161), (81, 81)])
def test_sixteen_chain_kernel_with_mixed_spectra_vs_oracle_and_vs_packing(nf, K, monkeypatch):
    import bench
    from bayes_drt_amd import _lib
    from bayes_drt_amd.engine import Sampler
    from bayes_drt_amd.model import Problem
    from oracle import oracle as orc
    lib = _lib.require_gpu()
    monkeypatch.setenv('BDRT_SOLO', '0'); monkeypatch.setenv('BDRT_WIDE1', '0'); monkeypatch.setenv('BDRT_WAVE', '0')
    monkeypatch.setenv('BDRT_CHAINS_PER_WG', '16')
    kw = bench.shape_problem_kwargs(nf, K, 5)
    blocks, Z, freq = kw.pop('blocks'), kw.pop('Z'), kw.pop('freq')
    prob = Problem(blocks, Z, freq, **kw)
    assert prob.evaluator() == 4
    n_units = len(SPEC)
    assert n_units == 19 and all(SPEC[w] != SPEC[w + 8] for w in range(8))
    assert SPEC[4] == 4 and SPEC[8] == 4 and 0 in SPEC
    cid = np.arange(n_units, dtype=np.int32)
    ctrl = _lib.NutsControl(); lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    warm, nd, seed = 6, 4, 4321
    with Sampler(prob, n_units, warm, nd, seed, ctrl, spec=SPEC, chain_ids=cid) as smp:
        assert smp.kind() == 0
        smp.run()
        draws, lp, diag = smp.results()
    assert np.all(np.isfinite(draws)) and np.all(np.isfinite(lp))

    # (a) every unit against the oracle on its own spectrum
    octrl = orc.nuts_control(max_treedepth=5)
    models = [orc.OracleModel(blocks, Z[s], freq, **kw) for s in range(Z.shape[0])]
    for u in range(n_units):
        ref, lpr, dr = orc.nuts_sample(models[SPEC[u]], int(cid[u]), seed, warm, nd, control=octrl)
        assert dr['n_leapfrog'] == diag[u]['n_leapfrog'], (u, dr, diag[u])
        assert np.max(np.abs(draws[u] - ref)) < 1e-6 * np.max(np.abs(ref)), u
        assert np.allclose(lp[u], lpr, rtol=1e-8, atol=1e-6), u

    # (b) three of them alone: other columns, one workgroup, same bits
    with Sampler(prob, len(PICK), warm, nd, seed, ctrl, spec=SPEC[PICK], chain_ids=cid[PICK]) as smp:
        assert smp.kind() == 0
        smp.run()
        da, lpa, _ = smp.results()
    assert np.array_equal(da, draws[PICK]) and np.array_equal(lpa, lp[PICK])
    prob.close()
