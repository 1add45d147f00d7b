"""The headline evaluator's entry phases (bdrt_tile_s1.h: P1 and P3) read and write their rows at lane bases + immediate offsets,
without a clamp of the row to K / nf, and the sampler's instantiations take the range tests of the rows below s1_kmin(NJ) for granted.
None of that may change a bit: the results are held to recordings of the build before the lane bases (tests/golden/
entry_phase_bits_*.npz, written by `python tests/test_gpu_entry_phase_bits.py --record` with that build as BDRT_LIBRARY; the recorder
runs every case twice and refuses to write unless the two runs agree bit for bit).

The shapes are the smallest at which an unclamped read or an always-true predicate can go wrong:
  (a) the sampler (LDSIO: theta rows in LDS), 19 units on five spectra -- the 16th chain of the first workgroup is there (its
      parameter reads beyond K leave the theta rows), the second workgroup has three live chains -- at 81 x 161 (six rows per lane,
      table GEMMs), 41 x 51 (two), 53 x 81 (three) and 106 x 101 (four, the any-shape table GEMMs), and at the shortest basis of each
      sampler instantiation, K = s1_kmin(NJ) = 60, 92, 108 (the rows below it carry no range test; the row that holds K does);
  (b) the evaluator on global memory (the clamped parameter reads must be untouched, P3 is shared), B = 19, at the same shapes plus
      the shortest basis of each evaluator instantiation (K = 33, 65, 97, 129), and with both outlier error models.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SPEC = np.array([0, 1, 2, 3, 4, 0, 1, 2,   4, 3, 0, 1, 0, 4, 3, 1,   4, 0, 3], dtype=np.int32)
SAMPLER_SHAPES = [(81, 161), (41, 51), (53, 81), (106, 101), (41, 60), (53, 92), (81, 108)]
EVAL_CASES = [(81, 161, 0), (41, 51, 0), (53, 81, 0), (106, 101, 0), (41, 33, 0), (41, 65, 0), (53, 97, 0), (81, 129, 0),
              (81, 161, 1), (81, 161, 2), (41, 51, 1), (41, 51, 2)]
ENV = {'BDRT_SOLO': '0', 'BDRT_WIDE1': '0', 'BDRT_WAVE': '0', 'BDRT_CHAINS_PER_WG': '16', 'BDRT_FEW_POINTS': '0'}
WARM, ND, SEED = 5, 3, 97531


def _problem(nf, K, omode=0):
    import bench
    from bayes_drt_amd.model import Problem
    kw = bench.shape_problem_kwargs(nf, K, 5)
    blocks, Z, freq = kw.pop('blocks'), kw.pop('Z'), kw.pop('freq')
    return Problem(blocks, Z, freq, outlier_mode=omode, **kw)


def run_sampler(nf, K):
    from bayes_drt_amd import _lib
    from bayes_drt_amd.engine import Sampler
    lib = _lib.require_gpu()
    prob = _problem(nf, K)
    assert prob.evaluator() in (2, 4) and prob.D == 2 * K + 9
    ctrl = _lib.NutsControl(); lib.bdrt_nuts_defaults(C.byref(ctrl))
    ctrl.max_treedepth = 5
    with Sampler(prob, len(SPEC), WARM, ND, SEED, ctrl, spec=SPEC, chain_ids=np.arange(len(SPEC), dtype=np.int32)) as smp:
        assert smp.kind() == 0
        smp.run()
        draws, lp, diag = smp.results()
    prob.close()
    return dict(draws=draws, lp=lp, n_leapfrog=np.array([d['n_leapfrog'] for d in diag], dtype=np.int64))


def run_eval(nf, K, omode):
    prob = _problem(nf, K, omode)
    assert prob.evaluator() in (2, 4) and prob.D == 2 * K + 9 + (2 * nf if omode else 0)
    th = np.random.default_rng(1000 * nf + K + omode).uniform(-2.0, 2.0, (len(SPEC), prob.D))
    lp, g = prob.logp_grad(th, jacobian=True, spec=SPEC)
    prob.close()
    return dict(lp=lp, grad=g)


def _same_bits(got, want, what):
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape)
        assert np.all(np.isfinite(a)), (what, k)
        assert a.tobytes() == b.tobytes(), (what, k, int(np.sum(a != b)), 'values differ')


@pytest.fixture(scope='module')
def golden():
    return {n: dict(np.load(os.path.join(GOLDEN, 'entry_phase_bits_%s.npz' % n))) for n in ('sampler', 'eval')}


@pytest.fixture
def env(monkeypatch):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize('nf,K', SAMPLER_SHAPES)
def test_sampler_bits_equal_the_recording(nf, K, golden, env):
    got = run_sampler(nf, K)
    _same_bits(got, {k: golden['sampler']['%dx%d_%s' % (nf, K, k)] for k in got}, (nf, K))


@pytest.mark.parametrize('nf,K,omode', EVAL_CASES)
def test_evaluator_bits_equal_the_recording(nf, K, omode, golden, env):
    got = run_eval(nf, K, omode)
    _same_bits(got, {k: golden['eval']['%dx%d_o%d_%s' % (nf, K, omode, k)] for k in got}, (nf, K, omode))


def _record():
    """Both recordings from the library that BDRT_LIBRARY names (the build to hold later ones to); every case twice."""
    os.environ.update(ENV)
    sys.path.insert(0, ROOT)
    out = {'sampler': {}, 'eval': {}}
    for nf, K in SAMPLER_SHAPES:
        a, b = run_sampler(nf, K), run_sampler(nf, K)
        _same_bits(a, b, ('recording', nf, K))
        out['sampler'].update({'%dx%d_%s' % (nf, K, k): v for k, v in a.items()})
    for nf, K, omode in EVAL_CASES:
        a, b = run_eval(nf, K, omode), run_eval(nf, K, omode)
        _same_bits(a, b, ('recording', nf, K, omode))
        out['eval'].update({'%dx%d_o%d_%s' % (nf, K, omode, k): v for k, v in a.items()})
    dest = os.environ.get('BDRT_RECORD_DIR', GOLDEN)
    os.makedirs(dest, exist_ok=True)
    for n, arrays in out.items():
        np.savez(os.path.join(dest, 'entry_phase_bits_%s.npz' % n), **arrays)
        print('wrote', n, len(arrays), 'arrays')


if __name__ == '__main__':
    if '--record' in sys.argv:
        _record()
