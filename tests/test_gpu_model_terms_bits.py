"""GPU test (-m gpu) that the one-chain evaluators keep their bits: solo_eval (bdrt_solo.h), wide1_eval (bdrt_solo_wide.h) and the
two wave evaluators (bdrt_wave.h) through their debug entries, and through the kernels that inline them with other instantiations and
register pressure -- the solo, wide1 and wave samplers and the device L-BFGS -- against the recorded fixture
tests/golden/model_terms_bits.npz (and model_terms_bits_<part>.npz beside it).

The fixture holds what the library answered before the pointwise terms of the model (likelihood point, outlier error model, ups prior,
scalar priors and gradients, parallel blocks) were moved into bdrt_model_terms.h; it holds outputs only.  It was recorded twice from
that library and every output below came out the same both times, so every output is held to its bits.  The inputs are rebuilt here:
the stored problems (tests/golden) and np.random.default_rng(seed).uniform(-2, 2, ...).  BDRT_RECORD_MODEL_TERMS=<file> writes the
answers there instead of comparing them.

A failure prints the largest ulp distance of every output that differs."""
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tests.test_gpu_post_stats_bits import _ulps
from tests.test_gpu_wave import _ctrl, _env

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'model_terms_bits.npz')
RECORD = os.environ.get('BDRT_RECORD_MODEL_TERMS')


def _part_file(path, part):
    return path if part is None else '%s_%s.npz' % (path[:-len('.npz')], part)


def _check(case, outs, part=None):
    """outs: {name: array} of one case, compared with (or recorded as) the fixture's '<case>/<name>'.  part: the cases with hundreds
    of kilobytes of gradients keep theirs in a file of their own, model_terms_bits_<part>.npz (no stored file beyond 1 MiB)."""
    outs = {'%s/%s' % (case, k): np.asarray(v) for k, v in outs.items()}
    if RECORD:
        path = _part_file(RECORD, part)
        table = dict(np.load(path)) if os.path.exists(path) else {}
        table.update(outs)
        np.savez_compressed(path, **table)
        return
    want = np.load(_part_file(FIXTURE, part))
    wrong = []
    for k, got in outs.items():
        ref = want[k]
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        if not np.array_equal(got, ref, equal_nan=got.dtype.kind == 'f'):
            d = _ulps(got, ref) if got.dtype.kind == 'f' else float(np.max(np.abs(got.astype(np.int64) - ref)))
            print('%s: largest distance %g ulp' % (k, d))
            wrong.append(k)
    assert not wrong, wrong


def _points(seed, n, D):
    return np.random.default_rng(seed).uniform(-2, 2, (n, D))


def _family_problem(name):
    from bayes_drt_amd.model import Problem
    from tests.test_gpu_solo_wide import _family
    return Problem(**_family(name))


# ------------------------------------------------------------------------------------------------ the evaluators on their own
@pytest.mark.parametrize('tag', ['K81', 'K101'])
@pytest.mark.parametrize('mode,pos', [('sample', True), ('optimize', True), ('sample', False)])
def test_solo_evaluator_bits(tag, mode, pos):
    from tests.test_gpu_solo import _problem, _solo_logp_grad
    prob, _ = _problem(tag, mode, pos)
    lp, g = _solo_logp_grad(prob, _points(201, 6, prob.D), mode == 'sample')
    prob.close()
    _check('solo_%s_%s_%s' % (tag, mode, 'pos' if pos else 'free'), {'lp': lp, 'grad': g})


@pytest.mark.parametrize('family', ['series_plain', 'series_outliers', 'series_parallel', 'series_parallel_outliers', 'kat_2parallel',
                                    'series_irregular_frequencies'])
def test_wide1_evaluator_bits(family):
    from tests.test_gpu_solo_wide import _wide1_logp_grad
    prob = _family_problem(family)
    theta = _points(202, 5, prob.D)
    outs = {}
    for jac in (True, False):
        lp, g = _wide1_logp_grad(prob, theta, jac)
        assert lp is not None
        outs.update({'lp_jac%d' % jac: lp, 'grad_jac%d' % jac: g})
    prob.close()
    _check('wide1_' + family, outs)


@pytest.mark.parametrize('tag', ['K81', 'K101'])
@pytest.mark.parametrize('occ', ['1', '2'])
def test_wave_evaluator_bits(tag, occ):
    """40 points: both halves of a wave's partition and a second workgroup"""
    from tests.test_gpu_wave import _problem, _wave_logp_grad
    prob, _ = _problem(tag)
    with _env(BDRT_WAVE_OCC=occ):
        lp, g = _wave_logp_grad(prob, _points(203, 40, prob.D), True)
    prob.close()
    _check('wave_%s_occ%s' % (tag, occ), {'lp': lp, 'grad': g})


@pytest.mark.parametrize('tag', ['K161', 'K81'])
@pytest.mark.parametrize('om_mode', [1, 2])
def test_wave_evaluator_with_the_outlier_model_bits(tag, om_mode):
    from tests.test_gpu_wave import _outlier_problem, _wave_logp_grad
    prob, _ = _outlier_problem(tag, om_mode)
    theta = _points(204, 40, prob.D)
    outs = {}
    for jac in (True, False):
        lp, g = _wave_logp_grad(prob, theta, jac)
        outs.update({'lp_jac%d' % jac: lp, 'grad_jac%d' % jac: g})
    prob.close()
    _check('wave_om%d_%s' % (om_mode, tag), outs, part='wave_om_' + tag)


@pytest.mark.parametrize('name', ['series_parallel', 'series_parallel_outliers', 'kat_2parallel'])
def test_wave_evaluator_of_the_multi_distribution_models_bits(name):
    from tests.test_gpu_wave import _wave_logp_grad
    prob = _family_problem(name)
    theta = _points(205, 40, prob.D)
    outs = {}
    for jac in (True, False):
        lp, g = _wave_logp_grad(prob, theta, jac)
        outs.update({'lp_jac%d' % jac: lp, 'grad_jac%d' % jac: g})
    prob.close()
    _check('wave_nb_' + name, outs, part='wave_nb_' + name)


# ------------------------------------------------------------------------------------------------ the evaluators inside their kernels
def _run_sampler(prob, n, warm, nd, seed, depth, kind=None):
    from bayes_drt_amd.engine import Sampler
    with Sampler(prob, n, warm, nd, seed, _ctrl(prob._lib, max_treedepth=depth)) as smp:
        if kind is not None:
            assert smp.kind() == kind, smp.kind()
        smp.run()
        draws, lp, diag = smp.results()
    return {'draws': draws, 'lp': lp, 'n_leapfrog': np.array([d['n_leapfrog'] for d in diag], dtype=np.int64)}


@pytest.mark.parametrize('kernel', ['solo', 'wave_occ1', 'wave_occ2'])
def test_sampler_of_the_headline_family_bits(kernel):
    from tests.test_gpu_solo import _problem
    prob, _ = _problem('K81')
    env = dict(BDRT_WAVE='0', BDRT_SOLO='1', BDRT_WAVE_OCC=None) if kernel == 'solo' else \
        dict(BDRT_WAVE='1', BDRT_SOLO=None, BDRT_WAVE_OCC=kernel[-1])
    with _env(**env):
        outs = _run_sampler(prob, 3, 30, 10, 31, 6, kind=1 if kernel == 'solo' else 3)
    prob.close()
    _check('nuts_K81_' + kernel, outs, part='kernels')


@pytest.mark.parametrize('family', ['series_parallel_outliers', 'kat_2parallel'])
@pytest.mark.parametrize('kernel', ['wide1', 'wave'])
def test_sampler_of_the_general_models_bits(family, kernel):
    prob = _family_problem(family)
    with _env(BDRT_WAVE='1' if kernel == 'wave' else None, BDRT_SOLO=None, BDRT_WIDE1=None, BDRT_WAVE_OCC=None):
        outs = _run_sampler(prob, 3, 12, 5, 32, 5, kind=2 if kernel == 'wide1' else 3)
    prob.close()
    _check('nuts_%s_%s' % (family, kernel), outs, part='kernels')


@pytest.mark.parametrize('which', ['K81', 'series_parallel'])
def test_device_lbfgs_bits(which):
    """the whole L-BFGS phase in lbfgs_kernel: on solo_eval (K81) and on wide1_eval (series_parallel)"""
    from bayes_drt_amd.engine import optimize_batch
    if which == 'K81':
        from tests.test_gpu_solo import _problem
        prob, _ = _problem('K81', 'optimize')
    else:
        prob = _family_problem(which)
    theta, rep = optimize_batch(prob, _points(206, 2, prob.D),max_iter=50, newton_max_iter=0)
    prob.close()
    _check('lbfgs_' + which, part='kernels', outs={'theta': theta, 'lp': np.array([r['lp'] for r in rep], dtype=np.float64),
                              'iterations': np.array([r['iterations'] for r in rep], dtype=np.int32),
                              'n_evals': np.array([r['n_evals'] for r in rep], dtype=np.int32)})
