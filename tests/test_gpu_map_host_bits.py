"""GPU test (-m gpu) that the host code of the MAP path keeps its bits on the branches tests/test_gpu_host_owner_bits.py does not
reach: bdrt_optimize (theta and every field of the report) under each switch of the Newton iteration, through the host-driven
L-BFGS loop, on a model whose Hessian is differenced because it has no closed form, and for a batch in which one start is refused.

The fixture tests/golden/map_host_bits.npz holds what the library answered before bdrt_optimize and newton_polish_device were
taken apart into NewtonEnv / NewtonWork / lbfgs_host and named phases; it holds outputs only.  It was recorded twice from that
library and every output came out the same both times, so every output is held to its bits.  Inputs as in test_optimize_bits: the
stored K = 81 problem with 2 spectra, 3 starts from the integer recurrence, spec = [0, 1, 0]; newton_max_iter = 6 keeps a case to
seconds.  BDRT_RECORD_MAP_HOST=<file> writes the answers there instead of comparing them."""
import os

import numpy as np
import pytest

from tests.helpers import GOLDEN
from tests.test_gpu_host_owner_bits import _check, _uniform, lib  # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'map_host_bits.npz')
RECORD = os.environ.get('BDRT_RECORD_MAP_HOST')
SWITCHES = ('BDRT_NEWTON_SPEC', 'BDRT_NEWTON_FD', 'BDRT_NEWTON_LINEAR', 'BDRT_NEWTON_PROF', 'BDRT_NEWTON_TRIAL_FEW', 'BDRT_NEWTON_ROUNDS',
            'BDRT_NEWTON_TRACE', 'BDRT_HOST_LBFGS', 'BDRT_LBFGS_BEFORE_NEWTON')


def _outs(theta, rep):
    outs = {'theta': theta}
    for k in ('lp', 'grad_norm', 'grad_inf'):
        outs[k] = np.array([r[k] for r in rep], dtype=np.float64)
    for k in ('iterations', 'n_evals', 'return_code', 'newton_iterations'):
        outs[k] = np.array([r[k] for r in rep], dtype=np.int32)
    return outs


def _k81(monkeypatch, env, refuse=None, **opts):
    """bdrt_optimize on the stored K = 81 problem under the switches `env` (every other switch unset); refuse: the start that
    is replaced by a point at which exp() overflows"""
    from bayes_drt_amd.engine import optimize_batch
    from tests.test_gpu_hessian import _dat_problem
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob, _, _ = _dat_problem('dat_optimize_2ZARC_uniform_0.25_K81', True, n_spectra=2)
    th0 = np.ascontiguousarray(_uniform(151, (3, prob.D)) * 4.0)
    if refuse is not None:
        th0[refuse] = 800.0
    theta, rep = optimize_batch(prob, th0, spec=[0, 1, 0], **opts)
    prob.close()
    return _outs(theta, rep)


@pytest.mark.parametrize('case,env', [('fd', {'BDRT_NEWTON_FD': '1'}), ('log_scale', {'BDRT_NEWTON_LINEAR': '0'}),
                                      ('one_attempt', {'BDRT_NEWTON_SPEC': '0'}), ('trial_tile', {'BDRT_NEWTON_TRIAL_FEW': '0'}),
                                      ('rounds1', {'BDRT_NEWTON_ROUNDS': '1'})])
def test_newton_switch_bits(lib, monkeypatch, case, env):
    outs = _k81(monkeypatch, env, newton_max_iter=6)
    assert np.all(outs['newton_iterations'] > 0)
    if case == 'one_attempt':                    # the speculative factorisations change the time, not the numbers
        plain = _k81(monkeypatch, {}, newton_max_iter=6)
        for k in outs:
            assert np.array_equal(outs[k], plain[k]), k
    _check(case, outs, FIXTURE, RECORD)


def test_host_lbfgs_then_newton_bits(lib, monkeypatch):
    outs = _k81(monkeypatch, {'BDRT_HOST_LBFGS': '1'}, lbfgs_before_newton=20, newton_max_iter=6)
    assert np.all(outs['iterations'] > 0) and np.all(outs['newton_iterations'] > 0)
    _check('host_lbfgs20_newton', outs, FIXTURE, RECORD)


def test_host_lbfgs_alone_bits(lib, monkeypatch):
    """no Newton phase: the reports come from the L-BFGS state"""
    outs = _k81(monkeypatch, {'BDRT_HOST_LBFGS': '1'}, max_iter=25, newton_max_iter=0)
    assert np.all(outs['iterations'] > 0) and np.all(outs['newton_iterations'] == 0)
    _check('host_lbfgs25', outs, FIXTURE, RECORD)


def test_differenced_by_the_model_bits(lib, monkeypatch):
    """12 x 9 general matrices: no closed-form Hessian (tests/test_gpu_hessian.py::test_models_without_a_closed_form_say_so), so
    the iteration differences gradients without being told to"""
    from bayes_drt_amd.engine import optimize_batch
    from bayes_drt_amd.model import Problem
    from tests.test_gpu_engine import _small_problem
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    blk, Z, f, kw = _small_problem()
    prob = Problem([blk], Z, f, **kw)
    th0 = np.ascontiguousarray(_uniform(152, (3, prob.D)) * 4.0)
    theta, rep = optimize_batch(prob, th0, newton_max_iter=3)
    prob.close()
    outs = _outs(theta, rep)
    assert np.all(outs['newton_iterations'] > 0)
    _check('small_general', outs, FIXTURE, RECORD)


def test_refused_start_bits(lib, monkeypatch):
    """start 1 overflows (lp is not finite there): it is refused with return code -1 before the first round, its neighbours go on"""
    outs = _k81(monkeypatch, {}, refuse=1, newton_max_iter=6)
    assert not np.isfinite(outs['lp'][1]) and outs['return_code'][1] == -1 and outs['newton_iterations'][1] == 0
    assert np.array_equal(outs['theta'][1], np.full(outs['theta'].shape[1], 800.0))
    assert np.all(outs['newton_iterations'][[0, 2]] > 0)
    _check('refused_start', outs, FIXTURE, RECORD)
