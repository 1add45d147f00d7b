"""GPU test (-m gpu) of the sampler's kernel choice at creation: `Sampler.kind()` of freshly created samplers (never advanced)
against the table tests/golden/sampler_plan_kinds.json, for one problem of each regime, unit counts at every threshold of the
choice and one past it, every override variable on its own, and the one pair of overrides that reaches the 4-units-per-CU limit.

The table holds what the library answered before the driver was rewritten around one launch plan (bdrt_sampler.hip); it is keyed
by multiples of the device's CU count.  BDRT_RECORD_SAMPLER_PLAN=<file> writes the answers there instead of comparing them."""
import ctypes as C
import json
import os

import pytest

from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu

TABLE = os.path.join(GOLDEN, 'sampler_plan_kinds.json')
RECORD = os.environ.get('BDRT_RECORD_SAMPLER_PLAN')

# thresholds of the choice in units per CU (numerator, denominator): one workgroup per CU; the wave kernel pays from two chains per CU on;
# the general one-chain kernel up to 11/4; the one-chain kernels up to 4 (5 when two workgroups share a CU); the wave kernel keeps
# 4 (outlier / multi-distribution models) or 8 chains per CU resident
THRESHOLDS = [(1, 1), (2, 1), (11, 4), (4, 1), (5, 1), (8, 1)]
OVERRIDES = [('BDRT_SOLO', '0'), ('BDRT_SOLO', '1'), ('BDRT_WAVE', '0'), ('BDRT_WAVE', '1'), ('BDRT_WIDE1', '0'),
             ('BDRT_CHAINS_PER_WG', '4')]
CHOICE_VARIABLES = ('BDRT_SOLO', 'BDRT_WAVE', 'BDRT_WIDE1', 'BDRT_CHAINS_PER_WG', 'BDRT_TAIL_MIGRATION', 'BDRT_COMPACTION',
                    'BDRT_SOLO_DUO')


def _make_problem(regime):
    from bayes_drt_amd.model import Problem
    if regime == 'headline':                    # solo-capable single DRT on a log-uniform grid (41 x 81)
        from tests.test_gpu_wave import _problem
        return _problem('K81')[0]
    if regime == 'outliers':                    # the same family with the outlier error model: wave-capable, not solo-capable
        from tests.test_gpu_solo_wide import _family
        return Problem(**_family('series_outliers'))
    if regime == 'wide1_only':                  # two distributions on a measured frequency grid: the general one-chain kernel only
        from tests.test_gpu_solo_wide import _family
        return Problem(**_family('kat_series_parallel_outliers'))
    from tests.test_gpu_big import _big_problem     # beyond the LDS budget: the streamed evaluator
    return _big_problem(nf=150, K=221)[0]


def _n_cu():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _cases(n_cu):
    for num, den in THRESHOLDS:
        for past in (0, 1):
            yield '%d/%d%s' % (num, den, '+1' if past else ''), (num * n_cu) // den + past, []
    for var, val in OVERRIDES:
        for label, n in (('1/1', n_cu), ('2/1+1', 2 * n_cu + 1)):
            yield '%s %s=%s' % (label, var, val), n, [(var, val)]
    # without the wave kernel the 512-thread one-chain kernels go up to 4 units per CU, or 5 when two workgroups share a CU
    for label, n in (('4/1', 4 * n_cu), ('4/1+1', 4 * n_cu + 1), ('5/1', 5 * n_cu), ('5/1+1', 5 * n_cu + 1)):
        yield '%s BDRT_WAVE=0' % label, n, [('BDRT_WAVE', '0')]
    # ... and 4 it is when two workgroups may not share a CU (the problems here are small enough that they otherwise fit)
    for label, n in (('4/1', 4 * n_cu), ('4/1+1', 4 * n_cu + 1)):
        yield '%s BDRT_WAVE=0 BDRT_SOLO_DUO=0' % label, n, [('BDRT_WAVE', '0'), ('BDRT_SOLO_DUO', '0')]


def _kinds(regime, monkeypatch):
    from bayes_drt_amd._lib import NutsControl
    from bayes_drt_amd.engine import Sampler
    for v in CHOICE_VARIABLES:
        monkeypatch.delenv(v, raising=False)
    prob = _make_problem(regime)
    ctrl = NutsControl(); prob._lib.bdrt_nuts_defaults(C.byref(ctrl))
    out = {}
    for label, n_units, override in _cases(_n_cu()):
        for var, val in override:
            monkeypatch.setenv(var, val)
        with Sampler(prob, n_units, 2, 1, 7, ctrl) as smp:
            out[label] = smp.kind()
            assert smp.tail_units() == 0 and smp.compactions() == 0
        for var, _ in override:
            monkeypatch.delenv(var)
    prob.close()
    return out


@pytest.mark.parametrize('regime', ['headline', 'outliers', 'wide1_only', 'big'])
def test_kernel_choice_at_creation_equals_the_recorded_table(regime, monkeypatch):
    got = _kinds(regime, monkeypatch)
    if RECORD:
        table = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        table[regime] = got
        with open(RECORD, 'w') as fh:
            json.dump(table, fh, indent=1, sort_keys=True)
        return
    want = json.load(open(TABLE))[regime]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
