"""The device path of PSIS-LOO (`Sampler.loo`, `fit_many(loo=...)`, `sample_sharded(loo=...)`) as far as it is reachable without
a GPU: arguments are refused before any GPU work with the messages of the host path, and the two entry points are declared in
the binding with the header's signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bayes_drt_amd import _lib
from bayes_drt_amd import loo as L
from bayes_drt_amd.inversion import Inverter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASIS = np.logspace(6, -2, 81)


def _spectrum():
    f = np.logspace(5, -1, 31)
    Z = 1.0 + 1.0 / (1.0 + (2j * np.pi * f * 1e-2) ** 0.8)
    return f, Z


def test_optimize_mode_refuses_loo_before_any_gpu_work(monkeypatch):
    f, Z = _spectrum()
    called = []
    monkeypatch.setattr(Inverter, '_batch_jobs', lambda *a, **k: called.append('batch') or ([], []))
    monkeypatch.setattr(Inverter, '_fit_prepare', lambda *a, **k: called.append('prepare'))
    inv = Inverter(basis_freq=BASIS)
    for kw in (dict(loo=True), dict(loo_predict=True), dict(loo=True, loo_predict=True, loo_kw=dict(reff=None))):
        with pytest.raises(ValueError, match="mode='sample'"):
            inv.fit_many(f, [Z, Z], mode='optimize', **kw)
        with pytest.raises(ValueError, match="mode='sample'"):
            inv.fit(f, Z, mode='optimize', **kw)
    assert called == []
    assert not hasattr(inv, 'loo_result') and not hasattr(inv, 'loo_predict_result')


def test_loo_kw_is_checked_with_the_existing_messages(monkeypatch):
    f, Z = _spectrum()
    called = []
    monkeypatch.setattr(Inverter, '_batch_jobs', lambda *a, **k: called.append('batch') or ([], []))
    inv = Inverter(basis_freq=BASIS)

    def many(**kw):
        return inv.fit_many(f, [Z], mode='sample', **kw)
    with pytest.raises(ValueError, match=r"unknown keys \['chunk', 'part'\]"):
        many(loo=True, loo_kw=dict(part='real', chunk=3))
    with pytest.raises(ValueError, match="unit must be 'frequency' or 'point', not 'pair'"):
        many(loo=True, loo_kw=dict(unit='pair'))
    with pytest.raises(ValueError, match="reff must be 'auto', None, a number or an array"):
        many(loo_predict=True, loo_kw=dict(reff='automatic'))
    for bad in (0.0, -1.0, np.nan, np.inf, [0.5, -0.5]):
        with pytest.raises(ValueError, match='reff must be positive and finite'):
            many(loo=True, loo_kw=dict(reff=bad))
    with pytest.raises(ValueError, match='neither loo nor loo_predict'):
        many(loo_kw=dict(reff=None))
    assert called == []
    # accepted arguments reach the engine: the stub's empty batch comes back
    assert many(loo=True, loo_predict=True, loo_kw=dict(unit='point', reff=0.37)) == [] and called == ['batch']


def test_argument_dict_of_the_engine():
    assert Inverter._loo_arguments(False, False, None, 'optimize', 'both') is None
    assert Inverter._loo_arguments(True, False, None, 'sample', 'both') == dict(unit='frequency', reff='auto', loo=True,
                                                                                 predict=False, part='both')
    # a fit of one part has points for units, as `loo(part='real')` of such a fit has
    assert Inverter._loo_arguments(False, True, dict(reff=None), 'sample', 'imag') == dict(unit='point', reff=None, loo=False,
                                                                                            predict=True, part='imag')
    assert L.check_device_args('point', 'real', 2.0) == (0, 1)
    assert L.check_device_args('frequency', 'both', None) == (1, 0)
    assert L.check_device_args('frequency', 'both', 'auto') == (1, 2)
    with pytest.raises(ValueError, match="unit='frequency' needs part='both'"):
        L.check_device_args('frequency', 'real', None)
    with pytest.raises(ValueError, match="part must be 'both', 'real' or 'imag'"):
        L.check_device_args('point', 'imaginary', None)
    with pytest.raises(ValueError, match='chunk_bytes'):
        L.chunk_or_default(-1)
    assert L.chunk_or_default(None) == 0 and L.chunk_or_default(1 << 20) == 1 << 20


def test_sample_units_checks_its_loo_dict_before_a_sampler_exists():
    from bayes_drt_amd.engine import sample_units
    with pytest.raises(ValueError, match='loo needs chains'):
        sample_units(None, 4, 10, 10, 1, loo=dict(reff=None))
    with pytest.raises(ValueError, match='loo needs chains'):
        sample_units(None, 4, 10, 10, 1, loo=dict(chains=2, parts='real'))
    with pytest.raises(ValueError, match="unit must be 'frequency' or 'point'"):
        sample_units(None, 4, 10, 10, 1, loo=dict(chains=2, unit='both'))


def test_sample_result_is_a_triple_with_named_extras():
    from bayes_drt_amd.engine import SampleResult
    d, l, g = np.zeros((2, 3, 4)), np.zeros((2, 3)), [{}, {}]
    res = SampleResult(d, l, g)
    a, b, c = res
    assert a is d and b is l and c is g and len(res) == 3 and isinstance(res, tuple) and res[2] is g
    assert res.diagnostics is None and res.loo is None and res.heldout is None
    stats, loo, held = (1, 2, 3, 4), {'loo': {}}, {'lpd': 0}
    res = SampleResult(d, l, g, diagnostics=stats, loo=loo, heldout=held)
    assert len(res) == 3 and res.diagnostics is stats and res.loo is loo and res.heldout is held


def test_loo_request_is_complete_and_checked_once():
    full = dict(chains=None, loo=True, predict=False, unit='frequency', part='both', reff='auto', chunk_bytes=None)
    assert tuple(full) == L.LOO_KEYS
    assert L.loo_request({}, 'f', need_chains=False) == full and L.loo_request(None, 'f', need_chains=False) == full
    assert L.loo_request(dict(chains=2), 'f', need_chains=True) == dict(full, chains=2)
    given = dict(chains=4, loo=False, predict=True, unit='point', part='imag', reff=0.5, chunk_bytes=1 << 20)
    assert L.loo_request(given, 'f', need_chains=True) == given
    # the request itself is taken as it stands; `check_loo_kw` is where a fit of one part gets points for units
    assert L.loo_request(dict(unit='point', part='real'), 'f', False)['unit'] == 'point'
    with pytest.raises(ValueError, match="unit='frequency' needs part='both'"):
        L.loo_request(dict(part='real'), 'f', False)
    assert L.check_loo_kw(None, 'real') == dict(unit='point', reff='auto')
    assert L.check_loo_kw(dict(unit='frequency', reff=None), 'imag') == dict(unit='point', reff=None)
    assert L.check_loo_kw(dict(unit='frequency'), 'both') == dict(unit='frequency', reff='auto')
    for kw, need, msg in ((dict(reff=None), True, 'loo needs chains'), (dict(chains=2, parts='real'), True, 'loo needs chains'),
                          (dict(chains=2, parts='real'), True, r"unknown keys \['parts'\]"),
                          (dict(chains=2), False, r"unknown keys \['chains'\]"), (dict(unit='pair'), False, "unit must be 'frequency' or 'point', not 'pair'"),
                          (dict(part='half'), False, "part must be 'both', 'real' or 'imag'"),
                          (dict(reff='automatic'), False, "reff must be 'auto', None, a number or an array"),
                          (dict(reff=-1.0), False, 'f: reff must be positive and finite'), (dict(chunk_bytes=-1), False, 'chunk_bytes must not be negative')):
        with pytest.raises(ValueError, match=msg):
            L.loo_request(kw, 'f', need)
    with pytest.raises(ValueError, match=r"loo_kw: unknown keys \['chunk', 'part'\]"):
        L.check_loo_kw(dict(part='real', chunk=3))


def test_the_rules_of_parts_and_units():
    assert [L.part_columns(p, 3) for p in L.PARTS] == [(0, 6), (0, 3), (3, 3)]
    assert [L.effective_unit(u, p) for u in L.UNITS for p in ('both', 'real')] == ['frequency', 'point', 'point', 'point']
    assert L.effective_unit('frequency', 'imag') == 'point'


def _header_args(name):
    txt = open(os.path.join(ROOT, 'include', 'bdrt.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    m = re.search(r'\b(\w[\w ]*?)\s*\b%s\s*\(([^)]*)\)\s*;' % name, txt)
    assert m, name
    return m.group(1).split()[-1], [' '.join(a.split()) for a in m.group(2).split(',')]


def _ctype(arg):
    if '*' in arg:
        return C.c_void_p
    return {'int': C.c_int, 'size_t': C.c_size_t}[arg.split()[0]]


@pytest.mark.parametrize('name', ['bdrt_sampler_loo', 'bdrt_sampler_loo_predict', 'bdrt_sampler_loo_group_bytes'])
def test_new_symbols_are_bound_with_the_headers_signatures(name):
    assert name in _lib.SYMBOLS
    ret, args = _header_args(name)
    fn = getattr(_lib.load_library(), name)
    assert [_ctype(a) for a in args] == list(fn.argtypes), (args, fn.argtypes)
    assert fn.restype is (C.c_size_t if ret == 'size_t' else C.c_int)
    front = ['bdrt_sampler *s', 'int unit_lo', 'int unit_hi', 'int chains_per_group', 'int pair', 'int col0', 'int ncols',
             'int reff_mode', 'const double *reff_in', 'size_t chunk_bytes']
    if name != 'bdrt_sampler_loo_group_bytes':
        assert args[:10] == front and args[-1] == 'double *reff_out'


def test_existing_symbols_keep_their_order_in_the_binding():
    i = _lib.SYMBOLS.index('bdrt_psis_predict_max_draws')
    assert _lib.SYMBOLS[i + 1:i + 4] == ['bdrt_sampler_loo', 'bdrt_sampler_loo_predict', 'bdrt_sampler_loo_group_bytes']
    assert _lib.SYMBOLS[i + 4] == 'bdrt_last_error'
