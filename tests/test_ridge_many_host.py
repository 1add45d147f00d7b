"""Inverter.ridge_fit_many without a GPU: argument errors are raised before any device call, an empty batch is an empty list,
and the two entries under the batch are part of the bound ABI."""
import numpy as np
import pytest

from bayes_drt_amd import _lib
from bayes_drt_amd.inversion import Inverter

F = np.logspace(5, -1, 13)
Z = 1.0 + 1.0 / (1.0 + 2j * np.pi * F * 1e-2)


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    def refuse():
        raise AssertionError('the GPU was asked for')
    monkeypatch.setattr(_lib, 'require_gpu', refuse)


@pytest.mark.parametrize('kw', [dict(lambda_0=[1e-2, 1e-1, 1.0]), dict(hl_fbeta=[0.1]), dict(hl_beta=[2.5, 2.5, 2.5])])
def test_list_lengths_must_match_the_spectra(kw):
    with pytest.raises(ValueError, match='ridge_fit_many'):
        Inverter(basis_freq=F).ridge_fit_many(F, [Z, Z], **kw)


def test_frequency_grids_must_match_the_spectra():
    with pytest.raises(ValueError):
        Inverter(basis_freq=F).ridge_fit_many(np.stack([F, F, F]), [Z, Z])
    with pytest.raises(ValueError):
        Inverter(basis_freq=F).ridge_fit_many(F, [Z, Z[:-1]])


def test_several_distributions_are_refused():
    inv = Inverter(basis_freq=F, distributions={'DRT': {'kernel': 'DRT'},
                                                'DDT': {'kernel': 'DDT', 'dist_type': 'parallel', 'symmetry': 'planar', 'bc': 'transmissive'}})
    with pytest.raises(ValueError, match='multiple distributions'):
        inv.ridge_fit_many(F, [Z, Z])


@pytest.mark.parametrize('kw', [dict(penalty='quadratic'), dict(part='modulus'), dict(preset='Nobody'), dict(hl_solution='newton'),
                                dict(penalty='integral', hl_beta=1.5), dict(hl_beta=[2.5, 0.5]),
                                dict(hyper_lambda=True, hyper_weights=True), dict(correct_phase_offset=True)])
def test_bad_arguments_are_refused_as_ridge_fit_refuses_them(kw):
    with pytest.raises(ValueError):
        Inverter(basis_freq=F).ridge_fit_many(F, [Z, Z], **kw)


def test_empty_batch():
    base = Inverter(basis_freq=F)
    assert base.ridge_fit_many(F, []) == []
    assert base.ridge_fit_many([], [], lambda_0='cv', preset='Huang') == []
    assert base.distribution_fits == {} and base.Z_train is None


def test_new_entries_are_bound():
    assert 'bdrt_gram_batch' in _lib.SYMBOLS and 'bdrt_ridge_ex' in _lib.SYMBOLS
    lib = _lib.load_library()
    assert len(lib.bdrt_gram_batch.argtypes) == 9
    assert len(lib.bdrt_ridge_ex.argtypes) == len(lib.bdrt_ridge.argtypes) + 2 == 25
