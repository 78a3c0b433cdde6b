"""Shared helpers of the sampling tests: the backend with the emulations of ``tpa_sample_select_batch`` / ``tpa_sample_gather_batch``
stacked on the others, and the recorded states of ``tests/golden/sample.pkl`` rebuilt as stand-alone ``MPS`` objects
(``measure_fixtures.build_psi``)."""
import os
import pickle

import pytest

from measure_fixtures import build_psi  # noqa: F401
from mpo_cell_fixtures import _forget

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sample.pkl')


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def sbackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point including the two of ``tests/mock_sample.py``; 'gpu': the HIP kernels
    on an MI355X.  The route is switched on for batches and single-sample calls alike and its counters start at zero."""
    from tenpy_amd import _lib
    from tenpy_amd.networks import measure, sample
    _forget()
    measure.clear_caches()
    sample.clear_caches()
    if request.param == "mock":
        import mock_sample
        mock_sample.install(monkeypatch)
    else:
        _lib.require_gpu()
    monkeypatch.setattr(sample, 'SAMPLE', True)
    monkeypatch.setattr(sample, 'SINGLE', True)
    sample.reset_stats()
    yield request.param
    _forget()
    measure.clear_caches()
    sample.clear_caches()


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN, 'rb') as f:
            _golden = pickle.load(f)
    return _golden
