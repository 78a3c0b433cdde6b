"""Shared helpers of the density-matrix / mutual-information tests: the backend with the emulation of ``tpa_site_rho_batch`` stacked on
the others, and the recorded states of ``tests/golden/mutinf.pkl`` rebuilt as stand-alone ``MPS`` objects."""
import os
import pickle

import pytest

from measure_fixtures import build_psi  # noqa: F401
from mpo_cell_fixtures import _forget

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mutinf.pkl')


def _clear():
    from tenpy_amd.networks import measure, rho
    _forget()
    measure.clear_caches()
    rho.clear_caches()


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def rbackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point including ``tpa_site_rho_batch`` (tests/mock_rho.py); 'gpu': the HIP
    kernels on an MI355X.  The stacked route is on and its counters are zero."""
    from tenpy_amd import _lib
    from tenpy_amd.networks import rho
    _clear()
    if request.param == "mock":
        import mock_rho
        mock_rho.install(monkeypatch)
    else:
        _lib.require_gpu()
    monkeypatch.setattr(rho, 'MUTINF', True)
    rho.reset_stats()
    yield request.param
    _clear()


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN, 'rb') as f:
            _golden = pickle.load(f)
    return _golden


_psi = {}


def state(name, backend):
    """The recorded state ``name`` and its stand-alone ``MPS``, built once per backend."""
    key = (name, backend)
    if key not in _psi:
        rec = [r for r in golden() if r['name'] == name][0]
        _psi[key] = (rec, build_psi(rec))
    return _psi[key]
