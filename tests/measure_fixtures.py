"""Shared helpers of the measurement tests: the backend with the emulation of ``tpa_site_inner_batch`` stacked on the others, the
recorded states of ``tests/golden/measure.pkl`` rebuilt as stand-alone ``MPS`` objects, and a counter of launches that works on both
backends."""
import os
import pickle

import numpy as np
import pytest

from mpo_cell_fixtures import _forget, blocked_array
from tenpy_amd.linalg.charges import ChargeInfo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'measure.pkl')


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def mbackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point including ``tpa_site_inner_batch`` (tests/mock_measure.py); 'gpu':
    the HIP kernels on an MI355X."""
    from tenpy_amd import _lib
    from tenpy_amd.networks import measure
    _forget()
    measure.clear_caches()
    if request.param == "mock":
        import mock_measure
        mock_measure.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    _forget()
    measure.clear_caches()


_golden = None


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN, 'rb') as f:
            _golden = pickle.load(f)
    return _golden


def build_psi(rec):
    """The stand-alone ``MPS`` of a recorded state (site tensors with the reference's charge blocks, S, forms)."""
    from tenpy_amd.networks.mps import MPS
    chinfo = ChargeInfo([int(m) for m in rec['chinfo_mod']])
    dtype = np.complex128 if rec['complex'] else np.float64
    Bs = [blocked_array(b, chinfo, dtype) for b in rec['Bs']]
    psi = MPS([B.get_leg('p') for B in Bs], Bs, rec['S'], form='B')
    psi.form = [tuple(f) for f in rec['forms']]
    return psi


class LaunchCounter:
    """Counts the calls of the entry point ``name`` of the installed library object (emulation or ctypes handle)."""

    def __init__(self, monkeypatch, name):
        from tenpy_amd.linalg import _device as dev
        L = dev.lib()
        self.n = 0
        real = getattr(L, name)

        def counted(*args):
            self.n += 1
            return real(*args)

        monkeypatch.setattr(L, name, counted, raising=False)
