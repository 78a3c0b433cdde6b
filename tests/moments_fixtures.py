"""Shared helpers of the MPO-moments tests: the backend (every emulated entry point, or the GPU), the recorded cases of
``tests/golden/moments.pkl`` (``make_golden_moments.py``) rebuilt as stand-alone ``MPS`` / ``MPO`` objects, shared per backend, and the
golden tolerance."""
import os
import pickle

import numpy as np
import pytest

from measure_fixtures import build_psi
from mpo_cell_fixtures import _forget, blocked_array
from tenpy_amd.linalg.charges import ChargeInfo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'moments.pkl')
TOL = 1.e-12        # the project's golden tolerance
NAMES = ['xxz', 'hubbard', 'xxz_sorted', 'tfi', 'xxz_tebd', 'neel', 'two_sites']


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def mobackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point (tests/mock_sample.py stacks them all); 'gpu': the HIP kernels on an
    MI355X.  The switches of the route start from their defaults and the counters from zero."""
    from tenpy_amd import _lib
    from tenpy_amd.networks import moments
    _forget()
    if request.param == "mock":
        import mock_sample
        mock_sample.install(monkeypatch)
    else:
        _lib.require_gpu()
    for name in ('TPA_MPO_MOMENTS', 'TPA_MPO_MOMENTS_PAIR'):
        monkeypatch.delenv(name, raising=False)
    moments.reset_stats()
    yield request.param
    _forget()


_golden = None
_cases = {}


def golden():
    global _golden
    if _golden is None:
        with open(GOLDEN, 'rb') as f:
            _golden = {rec['name']: rec for rec in pickle.load(f)}
    return _golden


def case(name, backend):
    """``(rec, psi, H)`` of a recorded case; the tensors are uploaded once per backend."""
    from tenpy_amd.networks.mpo import MPO
    key = (name, backend)
    if key not in _cases:
        rec = golden()[name]
        chinfo = ChargeInfo([int(m) for m in rec['chinfo_mod']])
        psi = build_psi(rec)
        w_dtype = np.complex128 if any(np.iscomplexobj(W['data']) for W in rec['Ws']) else np.float64
        Ws = [blocked_array(W, chinfo, w_dtype) for W in rec['Ws']]
        _cases[key] = (rec, psi, MPO([B.get_leg('p') for B in psi._B], Ws, rec['IdL'], rec['IdR']))
    return _cases[key]


def close(got, want, scale):
    """|got - want| <= TOL max(1, scale)."""
    return abs(got - want) <= TOL * max(1., abs(scale))
