"""Helpers of the TDVP tests: the backend fixture (emulation incl. the entry points of ``mock_evolve``, or the GPU) and the
records of ``tests/golden/tdvp.pkl`` as device objects."""
import os

import numpy as np
import pytest

from helpers import golden, load_array
from tenpy_amd.algorithms import mps_common

_cache = {}


def tdvp_golden():
    if 'g' not in _cache:
        _cache['g'] = golden('tdvp.pkl')
    return _cache['g']


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def zbackend(request, monkeypatch):
    from tenpy_amd import _lib
    from tenpy_amd.linalg import np_conserved as npc
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_evolve
        mock_evolve.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


def operator_record(model, op):
    return [r for r in tdvp_golden()['operators'] if r['model'] == model and r['op'] == op][0]


def build_operator(rec, factored=True):
    """``(H, theta)`` on the device from a dumped operator: the stand-alone classes built from explicit tensors."""
    LP, RP, theta = load_array(rec['LP']), load_array(rec['RP']), load_array(rec['theta'])
    if rec['op'] == 'two':
        H = mps_common.TwoSiteH(None, rec['i0'], tensors=(LP, RP, load_array(rec['W0']), load_array(rec['W1'])), factored=factored)
        assert H.factored == factored
        return H, H.combine_theta(theta)
    if rec['op'] == 'one':
        H = mps_common.OneSiteH.from_LP_W0_RP(LP, load_array(rec['W0']), RP, i0=rec['i0'])
    else:
        H = mps_common.ZeroSiteH.from_LP_RP(LP, RP, i0=rec['i0'])
    assert H.factored
    return H, theta


def dense_like(a, rec_array):
    """``a`` as a dense array in the leg order of a dumped Array (fused two-site vectors are split first)."""
    if a.rank == 2 and len(rec_array['labels']) == 4:
        a = a.split_legs()
    return a.transpose(rec_array['labels']).to_ndarray()


def note_parity(line):
    """Measured parity figures: printed, and appended to the file ``TPA_PARITY_FILE`` names (how ``profiles/tdvp_parity.txt`` is made)."""
    print(line)
    path = os.environ.get('TPA_PARITY_FILE')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')
