"""Shared helpers of the MPO-application tests: the backend with the emulation of ``tpa_mpo_cell_apply_batch`` stacked on the others,
and the rebuilding of a recorded tensor with the block structure its legs had in the reference."""
import numpy as np
import pytest

from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import LegCharge


def _forget():
    npc.clear_device_caches()
    npc._svd_worksize_cache.clear()     # (per job table; the emulation's work area is not the library's)


def blocked_array(rec, chinfo, dtype):
    """The Array of a fixture record (dense data, charge of every index and ``slices`` per leg) with the charge blocks the reference's
    legs had -- not one block per index, which is what ``LegCharge.from_qflat`` makes of the flat charges."""
    legs = []
    for (q, qc), sl in zip(rec['legs'], rec['slices']):
        q = np.asarray(q).reshape(len(q), -1)
        sl = np.asarray(sl, dtype=np.int64)
        assert sl[0] == 0 and sl[-1] == len(q) and all(np.all(q[a:b] == q[a]) for a, b in zip(sl[:-1], sl[1:]))
        legs.append(LegCharge.from_qind(chinfo, sl, q[sl[:-1]].reshape(len(sl) - 1, chinfo.qnumber), qconj=qc))
    return npc.Array.from_ndarray(rec['data'].astype(dtype), legs, dtype=dtype, qtotal=rec['qtotal'], labels=rec['labels'], cutoff=0.)


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def cbackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point including ``tpa_mpo_cell_apply_batch`` (tests/mock_mpo_cell.py); 'gpu':
    the HIP kernels on an MI355X."""
    from tenpy_amd import _lib
    _forget()
    if request.param == "mock":
        import mock_mpo_cell
        mock_mpo_cell.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    _forget()
