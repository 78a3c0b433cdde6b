"""Shared fixture of the subspace-expansion tests: the backend with the emulation of ``tpa_mpo_expand_batch`` stacked on the others."""
import pytest

from tenpy_amd.linalg import np_conserved as npc


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def xbackend(request, monkeypatch):
    """'mock': the numpy emulation of every device entry point including ``tpa_mpo_expand_batch`` (tests/mock_expand.py); 'gpu': the
    HIP kernels on an MI355X."""
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_expand
        mock_expand.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()
