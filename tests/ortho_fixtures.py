"""Helpers of the projected-Lanczos tests: the backend fixture (emulation incl. the entry points of ``mock_ortho``, or the GPU),
converged engines shared per backend, and generic vectors on a given block structure."""
import numpy as np
import pytest

from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def obackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_ortho
        mock_ortho.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


def random_like(theta, rng, cplx=None):
    """A generic vector on the block structure (and with the legs) of ``theta``."""
    cplx = (theta.dtype == np.complex128) if cplx is None else cplx
    n = theta._arena.numel()
    v = theta.astype(np.complex128) if cplx and theta.dtype != np.complex128 else theta.copy(deep=True)
    data = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.)
    v._arena = dev.to_device(data)
    return v


def inner(a, b):
    return npc.inner(a, b, axes='range', do_conj=True)
