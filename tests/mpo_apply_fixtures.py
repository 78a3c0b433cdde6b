"""Helpers of the block-MPO tests: the backend fixture (emulation incl. the entry points of ``mock_mpo_apply``, or the GPU), the
Hubbard ladder with an N-only physical leg (sectors of widths 1, 2, 1: up and down share a charge block) after two sweeps of the
stand-alone driver, shared per backend, and a counter of the calls of ``tpa_mpo_apply_batch`` that works on both backends."""
import numpy as np
import pytest

from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def bbackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_mpo_apply
        mock_mpo_apply.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


class CallCounter:
    """Counts the calls of one entry point of the installed library object by wrapping it for the duration of a test."""

    def __init__(self, monkeypatch, name='tpa_mpo_apply_batch'):
        self.n = 0
        L = dev.lib()
        real = getattr(L, name)

        def counted(*args):
            self.n += 1
            return real(*args)
        monkeypatch.setattr(L, name, counted, raising=False)


def ladder_engine(Lx, cplx=False, conserve=('N',), chi=32, sweeps=2, U=4.):
    """The stand-alone two-site DMRG engine on the 2 x Lx Hubbard ladder at half filling after ``sweeps`` sweeps."""
    from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
    from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
    from tenpy_amd.networks.mps import MPS
    L = 2 * Lx
    H = hubbard_ladder_mpo(Lx, 1., U, 0., conserve=conserve, peierls=0.3 if cplx else 0.)
    _, p = spinful_fermion_leg(conserve)
    psi = MPS.from_product_state([p] * L, [1, 2] * Lx)
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'lanczos_params': {}})
    for _ in range(sweeps):
        eng.sweep()
    return eng


def bond_tensors(eng, i0):
    return (eng.env.get_LP(i0), eng.env.get_RP(i0 + 1), eng.H.get_W(i0), eng.H.get_W(i0 + 1))


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))
