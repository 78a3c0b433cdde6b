"""Evolution through the three effective Hamiltonians at scale, on the MI355X: the XXZ L=32, chi=128 state that the stand-alone DMRG
driver grows in ``tests/test_midsize_golden.py`` (same construction, parameters of ``midsize.pkl``), made complex by two two-site
TDVP steps and brought into mixed canonical form around the middle site by the right-moving half of a third; there one two-site, one
one-site and one zero-site evolution by ``delta = -0.025j``:

* the native route is taken (``krylov_based.stats``);
* the result equals that of the step-by-step route (``krylov_based.NATIVE`` off: ``_build_krylov`` + ``_calc_result_full``) within
  ``1e-12 |theta|`` elementwise with equal ``N``;
* round trip ``U(-delta) U(delta) theta`` and norm drift (``normalize=False``) within ``1e-12 |theta|``, the class of
  ``tests/test_lanczos_evolution_native.py``."""
import numpy as np
import pytest

from helpers import golden
from tdvp_fixtures import note_parity
from tenpy_amd.algorithms import mps_common
from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
from tenpy_amd.algorithms.tdvp import TwoSiteTDVPEngine
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
from tenpy_amd.networks.mpo import MPOEnvironment
from tenpy_amd.networks.mps import MPS

pytestmark = pytest.mark.gpu
DELTA = -0.025j


def _check(name, H, theta, monkeypatch):
    n0 = npc.norm(theta)
    res = {}
    for native in (True, False):
        monkeypatch.setattr(kb, 'NATIVE', native)
        before = kb.stats['n_native_evolve']
        res[native] = kb.LanczosEvolution(H, theta, {}).run(DELTA, normalize=False)
        assert kb.stats['n_native_evolve'] - before == int(native), name
    monkeypatch.setattr(kb, 'NATIVE', True)
    (a, Na), (b, Nb) = res[True], res[False]
    diff = np.abs(a.to_ndarray() - b.to_ndarray()).max() / n0
    back, Nback = kb.LanczosEvolution(H, a, {}).run(-DELTA, normalize=False)
    rt = np.linalg.norm(back.to_ndarray() - theta.to_ndarray()) / n0
    drift = abs(npc.norm(a) - n0) / n0
    note_parity("gpu xxz_L32_chi128 %s (n = %d): native vs step-by-step %.3g, round trip %.3g, norm drift %.3g, N = %d, %d, %d" % (
        name, theta._arena.numel(), diff, rt, drift, Na, Nb, Nback))
    assert Na == Nb
    assert diff <= 1e-12 and rt <= 1e-12 and drift <= 1e-12


def test_three_operators_at_chi128(monkeypatch):
    from tenpy_amd import _lib
    _lib.require_gpu()
    npc.clear_device_caches()
    rec = golden('midsize.pkl')['xxz_L32_chi128']
    L = rec['L']
    H = xxz_chain_mpo(L, 1., 1., 0.)
    _, p = spin_half_leg('Sz')
    psi = MPS.from_product_state([p] * L, [1, 0] * (L // 2))
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': rec['chi'], 'svd_min': 1.e-10}})
    for _ in rec['E_sweeps']:
        eng.sweep()
    assert max(psi.chi) == rec['chi_final']
    tdvp = TwoSiteTDVPEngine(psi, H, {'dt': 0.05, 'N_steps': 2, 'trunc_params': {'chi_max': rec['chi'], 'svd_min': 1.e-10}})
    tdvp.run()
    mid = L // 2
    for i0 in range(mid):               # sites < mid in form A, site mid in form Th, sites > mid in form B
        tdvp.update_local(i0, True)
    assert psi.get_B(mid, None).dtype == np.complex128 and max(psi.chi) == rec['chi']
    psi.dtype = np.dtype(np.complex128)
    env = MPOEnvironment(psi, H)        # grown from the A tensors on the left and the B tensors on the right: all complex
    H2 = mps_common.TwoSiteH(env, mid, combine=True)
    _check('two-site', H2, H2.combine_theta(psi.get_theta(mid, n=2)), monkeypatch)
    H1 = mps_common.OneSiteH(env, mid)
    theta1 = psi.get_theta(mid, n=1)
    assert H1.factored
    _check('one-site', H1, theta1, monkeypatch)
    # the bond matrix right of site mid, as SingleSiteTDVPEngine.right_moving_update makes it
    U, S, VH = npc.svd(theta1.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0), qtotal_LR=[theta1.qtotal, None], inner_labels=['vR', 'vL'])
    psi.set_B(mid, U.split_legs(['(vL.p0)']).replace_label('p0', 'p'), form='A')
    psi.set_SR(mid, S)
    env.invalidate(mid, mid, keep_LP=True, keep_RP=True)
    H0 = mps_common.ZeroSiteH(env, mid + 1)
    assert H0.factored
    _check('zero-site', H0, VH.scale_axis(S, 'vL'), monkeypatch)
    npc.clear_device_caches()
