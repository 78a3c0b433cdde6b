"""The stand-alone drivers on MPOs built with ``explicit_plus_hc=True`` against what the reference's engines produce for the same
models (``tests/golden/plus_hc.pkl``, written by ``tests/golden/make_golden_plus_hc.py``): two-site DMRG on the XXZ chain L = 16 and on
the Fermi-Hubbard ladder 2 x 4 with a Peierls phase (complex MPO that is not Hermitian) at chi = 32, and three steps of two-site TDVP.
The effective Hamiltonians are the doubled device operators (``plus_hc``), in the ``LHeff . theta . RHeff`` form that the driver chooses
for sectors this small and with the factored form forced on.

Tolerances: those of ``tests/test_dmrg_golden.py`` (sweep energies 1e-10 relative, bond dimensions equal, entropies 1e-8) and of
``tests/test_tdvp_golden.py`` (bond dimensions equal, entropies 1e-10, ``psi.norm`` 1e-12)."""
import numpy as np
import pytest

from plus_hc_fixtures import ebackend, plus_hc_golden  # noqa: F401
from tenpy_amd.algorithms import mps_common
from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
from tenpy_amd.algorithms.tdvp import TwoSiteTDVPEngine
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.networks.mps import MPS


def _model(rec, dtype=None):
    par = rec['params']
    if rec['name'] == 'xxz':
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        n = rec['L']
        H, p = xxz_chain_mpo(n, par['Jxx'], par['Jz'], par['hz'], explicit_plus_hc=True), spin_half_leg('Sz')[1]
        state = [1, 0] * (n // 2)              # up, down, ... (index 1 = up)
    else:
        from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
        n = 2 * rec['L']
        H = hubbard_ladder_mpo(rec['L'], par['t'], par['U'], par['mu'], peierls=par['peierls'], explicit_plus_hc=True)
        p = spinful_fermion_leg()[1]
        state = [1, 2] * (n // 2)              # up, down, ...
    assert rec['init'] == ['up', 'down'] and H.explicit_plus_hc
    kwargs = {} if dtype is None else {'dtype': dtype}
    return H, MPS.from_product_state([p] * n, state, **kwargs)


def _spy(monkeypatch):
    """Which operators the driver built: (class of the operator handed to the Krylov loop, factored?)."""
    from tenpy_amd.algorithms import dmrg
    seen = []
    orig = dmrg._plus_hc

    def spy(eff_H):
        res = orig(eff_H)
        seen.append((type(res).__name__, type(eff_H).__name__, bool(getattr(eff_H, 'factored', False))))
        return res
    monkeypatch.setattr(dmrg, '_plus_hc', spy)
    from tenpy_amd.algorithms import tdvp
    monkeypatch.setattr(tdvp, '_plus_hc', spy)
    return seen


@pytest.mark.parametrize("factored", [False, True], ids=['fused', 'factored'])
@pytest.mark.parametrize("name", ['xxz', 'peierls_ladder'])
def test_dmrg_golden(ebackend, monkeypatch, name, factored):
    rec = [r for r in plus_hc_golden()['dmrg'] if r['name'] == name][0]
    if factored:
        monkeypatch.setattr(mps_common, 'FACTORED_MIN_SECTOR', 0)
    seen = _spy(monkeypatch)
    H, psi = _model(rec)
    assert max(H.chi) == rec['D_mpo'] and str(H.dtype) == rec['dtype']
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': rec['chi'], 'svd_min': 1.e-10}, 'lanczos_params': {}})
    n_sweeps = rec['n_sweeps'] if ebackend == 'mock' else 3          # (the device: three sweeps)
    for s in range(n_sweeps):
        eng.sweep()
        E, Eref = eng.sweep_stats['E'][-1], rec['E_sweeps'][s]
        print("%s sweep %d: E = %.14f, golden %.14f" % (name, s, E, Eref))
        assert abs(E - Eref) <= 1e-10 * abs(Eref), (s, E, Eref)
        assert eng.sweep_stats['max_chi'][-1] == rec['chi_sweeps'][s]
    if n_sweeps == rec['n_sweeps']:
        np.testing.assert_allclose(psi.entanglement_entropy(), rec['S_ent'], rtol=0, atol=1e-8)
    if ebackend == 'mock':
        np.testing.assert_allclose(eng.update_stats['E_total'], rec['E_updates'], rtol=1e-10, atol=1e-10)
    assert seen and all(kind == 'PlusHcH' and f is factored for kind, _, f in seen), "every bond ran on the doubled operator"


@pytest.mark.parametrize("name", ['xxz', 'peierls_ladder'])
def test_tdvp_golden(ebackend, monkeypatch, name):
    rec = [r for r in plus_hc_golden()['tdvp'] if r['name'] == name][0]
    monkeypatch.setattr(mps_common, 'FACTORED_MIN_SECTOR', 0)
    seen = _spy(monkeypatch)
    H, psi = _model(rec, dtype=np.complex128)
    eng = TwoSiteTDVPEngine(psi, H, {'dt': rec['dt'], 'N_steps': 1, 'trunc_params': {'chi_max': rec['chi_max'], 'svd_min': rec['svd_min']}})
    before = kb.stats['n_native_evolve']
    for step in range(rec['n_steps']):
        eng.run()
        assert list(psi.chi) == list(rec['chi'][step]), "step %d" % step
        dS = np.abs(psi.entanglement_entropy() - rec['S'][step]).max()
        print("%s step %d: max |S - golden| = %.3g, |norm - golden| = %.3g" % (name, step, dS, abs(psi.norm - rec['norm'][step])))
        np.testing.assert_allclose(psi.entanglement_entropy(), rec['S'][step], rtol=0, atol=1e-10)
        assert abs(psi.norm - rec['norm'][step]) <= 1e-12
    assert seen and all(kind == 'PlusHcH' for kind, _, _ in seen)
    assert {cls for _, cls, _ in seen} == {'TwoSiteH', 'OneSiteH'}
    assert kb.stats['n_native_evolve'] > before, "evolutions ran in the native loop on the doubled operators"
