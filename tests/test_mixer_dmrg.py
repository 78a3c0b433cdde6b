"""The stand-alone two-site DMRG driver with the density-matrix mixer on (``mixer=True``): energies against the exact value and against
the mixer-off run of the same model, the amplitude schedule and the sweep at which the mixer goes away, 2D bond matrices in the MPS,
the checkpoint round trip, the options that exclude each other -- on the emulation and on the GPU.

Models: the open Heisenberg chain L = 10 with Sz (real; exact ground-state energy from exact diagonalisation, as in ``smoke()``), the
Hubbard ladder 2 x 3 with (N, 2Sz) and a Peierls phase (complex) and the XXZ chain with ``explicit_plus_hc`` (``PlusHcH``: the
mixer takes the plain operator behind it and doubled weights), each against its own mixer-off run at chi_max = 64, where nothing but ``svd_min`` truncates
(the largest possible bond dimension of these chains is 32, 64 and 16): both runs converge to the exact ground state.  Tolerance on
energies: 1e-8 (tests/test_plus_hc_golden.py compares converged energies with 1e-8 as well); on the entropy 1e-5: the entropy is first
order in the error of the state, which is the square root of the error of the energy (<= 1e-10 after four to six sweeps)."""
import numpy as np
import pytest

import plus_hc_fixtures as phc
from mixer_fixtures import mbackend  # noqa: F401
from tenpy_amd.algorithms import mixer
from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
from tenpy_amd.linalg import np_conserved as npc

E_HEISENBERG_L10 = -4.258035207282882
PARAMS = {'amplitude': 1.e-5, 'decay': 2., 'disable_after': 4}


def _model(name):
    if name == 'heisenberg':
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        from tenpy_amd.networks.mps import MPS
        p = spin_half_leg('Sz')[1]
        return xxz_chain_mpo(10, 1., 1., 0.), MPS.from_product_state([p] * 10, [1, 0] * 5)
    if name == 'ladder_complex':
        H, p = phc.make_mpo('hubbard', False, n=6)
        return H, phc.initial_state('hubbard', p, n=6)
    H, p = phc.make_mpo('xxz', True)
    return H, phc.initial_state('xxz', p)


def _engine(name, mix, **more):
    H, psi = _model(name)
    opts = {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-12}, 'lanczos_params': {}, 'mixer': mix, 'mixer_params': dict(PARAMS)}
    opts.update(more)
    return TwoSiteDMRGEngine(psi, H, opts)


@pytest.mark.parametrize("name", ['heisenberg', 'ladder_complex', 'xxz_plus_hc'])
def test_mixer_on_run(mbackend, name):
    eng = _engine(name, True)
    n_dev, n_decl = mixer.stats['device_mix_rho'], mixer.stats['declined']
    amplitudes, seen_2d = [], False
    for s in range(6):
        assert (eng.mixer is not None) == (s < 4)
        eng.sweep()
        amplitudes.append(None if eng.mixer is None else eng.mixer.amplitude)
        seen_2d = seen_2d or any(isinstance(S, npc.Array) for S in eng.psi._S)
    # amplitude / decay after every sweep; gone after `disable_after` = 4 sweeps (reference update_amplitude :1626-1653)
    assert amplitudes == [5.e-6, 2.5e-6, 1.25e-6, None, None, None]
    assert seen_2d and all(isinstance(S, np.ndarray) for S in eng.psi._S)       # 2D bond matrices while mixing, singular values after
    n_updates = 4 * 2 * (eng.psi.L - 2)
    assert mixer.stats['device_mix_rho'] - n_dev == n_updates and mixer.stats['declined'] == n_decl      # every mixer update on the device route
    plain = _engine(name, None)
    for s in range(4):
        plain.sweep()
    E, E_plain = eng.sweep_stats['E'][-1], plain.sweep_stats['E'][-1]
    print(name, "E mixer %.12f plain %.12f; S %.10f %.10f" % (E, E_plain, eng.sweep_stats['S'][-1], plain.sweep_stats['S'][-1]))
    assert abs(E - E_plain) < 1.e-8
    assert abs(eng.sweep_stats['S'][-1] - plain.sweep_stats['S'][-1]) < 1.e-5
    if name == 'heisenberg':
        assert abs(E - E_HEISENBERG_L10) < 1.e-8
        # what the mixer is for: it populates the charge sectors in the first sweep, where the plain run cannot grow them yet
        assert abs(eng.sweep_stats['E'][0] - E_HEISENBERG_L10) < abs(plain.sweep_stats['E'][0] - E_HEISENBERG_L10)
    assert abs(eng.psi.norm_test() - 1.) < 1.e-10


def test_mixer_checkpoint_round_trip(mbackend, tmp_path):
    """Resume data carries the mixer's amplitude and activation sweep: a resumed engine continues the schedule and the energies."""
    eng = _engine('heisenberg', 'DensityMatrixMixer')
    for _ in range(2):
        eng.sweep()
    fn = str(tmp_path / 'ckpt.pkl')
    eng.save_checkpoint(fn)
    H, _ = _model('heisenberg')
    opts = {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-12}, 'lanczos_params': {}, 'mixer': True, 'mixer_params': dict(PARAMS)}
    res = TwoSiteDMRGEngine.from_checkpoint(fn, H, opts)
    assert res.sweeps == 2 and res.mixer is not None
    assert res.mixer.amplitude == eng.mixer.amplitude == 2.5e-6 and res.mixer.sweep_activated == 0
    for e in (eng, res):
        for _ in range(3):
            e.sweep()
    assert res.mixer is None and eng.mixer is None
    assert abs(res.sweep_stats['E'][-1] - eng.sweep_stats['E'][-1]) < 1.e-10
    # a checkpoint written after the mixer went away resumes without one
    eng.save_checkpoint(fn)
    assert TwoSiteDMRGEngine.from_checkpoint(fn, H, opts).mixer is None


def test_mixer_options(mbackend):
    H, psi = _model('heisenberg')
    with pytest.raises(ValueError):
        TwoSiteDMRGEngine(psi, H, {'mixer': True, 'shard_matvec': True})
    with pytest.raises(ValueError):
        TwoSiteDMRGEngine(psi, H, {'mixer': 'SubspaceExpansion'})
    assert TwoSiteDMRGEngine(psi, H, {}).mixer is None and TwoSiteDMRGEngine(psi, H, {'mixer': None}).mixer is None
    # a step of chi_list switches the mixer on again (default), or not
    for again in (True, False):
        eng = _engine('heisenberg', True, chi_list={0: 8, 3: 16}, chi_list_reactivates_mixer=again,
                      mixer_params=dict(PARAMS, disable_after=2))
        for _ in range(3):
            eng.sweep()
        assert eng.mixer is None
        eng.sweep()
        assert (eng.mixer is not None) == again
        if again:
            assert eng.mixer.sweep_activated == 3 and eng.mixer.amplitude == 5.e-6


def test_mixer_publishes_no_svd_hint(mbackend, monkeypatch):
    """No SVD warm-start hint on mixer updates (the decomposition is two ``eigh``)."""
    eng = _engine('heisenberg', True)
    hints = []
    orig = eng.mixer.mix_and_decompose_2site

    def spy(*a, **k):
        hints.append(npc.svd_hint)
        return orig(*a, **k)
    eng.mixer.mix_and_decompose_2site = spy
    eng.sweep()
    assert len(hints) == 16 and all(h is None for h in hints)


def test_mps_with_2d_bond_matrix(mbackend):
    """``set_SR`` keeps a 2D Array; ``_scaled`` multiplies by it for power +1 and raises otherwise; ``chi`` and the entropy read it."""
    eng = _engine('heisenberg', None)
    for _ in range(2):
        eng.sweep()
    psi = eng.psi
    i = 4
    S = psi.get_SR(i)
    want_S, want_theta = psi.entanglement_entropy()[i], psi.get_theta(i, n=2).to_ndarray()
    leg = psi.get_B(i, None).get_leg('vR')
    rng = np.random.default_rng(3)
    # S -> Q diag(S) with a block-diagonal orthogonal Q absorbed into the tensor on the left: the same state
    Q = npc.Array.from_func_square(lambda sh: np.linalg.qr(rng.standard_normal(sh))[0], leg.conj(), labels=['vL', 'vR'])
    A = psi.get_B(i, 'A')
    psi.set_B(i, npc.tensordot(A, Q.conj().itranspose().ireplace_labels(['vR*', 'vL*'], ['vL', 'vR']), axes=['vR', 'vL']), form='A')
    psi.set_SR(i, Q.scale_axis(S, 'vR'))
    assert isinstance(psi.get_SR(i), npc.Array) and psi.chi[i] == len(S)
    assert abs(psi.entanglement_entropy()[i] - want_S) < 1.e-12
    got = psi.get_theta(i, n=2).to_ndarray()
    assert np.abs(got - want_theta).max() < 1.e-13
    with pytest.raises(ValueError):
        psi.get_B(i, 'C')               # needs the square root of the bond matrix


def _golden_dmrg():
    import os
    import pickle
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mixer.pkl'), 'rb') as f:
        return pickle.load(f)['dmrg']


@pytest.mark.parametrize("name", ['xxz', 'peierls_ladder', 'xxz_plus_hc'])
def test_mixer_dmrg_golden(mbackend, name):
    """The reference's own mixer-on runs (tests/golden/mixer.pkl, record ``dmrg``: amplitude 1e-5, decay 2, disable_after 4, six sweeps,
    chi_max 24 from a product state) sweep by sweep, with the tolerances of tests/test_plus_hc_golden.py: sweep energies 1e-10
    relative, bond dimensions equal, final entropies 1e-8, per-update energies 1e-10 (emulation); and the sweep after which the
    mixer is gone."""
    from tenpy_amd.networks.mps import MPS
    rec = [r for r in _golden_dmrg() if r['name'] == name][0]
    par, hc = rec['params'], rec['explicit_plus_hc']
    if rec['kind'] == 'xxz':        # the reference's own MPO tensors: the perturbation depends on the representation (generator docstring)
        from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
        from tenpy_amd.networks.mpo import MPO
        m = rec['mpo']
        chinfo = ChargeInfo([int(x) for x in m['chinfo_mod']])
        Ws = [npc.Array.from_ndarray(w['data'], [LegCharge.from_qflat(chinfo, q, qconj=qc) for q, qc in w['legs']], qtotal=w['qtotal'],
                                     labels=w['labels'], cutoff=0.) for w in m['W']]
        n = rec['L']
        H = MPO([W.get_leg('p') for W in Ws], Ws, m['IdL'][0], m['IdR'][-1], explicit_plus_hc=hc)
        H.IdL_bonds, H.IdR_bonds = m['IdL'], m['IdR']
        p, state = Ws[0].get_leg('p'), m['init']
    else:
        from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
        n = 2 * rec['L']
        H = hubbard_ladder_mpo(rec['L'], par['t'], par['U'], par['mu'], peierls=par['peierls'], explicit_plus_hc=hc)
        p, state = spinful_fermion_leg()[1], [1, 2] * (n // 2)
    assert max(H.chi) == rec['D_mpo'] and str(H.dtype) == rec['dtype']
    psi = MPS.from_product_state([p] * n, state)
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': rec['chi'], 'svd_min': rec['svd_min']}, 'lanczos_params': {}, 'mixer': True,
                                     'mixer_params': dict(rec['mixer_params'])})
    gone = None
    for s in range(rec['n_sweeps']):
        eng.sweep()
        E, Eref = eng.sweep_stats['E'][-1], rec['E_sweeps'][s]
        print("%s sweep %d: E = %.14f, golden %.14f, chi %d / %d" % (name, s, E, Eref, eng.sweep_stats['max_chi'][-1], rec['chi_sweeps'][s]))
        assert abs(E - Eref) <= 1e-10 * abs(Eref), (s, E, Eref)
        assert eng.sweep_stats['max_chi'][-1] == rec['chi_sweeps'][s]
        if eng.mixer is None and gone is None:
            gone = s + 1
    assert gone == rec['mixer_gone_after'] == 4
    np.testing.assert_allclose(psi.entanglement_entropy(), rec['S_ent'], rtol=0, atol=1e-8)
    if mbackend == 'mock':
        np.testing.assert_allclose(eng.update_stats['E_total'], rec['E_updates'], rtol=1e-10, atol=1e-10)
