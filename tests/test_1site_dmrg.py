"""The stand-alone single-site DMRG driver (``SingleSiteDMRGEngine``) with the subspace expansion on the device: the reference's own
run sweep by sweep, converged energies against exact values and against the two-site driver, the amplitude schedule, 2D bond matrices
in the MPS while mixing, the checkpoint round trip, the options that raise, and ``explicit_plus_hc`` on the generic route -- on the
emulation and on the GPU.

Golden run (tests/golden/dmrg_1site.pkl, record ``dmrg``; generator tests/golden/make_golden_1site.py): XXZ chain L = 12, chi_max = 24,
svd_min = 1e-8, amplitude 1e-5, decay 2, disable_after 4, six sweeps from a product state; the smallest relative gap at the cut over
all 132 SVD calls is 2.04e-4 (stored, >= 1e-4 asserted by the generator), so the kept subspace is well conditioned and the tolerances of
tests/test_mixer_dmrg.py apply: sweep energies 1e-10 relative, bond dimensions equal, final entropies 1e-8, per-update energies
1e-10 (emulation).  The ladder cuts exactly degenerate pairs in its single-site runs and is tested on convergence instead."""
import os
import pickle

import numpy as np
import pytest

import plus_hc_fixtures as phc
from expand_fixtures import xbackend  # noqa: F401
from tenpy_amd.algorithms import mixer
from tenpy_amd.algorithms.dmrg import SingleSiteDMRGEngine, TwoSiteDMRGEngine
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.truncation import svd_theta
from tenpy_amd.networks.mps import MPS
from test_mixer_dmrg import E_HEISENBERG_L10, PARAMS

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dmrg_1site.pkl'), 'rb') as _f:
    GOLDEN = pickle.load(_f)['dmrg']


def _heisenberg():
    from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
    p = spin_half_leg('Sz')[1]
    return xxz_chain_mpo(10, 1., 1., 0.), MPS.from_product_state([p] * 10, [1, 0] * 5)


def _opts(mix=True, **more):
    opts = {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-12}, 'lanczos_params': {}, 'mixer': mix, 'mixer_params': dict(PARAMS)}
    opts.update(more)
    return opts


def _golden_mpo(rec):
    from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
    from tenpy_amd.networks.mpo import MPO
    m = rec['mpo']
    chinfo = ChargeInfo([int(x) for x in m['chinfo_mod']])
    Ws = [npc.Array.from_ndarray(w['data'], [LegCharge.from_qflat(chinfo, q, qconj=qc) for q, qc in w['legs']], qtotal=w['qtotal'],
                                 labels=w['labels'], cutoff=0.) for w in m['W']]
    H = MPO([W.get_leg('p') for W in Ws], Ws, m['IdL'][0], m['IdR'][-1])
    H.IdL_bonds, H.IdR_bonds = m['IdL'], m['IdR']
    return H, Ws[0].get_leg('p'), m['init']


def test_golden_run_sweep_by_sweep(xbackend):
    rec, = [r for r in GOLDEN if r['name'] == 'xxz']
    assert rec['min_gap'] >= 1.e-4 and rec['n_svd_calls'] == 132 and rec['mixer_gone_after'] == 4 and rec['chi_sweeps'][:3] == [4, 24, 24]
    H, p, state = _golden_mpo(rec)
    assert max(H.chi) == rec['D_mpo'] and str(H.dtype) == rec['dtype']
    psi = MPS.from_product_state([p] * rec['L'], state)
    eng = SingleSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': rec['chi'], 'svd_min': rec['svd_min']}, 'lanczos_params': {},
                                        'mixer_params': dict(rec['mixer_params'])})      # (mixer: on by default)
    n_dev, n_decl = mixer.stats['device_expand'], mixer.stats['expand_declined']
    gone = None
    for s in range(rec['n_sweeps']):
        eng.sweep()
        E, Eref = eng.sweep_stats['E'][-1], rec['E_sweeps'][s]
        print("sweep %d: E = %.14f, golden %.14f, chi %d / %d" % (s, E, Eref, eng.sweep_stats['max_chi'][-1], rec['chi_sweeps'][s]))
        assert abs(E - Eref) <= 1e-10 * abs(Eref), (s, E, Eref)
        assert eng.sweep_stats['max_chi'][-1] == rec['chi_sweeps'][s]
        if eng.mixer is None and gone is None:
            gone = s + 1
    assert gone == rec['mixer_gone_after'] == 4
    # every mixer update on the device route, none declined
    assert mixer.stats['device_expand'] - n_dev == 4 * 2 * (rec['L'] - 1) and mixer.stats['expand_declined'] == n_decl
    np.testing.assert_allclose(psi.entanglement_entropy(), rec['S_ent'], rtol=0, atol=1e-8)
    if xbackend == 'mock':
        np.testing.assert_allclose(eng.update_stats['E_total'], rec['E_updates'], rtol=1e-10, atol=0)


def test_heisenberg_schedule_and_bond_matrices(xbackend):
    H, psi = _heisenberg()
    eng = SingleSiteDMRGEngine(psi, H, _opts('SubspaceExpansion'))
    assert isinstance(eng.mixer, mixer.SubspaceExpansion) and eng.mixer.can_decompose_1site
    L = psi.L
    assert eng.get_sweep_schedule() == [(i, True, (True, False)) for i in range(L - 1)] + [(i, False, (False, True)) for i in range(L - 1, 0, -1)]
    amplitudes, seen_2d = [], False
    for s in range(6):
        assert (eng.mixer is not None) == (s < 4)
        eng.sweep()
        amplitudes.append(None if eng.mixer is None else eng.mixer.amplitude)
        seen_2d = seen_2d or any(isinstance(S, npc.Array) for S in psi._S)
    assert amplitudes == [5.e-6, 2.5e-6, 1.25e-6, None, None, None]
    assert seen_2d and all(isinstance(S, np.ndarray) for S in psi._S)       # 2D bond matrices while mixing, singular values after
    assert eng.update_stats['i0'][:2 * (L - 1)] == list(range(L - 1)) + list(range(L - 1, 0, -1))
    E = eng.sweep_stats['E'][-1]
    print("single-site Heisenberg L = 10: E = %.14f, exact %.14f" % (E, E_HEISENBERG_L10))
    assert abs(E - E_HEISENBERG_L10) < 1.e-8
    assert abs(psi.norm_test() - 1.) < 1.e-10


def test_peierls_ladder_converges_to_the_two_site_energy(xbackend):
    """Hubbard ladder 2 x 3 with (N, 2Sz) and a Peierls phase (complex), chi_max = 64 (the largest possible bond dimension): eight
    single-site sweeps against the stand-alone two-site run of the same model."""
    H, p = phc.make_mpo('hubbard', False, n=6)
    two = TwoSiteDMRGEngine(phc.initial_state('hubbard', p, n=6), H, {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-12}, 'lanczos_params': {}})
    for _ in range(4):
        two.sweep()
    psi = phc.initial_state('hubbard', p, n=6)
    eng = SingleSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-8}, 'lanczos_params': {}, 'mixer_params': dict(PARAMS)})
    n_decl = mixer.stats['expand_declined']
    for _ in range(8):
        eng.sweep()
    E, E2 = eng.sweep_stats['E'][-1], two.sweep_stats['E'][-1]
    print("ladder 2 x 3: single-site E = %.13f, two-site E = %.13f" % (E, E2))
    assert psi.dtype == np.complex128 or H.dtype == np.complex128
    assert abs(E - E2) < 1.e-8
    assert abs(psi.norm_test() - 1.) < 1.e-10
    # (the first update meets a real theta -- a product state -- between complex environments: 'mixed dtypes', the generic route)
    assert mixer.stats['expand_declined'] - n_decl <= 1


def test_without_mixer_is_plain_svd_theta(xbackend, monkeypatch):
    """``mixer=None``: every update decomposes theta with the plain ``svd_theta`` and leaves 1D singular values; from a converged
    state the energy stays."""
    H, psi = _heisenberg()
    eng = SingleSiteDMRGEngine(psi, H, _opts(True))
    for _ in range(3):
        eng.sweep()
    E = eng.sweep_stats['E'][-1]
    plain = SingleSiteDMRGEngine(psi, H, _opts(None))
    assert plain.mixer is None
    import tenpy_amd.algorithms.dmrg as dmrg_mod
    calls = []
    monkeypatch.setattr(dmrg_mod, 'svd_theta', lambda theta, *a, **k: calls.append(theta.get_leg_labels()) or svd_theta(theta, *a, **k))
    n_dev = mixer.stats['device_expand']
    plain.sweep()
    assert len(calls) == 2 * (psi.L - 1) and calls[0] == ['(vL.p0)', 'vR'] and calls[-1] == ['vL', '(p0.vR)']
    assert mixer.stats['device_expand'] == n_dev
    assert all(isinstance(S, np.ndarray) for S in psi._S)
    assert abs(plain.sweep_stats['E'][-1] - E) < 1.e-9


def test_checkpoint_round_trip(xbackend, tmp_path):
    H, psi = _heisenberg()
    eng = SingleSiteDMRGEngine(psi, H, _opts())
    for _ in range(2):
        eng.sweep()
    fn = str(tmp_path / 'ckpt.pkl')
    eng.save_checkpoint(fn)
    res = SingleSiteDMRGEngine.from_checkpoint(fn, H, _opts())
    assert res.sweeps == 2 and isinstance(res.mixer, mixer.SubspaceExpansion)
    assert res.mixer.amplitude == eng.mixer.amplitude == 2.5e-6 and res.mixer.sweep_activated == 0
    for e in (eng, res):
        for _ in range(3):
            e.sweep()
    assert res.mixer is None and eng.mixer is None
    assert abs(res.sweep_stats['E'][-1] - eng.sweep_stats['E'][-1]) < 1.e-10
    eng.save_checkpoint(fn)
    assert SingleSiteDMRGEngine.from_checkpoint(fn, H, _opts()).mixer is None


def test_options_that_raise(xbackend):
    H, psi = _heisenberg()
    with pytest.raises(ValueError):
        SingleSiteDMRGEngine(psi, H, {'shard_matvec': True})
    with pytest.raises(ValueError):
        SingleSiteDMRGEngine(psi, H, {}, orthogonal_to=[psi.copy()])
    with pytest.raises(ValueError):
        SingleSiteDMRGEngine(psi, H, {'mixer': 'DensityMatrixMixer'})
    with pytest.raises(ValueError):
        TwoSiteDMRGEngine(psi, H, {'mixer': 'SubspaceExpansion'})
    with pytest.raises(AssertionError):
        SingleSiteDMRGEngine(psi, H, {'mixer_params': {'amplitude': 2.}})
    assert isinstance(SingleSiteDMRGEngine(psi, H, {}).mixer, mixer.SubspaceExpansion)       # on by default
    assert SingleSiteDMRGEngine(psi, H, {'mixer': None}).mixer is None and TwoSiteDMRGEngine(psi, H, {}).mixer is None


def test_explicit_plus_hc_on_the_generic_route(xbackend):
    """An MPO that holds half of H: the device route declines every mixer update with 'explicit_plus_hc', the reference's statements
    (with the adjoint part stacked) serve it, and the run converges to the energy of the two-site run of the same model."""
    H, p = phc.make_mpo('xxz', True)
    psi = phc.initial_state('xxz', p)
    eng = SingleSiteDMRGEngine(psi, H, _opts())
    why = dict(mixer.stats['why'])
    for _ in range(6):
        eng.sweep()
    n = 4 * 2 * (psi.L - 1)
    got = {k: v - why.get(k, 0) for k, v in mixer.stats['why'].items() if v != why.get(k, 0)}
    assert got == {'explicit_plus_hc': n}
    two = TwoSiteDMRGEngine(phc.initial_state('xxz', p), H, {'trunc_params': {'chi_max': 64, 'svd_min': 1.e-12}, 'lanczos_params': {}})
    for _ in range(4):
        two.sweep()
    E, E2 = eng.sweep_stats['E'][-1], two.sweep_stats['E'][-1]
    print("xxz + h.c.: single-site E = %.13f, two-site E = %.13f" % (E, E2))
    assert abs(E - E2) < 1.e-8
