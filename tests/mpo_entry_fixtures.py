"""Helpers of the entry-MPO tests: the backend fixture (emulation incl. the entry points of ``mock_mpo_entry``, or the GPU) and the two
kinds of MPO that ``MpoEntryApplyPlan`` serves -- MPOs whose bond legs are sorted and bunched (blocks wider than 1) and a Bose-Hubbard
chain whose physical sectors are wider than ``TPA_MPO_APPLY_MAXD`` in the two-site product -- with the states of the stand-alone driver
they are tested on, shared per backend."""
import numpy as np
import pytest

from mpo_apply_fixtures import CallCounter, rel_err  # noqa: F401
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks.mpo import MPO, MPOEnvironment, mpo_from_dense

ENTRY = 'tpa_mpo_entry_apply_batch'


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def ebackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_mpo_entry
        mock_mpo_entry.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


def sorted_mpo(H):
    """``H`` with every MPO bond leg sorted by charge and bunched: the same permutation on ``wR`` of site i and ``wL`` of site i + 1.
    The boundary legs have one index, so ``IdL`` / ``IdR`` keep their values.  At least one bond block must come out wider than 1."""
    chinfo = H.chinfo
    perms, legs = [], []
    for j in range(H.L + 1):
        leg = H.get_W(j).get_leg('wL') if j < H.L else H.get_W(H.L - 1).get_leg('wR').conj()
        q = leg.to_qflat()
        perm = np.lexsort(q.T) if chinfo.qnumber else np.arange(leg.ind_len)
        _, new = LegCharge.from_qflat(chinfo, q[perm], qconj=leg.qconj).bunch()
        perms.append(perm)
        legs.append(new)
    Ws = []
    for i in range(H.L):
        W = H.get_W(i)
        dense = W.transpose(['wL', 'wR', 'p', 'p*']).to_ndarray()[perms[i]][:, perms[i + 1]]
        Ws.append(npc.Array.from_ndarray(dense, [legs[i], legs[i + 1].conj(), W.get_leg('p'), W.get_leg('p*')], dtype=W.dtype,
                                         qtotal=W.qtotal, labels=['wL', 'wR', 'p', 'p*']))
    assert len(perms[0]) == 1 and len(perms[-1]) == 1
    assert max(int(np.max(leg.get_block_sizes())) for leg in legs) > 1, "no bond block wider than 1: nothing to test"
    return MPO(H.p_legs, Ws, H.IdL, H.IdR)


def boson_leg(Nmax=9):
    """Boson site with ``Nmax + 1`` states and parity conserved, the even occupations first: two sectors of (Nmax + 1) / 2 states.
    Returns (chinfo, leg, occupation of every index)."""
    chinfo = ChargeInfo([2], ['parity_N'])
    occ = np.array([n for n in range(Nmax + 1) if n % 2 == 0] + [n for n in range(Nmax + 1) if n % 2 == 1])
    n_even = (Nmax + 2) // 2
    leg = LegCharge.from_qind(chinfo, [0, n_even, Nmax + 1], [[0], [1]])
    return chinfo, leg, occ


def bose_hubbard_mpo(L, Nmax=9, t=1., U=2., mu=0.5):
    """``H = -t sum (b+_i b_{i+1} + h.c.) + U/2 sum n (n - 1) - mu sum n`` with parity conserved, through ``mpo_from_dense``."""
    chinfo, p, occ = boson_leg(Nmax)
    d = Nmax + 1
    b = np.zeros((d, d))
    for k, n in enumerate(occ):          # b |n> = sqrt(n) |n - 1>
        if n > 0:
            b[list(occ).index(n - 1), k] = np.sqrt(n)
    n_op = np.diag(occ.astype(float))
    W = np.zeros((4, 4, d, d))
    W[0, 0] = W[3, 3] = np.eye(d)
    W[0, 1], W[0, 2] = b.T, b
    W[0, 3] = 0.5 * U * n_op @ (n_op - np.eye(d)) - mu * n_op
    W[1, 3], W[2, 3] = -t * b, -t * b.T
    Ws = [W[0:1] if i == 0 else (W[:, 3:4] if i == L - 1 else W) for i in range(L)]
    return mpo_from_dense(Ws, [p] * L, chinfo), p, occ


_states = {}


def model_state(backend, name):
    """``(H, psi, env)`` of a named input after two sweeps of the stand-alone two-site DMRG at chi <= 32 (with the UNSORTED MPO for
    the sorted inputs: ``env`` is then the environment of the same state with the sorted MPO), shared per backend.
    Names: 'xxz', 'xxz_sorted', 'ladder', 'ladder_sorted', 'ladder_sorted_complex', 'bosons'."""
    key = (backend, name)
    if key in _states:
        return _states[key]
    from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
    from tenpy_amd.networks.mps import MPS
    base = name.split('_')[0]
    pkey = ('plain', backend, base, name.endswith('complex'))
    if pkey not in _states:
        if base == 'xxz':
            from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
            L = 8
            H = xxz_chain_mpo(L, 1., 0.7, 0.1)
            psi = MPS.from_product_state([spin_half_leg('Sz')[1]] * L, [1, 0] * (L // 2))
        elif base == 'ladder':
            from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
            L = 6
            H = hubbard_ladder_mpo(3, 1., 4., 0., conserve=('N', '2*Sz'), peierls=0.3 if name.endswith('complex') else 0.)
            psi = MPS.from_product_state([spinful_fermion_leg(('N', '2*Sz'))[1]] * L, [1, 2] * 3)
        else:
            L = 6
            H, p, occ = bose_hubbard_mpo(L)
            psi = MPS.from_product_state([p] * L, [list(occ).index(n) for n in [1, 2] * (L // 2)])
        eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 32 if base != 'bosons' else 16, 'svd_min': 1.e-10},
                                         'lanczos_params': {}})
        for _ in range(2):
            eng.sweep()
        _states[pkey] = (H, psi, eng.env)
    H, psi, env = _states[pkey]
    if 'sorted' in name:
        H = sorted_mpo(H)
        env = MPOEnvironment(psi, H)
    _states[key] = (H, psi, env)
    return _states[key]


def plain_of(backend, name):
    """``(H, psi, env)`` with the unsorted MPO for the state of a sorted input."""
    model_state(backend, name)
    return _states[('plain', backend, name.split('_')[0], name.endswith('complex'))]


def bond_tensors(H, env, i0):
    return (env.get_LP(i0), env.get_RP(i0 + 1), H.get_W(i0), H.get_W(i0 + 1))
