"""Helpers of the ``H + h.c.`` tests: MPOs built with ``explicit_plus_hc=True`` (half of the Hamiltonian) and the states of the
stand-alone driver they are tested on -- L = 8 chains after two warm-up sweeps at chi <= 24, shared per backend --, the dense
contraction ``H theta + H^dagger theta`` on the host, and an exact diagonalisation that shares no bookkeeping with the code under test."""
import os
import pickle

import numpy as np

from mpo_entry_fixtures import ebackend, sorted_mpo  # noqa: F401
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.networks.mpo import MPOEnvironment

CASES = ['xxz', 'hubbard', 'hubbardN_real', 'hubbardN', 'xxz_sorted', 'hubbard_sorted']
L = 8
_states = {}


def plus_hc_golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plus_hc.pkl'), 'rb') as f:
        return pickle.load(f)


def make_mpo(name, plus_hc, n=L):
    """The MPO of a case (``_sorted``: bond legs sorted and bunched afterwards), as half of H (``plus_hc``) or in full, and the site leg."""
    base = name.split('_')[0]
    if base == 'xxz':
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        H, p = xxz_chain_mpo(n, 1., 0.7, 0.1, explicit_plus_hc=plus_hc), spin_half_leg('Sz')[1]
    else:
        from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
        conserve = ('N', '2*Sz') if base == 'hubbard' else ('N',)
        H = hubbard_ladder_mpo(n // 2, 1., 4., 0., conserve=conserve, peierls=0. if name.endswith('real') else 0.3, explicit_plus_hc=plus_hc)
        p = spinful_fermion_leg(conserve)[1]
    if name.endswith('sorted'):
        H = sorted_mpo(H)
        H.explicit_plus_hc = plus_hc
    return H, p


def initial_state(name, p, n=L):
    from tenpy_amd.networks.mps import MPS
    return MPS.from_product_state([p] * n, ([1, 0] if name.startswith('xxz') else [1, 2]) * (n // 2))


def model_state(backend, name):
    """``(H, psi, env)``: the half MPO of the case, the state after two sweeps of the stand-alone DMRG on it at chi <= 24 (the
    sorted cases: on the unsorted MPO of the same model) and its environments."""
    key = (backend, name)
    if key not in _states:
        from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
        base = name[:-len('_sorted')] if name.endswith('_sorted') else name
        if (backend, base, 'run') not in _states:
            H, p = make_mpo(base, True)
            psi = initial_state(base, p)
            eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 24, 'svd_min': 1.e-10}, 'lanczos_params': {}})
            for _ in range(2):
                eng.sweep()
            _states[(backend, base, 'run')] = (H, psi, eng.env)
        H, psi, env = _states[(backend, base, 'run')]
        if name != base:
            H = make_mpo(name, True)[0]
            env = MPOEnvironment(psi, H)
        _states[key] = (H, psi, env)
    return _states[key]


def nonsquare_bond(psi, env):
    """A bond ``i0`` (two-site operator on i0, i0 + 1) whose ``LP`` has a block with different extents on its two virtual legs -- a
    charged MPO index between sectors of different size: on square blocks a missing exchange of the virtual legs is invisible."""
    for i0 in sorted(range(1, psi.L - 2), key=lambda i: abs(i - (psi.L // 2 - 1))):
        LP = env.get_LP(i0)
        sh = LP._block_shapes()
        a, b = LP.get_leg_index('vR*'), LP.get_leg_index('vR')
        if np.any(sh[:, a] != sh[:, b]):
            return i0
    raise AssertionError("no bond with a non-square block of LP: the case tests nothing about the exchange of the virtual legs")


def _dense(A, labels):
    return A.transpose(labels).to_ndarray()


def dense_plus_hc(LP, Ws, RP, theta):
    """numpy: ``H theta + H^dagger theta`` for ``theta`` [vL, p.., vR] from ``to_ndarray()`` of the PLAIN tensors, the adjoint as the
    conjugate transpose of the dense operator (no leg bookkeeping shared with the code under test)."""
    lp, rp = _dense(LP, ['vR*', 'wR', 'vR']), _dense(RP, ['wL', 'vL', 'vL*'])        # a w a',  w c' c
    ws = [_dense(W, ['wL', 'wR'] + [l for l in W.get_leg_labels() if l not in ('wL', 'wR')]) for W in Ws]
    x = theta.to_ndarray()
    n = len(ws)
    if n == 2:
        op = np.einsum('aub,uvst,vwxy,wdc->asxcbtyd', lp, ws[0], ws[1], rp, optimize=True)
    elif n == 1:
        op = np.einsum('aub,uvst,vdc->ascbtd', lp, ws[0], rp, optimize=True)
    else:
        op = np.einsum('aub,udc->acbd', lp, rp)
    mat = op.reshape(x.size, x.size)
    return ((mat + mat.conj().T) @ x.reshape(-1)).reshape(x.shape)


def bond_matrix(psi, i, dtype):
    """The bond matrix left of site ``i`` (``diag(S)``) as the vector of a zero-site operator."""
    S = psi.get_SL(i)
    leg = psi.get_B(i, None).get_leg('vL').conj()
    return npc.Array.from_ndarray(np.diag(S).astype(dtype), [leg.conj(), leg], dtype=dtype, labels=['vL', 'vR'])


def operator_and_vector(psi, env, i0, n):
    """The plain stand-alone operator on ``n`` sites at ``i0`` and the state's vector for it."""
    from tenpy_amd.algorithms import mps_common
    if n == 2:
        op = mps_common.TwoSiteH(env, i0, factored=True)
        return op, op.combine_theta(psi.get_theta(i0, n=2))
    if n == 1:
        op = mps_common.OneSiteH(env, i0)
        return op, op.combine_theta(psi.get_theta(i0, n=1))
    op = mps_common.ZeroSiteH(env, i0)
    return op, bond_matrix(psi, i0, op.LP.dtype)


# ---- exact diagonalisation with numpy alone --------------------------------------------------------------------------------------------
def _site_op(op, j, n, fill=None):
    d = op.shape[0]
    mats = [(fill if (fill is not None and l < j) else np.eye(d)) for l in range(n)]
    mats[j] = op
    out = mats[0]
    for m in mats[1:]:
        out = np.kron(out, m)
    return out


def exact_ground_energy(name, n):
    """Lowest eigenvalue of the model of ``make_mpo(name, ...)`` on ``n`` sites in the charge sector of ``initial_state``: operators
    from Kronecker products (fermions: explicit Jordan-Wigner strings), ``numpy.linalg.eigvalsh``."""
    if name.startswith('xxz'):
        Sp = np.array([[0., 0.], [1., 0.]])
        Sz = np.diag([-0.5, 0.5])
        H = np.zeros((2 ** n, 2 ** n))
        for i in range(n - 1):
            pm = _site_op(Sp, i, n) @ _site_op(Sp.T, i + 1, n)
            H += 0.5 * (pm + pm.T) + 0.7 * _site_op(Sz, i, n) @ _site_op(Sz, i + 1, n)
        tot = sum(_site_op(Sz, i, n) for i in range(n))
        H -= 0.1 * tot
        keep = np.abs(np.diag(tot)) < 1e-12
    else:
        from tenpy_amd.models.hubbard import hubbard_ops
        o = hubbard_ops()
        phi = 0. if name.endswith('real') else 0.3
        c = {(j, s): _site_op(o[s], j, n, fill=o['JW']) for j in range(n) for s in ('Cu', 'Cd')}
        H = np.zeros((4 ** n, 4 ** n), dtype=complex)
        for j in range(n):
            H += 4. * _site_op(o['NuNd'], j, n)
            for s in ('Cu', 'Cd'):
                if j % 2 == 0:                      # rung (2x, 2x + 1)
                    hop = c[(j, s)].conj().T @ c[(j + 1, s)]
                    H -= hop + hop.conj().T
                if j + 2 < n:                       # leg y = j % 2: phase exp(+i phi) on y = 0, exp(-i phi) on y = 1
                    hop = np.exp(1j * phi * (1 - 2 * (j % 2))) * (c[(j, s)].conj().T @ c[(j + 2, s)])
                    H -= hop + hop.conj().T
        Nu = np.diag(sum(_site_op(o['Nu'], j, n) for j in range(n)))
        Nd = np.diag(sum(_site_op(o['Nd'], j, n) for j in range(n)))
        keep = (np.abs(Nu - n // 2) < 1e-12) & (np.abs(Nd - n // 2) < 1e-12)
    assert np.abs(H - H.conj().T).max() < 1e-14
    return float(np.linalg.eigvalsh(H[np.ix_(keep, keep)])[0])
