"""Generate the mutual-information fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its
``MPS.mutinf_two_site`` (networks/mps.py:4180-4233) and ``MPS.get_rho_segment`` (:3979-4023) return on small states.

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_mutinf.py

Output (committed): ``tests/golden/mutinf.pkl`` -- plain dict / list / numpy content only.  A list of states, each with

* ``Bs``      the stored site tensors ([vL, p, vR]) in the ``blocked_array`` format of ``tests/mpo_cell_fixtures.py``, ``forms``, ``S``
              (L + 1 spectra), ``chinfo_mod``, ``complex``;
* ``mutinf``  {(max_range, n): (coords, mutinf)} for max_range None and 3, n = 1 and 2;
* ``rho2``    {(i, j): ``get_rho_segment([i, j])`` as a dense array [p0, p1, p0*, p1*]} for every pair i < j;
* ``rho1``    the one-site density matrices [p0, p0*], one per site.

States: the XXZ chain L = 8 with Sz conserved in a staggered field, chi <= 16; the same state after three complex TEBD steps; the TFI
chain L = 8 without a charge (one physical sector of width 2); the S = 1 Heisenberg chain L = 6 without a charge (width 3); the
Fermi-Hubbard chain L = 6 with N and Sz conserved (d = 4: ten slots (a >= b) per row)."""
import os
import pickle
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import build_ref  # noqa: E402  (where the reference lives)

sys.path.insert(0, build_ref.reference_root())
os.environ.setdefault('TENPY_NO_CYTHON', '1')
from make_golden_mpo_apply import dense  # noqa: E402
from tenpy.algorithms import dmrg, tebd  # noqa: E402
from tenpy.models.hubbard import FermiHubbardChain  # noqa: E402
from tenpy.models.spins import SpinChain  # noqa: E402
from tenpy.models.tf_ising import TFIChain  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402


def ground_state(M, init, chi=16):
    sites = M.lat.mps_sites()
    psi = MPS.from_product_state(sites, init * (len(sites) // 2), bc='finite')
    eng = dmrg.TwoSiteDMRGEngine(psi, M, {'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'mixer': True, 'max_sweeps': 4,
                                          'min_sweeps': 4, 'max_trunc_err': None})      # (any state will do: Hubbard truncates at 16)
    eng.run()
    return psi


def record(name, psi):
    L = psi.L
    rec = dict(name=name, L=L, chinfo_mod=np.array(psi.chinfo.mod), complex=bool(psi.dtype.kind == 'c'),
               Bs=[dense(psi.get_B(i, None), ['vL', 'p', 'vR']) for i in range(L)], forms=[tuple(f) for f in psi.form],
               S=[np.array(psi.get_SL(i)) for i in range(L)] + [np.array(psi.get_SR(L - 1))], mutinf={}, rho2={}, rho1=[])
    for max_range in (None, 3):
        for n in (1, 2):
            coords, mi = psi.mutinf_two_site(max_range=max_range, n=n)
            rec['mutinf'][(max_range, n)] = (np.array(coords), np.array(mi))
    for i in range(L):
        rec['rho1'].append(np.array(psi.get_rho_segment([i]).itranspose(['p0', 'p0*']).to_ndarray()))
        for j in range(i + 1, L):
            rec['rho2'][(i, j)] = np.array(psi.get_rho_segment([i, j]).itranspose(['p0', 'p1', 'p0*', 'p1*']).to_ndarray())
    print(name, 'chi', psi.chi, 'dtype', psi.dtype, 'd', rec['rho1'][0].shape[0], 'max I', float(np.max(rec['mutinf'][(None, 1)][1])))
    return rec


def main():
    out = []
    L = 8
    hz = 0.5 * (-1.)**np.arange(L)
    xxz = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=hz, conserve='Sz', bc_MPS='finite', sort_charge=True))
    psi = ground_state(xxz, ['up', 'down'])
    assert max(psi.chi) <= 16
    out.append(record('xxz', psi))

    psi_c = psi.copy()           # a quench: the ground state in the staggered field evolves under the chain without it
    xxz0 = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=0., conserve='Sz', bc_MPS='finite', sort_charge=True))
    eng = tebd.TEBDEngine(psi_c, xxz0, {'dt': 0.1, 'order': 2, 'N_steps': 3, 'trunc_params': {'chi_max': 16, 'svd_min': 1.e-10}})
    eng.run()
    assert psi_c.dtype.kind == 'c'
    out.append(record('xxz_tebd', psi_c))

    tfi = TFIChain(dict(L=L, J=1., g=1.3, conserve=None, bc_MPS='finite'))
    out.append(record('tfi', ground_state(tfi, ['up', 'up'])))

    spin1 = SpinChain(dict(L=6, S=1., Jx=1., Jy=1., Jz=1., conserve=None, bc_MPS='finite'))
    out.append(record('spin1', ground_state(spin1, ['up', 'down'])))

    hub = FermiHubbardChain(dict(L=6, t=1., U=2., mu=0., cons_N='N', cons_Sz='Sz', bc_MPS='finite'))
    out.append(record('hubbard', ground_state(hub, ['up', 'down'])))
    return out


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = main()
    path = os.path.join(HERE, 'mutinf.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote mutinf.pkl", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
