"""Generate the fixtures of the MPO moments from the REFERENCE implementation (TeNPy, pure-Python path): what its
``MPO.expectation_value`` and ``MPO.variance`` (networks/mpo.py:1111-1171, :1296-1342) return on small states.

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_moments.py

Output (committed): ``tests/golden/moments.pkl`` -- plain dict / list / numpy content only.  A list of cases, each with

* ``Bs``   the stored site tensors ([vL, p, vR]) and ``Ws`` the MPO tensors ([wL, wR, p, p*]) as dense arrays with the charges of every
           index and the block boundaries of every leg (the ``blocked_array`` format of ``tests/mpo_cell_fixtures.py``), ``forms``,
           ``S`` (L + 1 spectra), ``IdL`` / ``IdR`` (the index on the first and behind the last bond), ``chinfo_mod``, ``complex``;
* ``E``    ``H.expectation_value(psi)``, ``H2`` = ``H.variance(psi, 0.)``, ``var`` = ``H.variance(psi)``.

Cases (small: the sizes at which each plan and edge can still go wrong):

(a) ``xxz``         XXZ chain in a staggered field, Sz conserved, L = 6, chi <= 8: the state after two sweeps for the chain WITHOUT the
                    field (at L = 6 two sweeps at chi = 8 converge, and the variance of an eigenstate is a cancellation down to
                    rounding), measured with the MPO of the chain in the field, so that the variance is of order one: the scalar plan;
(b) ``hubbard``     Fermi-Hubbard chain with only N conserved, L = 4: a physical sector two states wide, the block plan;
(c) ``xxz_sorted``  the state of (a) with the MPO's bond legs sorted by charge and bunched: bond blocks wider than 1, the entry plan;
(d) ``tfi``         transverse-field Ising chain without a charge, L = 6 (entry plan where it is allowed, else a decline);
(e) ``xxz_tebd``    the state of (a) after three complex TEBD steps: complex tensors;
(f) ``neel``        the Neel product state with the MPO of (a): every block 1 x 1;
(g) ``two_sites``   the XXZ chain with L = 2 in a singlet: a first and a last site and nothing between them."""
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


def two_sweeps(M, init, chi=8):
    sites = M.lat.mps_sites()
    psi = MPS.from_product_state(sites, (init * len(sites))[:len(sites)], bc='finite')
    dmrg.TwoSiteDMRGEngine(psi, M, {'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'mixer': True, 'max_sweeps': 2,
                                    'min_sweeps': 2, 'max_trunc_err': None}).run()
    return psi


def record(name, psi, H):
    E, H2, var = H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi)
    rec = dict(name=name, L=psi.L, chinfo_mod=np.array(psi.chinfo.mod), complex=bool(np.result_type(psi.dtype, H.dtype).kind == 'c'),
               Bs=[dense(psi.get_B(i, None), ['vL', 'p', 'vR']) for i in range(psi.L)], forms=[tuple(f) for f in psi.form],
               S=[np.array(psi.get_SL(i)) for i in range(psi.L)] + [np.array(psi.get_SR(psi.L - 1))],
               Ws=[dense(H.get_W(i), ['wL', 'wR', 'p', 'p*']) for i in range(H.L)],
               IdL=int(H.get_IdL(0)), IdR=int(H.get_IdR(H.L - 1)), E=np.array(E), H2=np.array(H2), var=np.array(var))
    print("%-11s L=%d chi=%s D=%s E=%.12g H2=%.12g var=%.6g" % (name, psi.L, psi.chi, H.chi, np.real(E), np.real(H2), np.real(var)))
    return rec


def xxz(L, hz=0.5):
    return SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=hz * (-1.)**np.arange(L), conserve='Sz', bc_MPS='finite', sort_charge=True))


def main():
    out = []
    M = xxz(6)
    psi = two_sweeps(xxz(6, 0.), ['up', 'down'], chi=8)
    assert max(psi.chi) <= 8
    out.append(record('xxz', psi, M.H_MPO))
    assert abs(out[-1]['var']) > 1.e-3, "case (a) must not be converged"

    hub = FermiHubbardChain(dict(L=4, t=1., U=4., mu=0., cons_N='N', cons_Sz=None, bc_MPS='finite'))
    out.append(record('hubbard', two_sweeps(hub, ['up', 'down']), hub.H_MPO))
    assert max(np.max(np.diff(W['slices'][2])) for W in out[-1]['Ws']) == 2

    Hs = M.H_MPO.copy()
    Hs.sort_legcharges()
    out.append(record('xxz_sorted', psi, Hs))
    assert max(np.max(np.diff(W['slices'][0])) for W in out[-1]['Ws']) > 1

    tfi = TFIChain(dict(L=6, J=1., g=1.3, conserve=None, bc_MPS='finite'))
    out.append(record('tfi', two_sweeps(tfi, ['up']), tfi.H_MPO))

    psi_c = psi.copy()              # a quench: the state evolves under the chain in the staggered field
    tebd.TEBDEngine(psi_c, M, {'dt': 0.1, 'order': 2, 'N_steps': 3, 'trunc_params': {'chi_max': 8, 'svd_min': 1.e-10}}).run()
    assert psi_c.dtype.kind == 'c'
    out.append(record('xxz_tebd', psi_c, M.H_MPO))

    neel = MPS.from_product_state(M.lat.mps_sites(), ['up', 'down'] * 3, bc='finite')
    out.append(record('neel', neel, M.H_MPO))

    M2 = xxz(2)
    out.append(record('two_sites', MPS.from_singlets(M2.lat.mps_sites()[0], 2, [(0, 1)], bc='finite'), M2.H_MPO))
    return out


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = main()
    path = os.path.join(HERE, 'moments.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote moments.pkl", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
