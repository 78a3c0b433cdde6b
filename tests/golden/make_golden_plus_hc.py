"""Generate the ``H + h.c.`` fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its engines produce for models
built with ``explicit_plus_hc=True``, where the MPO holds half of the Hamiltonian and every effective Hamiltonian is
``SumNpcLinearOperator(eff_H, eff_H.adjoint())`` (mps_common.py:519, tdvp.py:310, :422).

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_plus_hc.py

Output (committed): ``tests/golden/plus_hc.pkl`` -- plain dict / list / numpy content only.

* ``dmrg``  two-site DMRG with Lanczos always used (``max_N_for_ED=0``, mixer off, the options of ``make_golden.py``): per-sweep energies,
            bond dimensions and final entropies of the XXZ chain L = 16 (Sz) at chi = 32 and of the Fermi-Hubbard ladder 2 x 4 with
            (N, 2Sz) and a Peierls phase on the legs (complex MPO that is not Hermitian) at chi = 32.
* ``tdvp``  two-site TDVP from a product state, three steps: entropies, bond dimensions and ``psi.norm`` per step, same two models
            (XXZ L = 12, ladder 2 x 3).
Every record also holds the result of the same run with the full MPO (``explicit_plus_hc=False``) for information; the generator
asserts that the two agree, so the fixture pins the model and not a convention."""
import os
import pickle
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import build_ref  # noqa: E402  (where the reference lives)

sys.path.insert(0, build_ref.reference_root())
os.environ.setdefault('TENPY_NO_CYTHON', '1')
from tenpy.algorithms import dmrg, tdvp  # noqa: E402
from tenpy.models.hubbard import FermiHubbardModel  # noqa: E402
from tenpy.models.xxz_chain import XXZChain2  # noqa: E402  (the CouplingMPOModel form: takes explicit_plus_hc)
from tenpy.networks.mps import MPS  # noqa: E402


class PeierlsLadder(FermiHubbardModel):
    """Fermi-Hubbard ladder whose hoppings along leg y = 0 carry the phase exp(+i peierls) and those along y = 1 exp(-i peierls):
    ``-t e^{+-i peierls} c^dag_{x, y} c_{x + 1, y} + h.c.``, rungs ``-t c^dag_{x, 0} c_{x, 1} + h.c.``, ``U n_up n_down - mu n``."""

    def init_terms(self, model_params):
        t, U, mu = model_params.get('t', 1., 'real'), model_params.get('U', 0, 'real'), model_params.get('mu', 0., 'real')
        phi = model_params.get('peierls', 0., 'real')
        model_params.get('V', 0, 'real'), model_params.get('phi_ext', None, 'real')
        for u in range(2):
            self.add_onsite(-mu, u, 'Ntot')
            self.add_onsite(U, u, 'NuNd')
            hop = -t * np.exp(1.j * phi * (1 - 2 * u))
            for cd, c in (('Cdu', 'Cu'), ('Cdd', 'Cd')):
                self.add_coupling(hop, u, cd, u, c, 1, plus_hc=True)
        for cd, c in (('Cdu', 'Cu'), ('Cdd', 'Cd')):
            self.add_coupling(-t, 0, cd, 1, c, 0, plus_hc=True)


def make_model(kind, par, plus_hc):
    if kind == 'xxz':
        return XXZChain2(dict(par, bc_MPS='finite', sort_charge=True, explicit_plus_hc=plus_hc))
    return PeierlsLadder(dict(par, lattice='Ladder', cons_N='N', cons_Sz='Sz', bc_MPS='finite', sort_charge=True,
                              explicit_plus_hc=plus_hc))


MODELS = [('xxz', dict(Jxx=1., Jz=0.7, hz=0.1), ['up', 'down']),
          ('peierls_ladder', dict(t=1., U=4., mu=0., peierls=0.3), ['up', 'down'])]


def run_dmrg(kind, par, init, chi, n_sweeps, plus_hc):
    M = make_model(kind, par, plus_hc)
    assert bool(M.H_MPO.explicit_plus_hc) == plus_hc
    n = len(M.lat.mps_sites())
    psi = MPS.from_product_state(M.lat.mps_sites(), init * (n // 2), bc='finite')
    eng = dmrg.TwoSiteDMRGEngine(psi, M, {'mixer': None, 'combine': True, 'max_N_for_ED': 0,
                                          'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'lanczos_params': {}})
    Es, chis = [], []
    for _ in range(n_sweeps):
        eng.sweep()
        Es.append(float(np.real(eng.update_stats['E_total'][-1])))
        chis.append(int(max(psi.chi)))
    return dict(E_sweeps=Es, chi_sweeps=chis, S_ent=np.array(psi.entanglement_entropy()), D_mpo=int(max(M.H_MPO.chi)),
                dtype=str(M.H_MPO.dtype), E_updates=[float(np.real(e)) for e in eng.update_stats['E_total']])


def run_tdvp(kind, par, init, chi, dt, n_steps, plus_hc):
    M = make_model(kind, par, plus_hc)
    n = len(M.lat.mps_sites())
    psi = MPS.from_product_state(M.lat.mps_sites(), init * (n // 2), bc='finite')
    eng = tdvp.TwoSiteTDVPEngine(psi, M, {'dt': dt, 'N_steps': 1, 'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}})
    S, chis, norm = [], [], []
    for _ in range(n_steps):
        eng.run()
        S.append(np.array(psi.entanglement_entropy()))
        chis.append(list(psi.chi))
        norm.append(float(psi.norm))
    return dict(S=np.array(S), chi=chis, norm=np.array(norm))


if __name__ == '__main__':
    out = dict(dmrg=[], tdvp=[])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for (kind, par, init), size in zip(MODELS, (dict(L=16), dict(L=4))):
            half, full = (run_dmrg(kind, dict(par, **size), init, 32, 4, hc) for hc in (True, False))
            dE = max(abs(a - b) for a, b in zip(half['E_sweeps'], full['E_sweeps']))
            print(kind, 'dmrg E', half['E_sweeps'], 'chi', half['chi_sweeps'], 'MPO D', half['D_mpo'], 'vs', full['D_mpo'], half['dtype'],
                  'max |E - E(full MPO)| %.2e' % dE)
            assert dE < 1.e-10 and half['D_mpo'] < full['D_mpo']
            out['dmrg'].append(dict(name=kind, params=par, init=init, chi=32, n_sweeps=4, full_mpo=full, **size, **half))
        for (kind, par, init), size in zip(MODELS, (dict(L=12), dict(L=3))):
            half, full = (run_tdvp(kind, dict(par, **size), init, 16, 0.05, 3, hc) for hc in (True, False))
            dS = float(np.abs(half['S'] - full['S']).max())
            print(kind, 'tdvp chi', half['chi'][-1], 'norm', half['norm'], 'max |S - S(full MPO)| %.2e' % dS)
            assert dS < 1.e-10 and half['chi'] == full['chi']
            out['tdvp'].append(dict(name=kind, params=par, init=init, chi_max=16, svd_min=1.e-10, dt=0.05, n_steps=3, full_mpo=full,
                                    **size, **half))
    path = os.path.join(HERE, 'plus_hc.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote plus_hc.pkl", os.path.getsize(path), "bytes")
