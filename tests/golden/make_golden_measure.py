"""Generate the measurement fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its ``MPS.expectation_value``
and ``MPS.correlation_function`` (networks/mps.py:680-887) return on small ground states.

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_measure.py

Output (committed): ``tests/golden/measure.pkl`` -- plain dict / list / numpy content only.  A list of states, each with

* ``Bs``     the stored site tensors ([vL, p, vR]) as dense arrays with the charges of every index and the block boundaries
             (``slices``) of every leg (the ``blocked_array`` format of ``tests/mpo_cell_fixtures.py``), ``forms``, ``S`` (L + 1 spectra),
             ``chinfo_mod``, ``complex``;
* ``ops``    the dense one-site operators ([p, p*]) by name;
* ``expval`` {name: the reference's ``expectation_value``};
* ``corr``   a list of calls: ``op1`` / ``op2`` (names), ``opstr`` (a name or None: the dense string the call is to be given),
             ``sites1`` / ``sites2`` (or None), ``str_on_first``, ``hermitian`` and ``result``.

States: the XXZ chain L = 8 with Sz conserved in a staggered field (so that <Sz> != 0), chi <= 16 after four sweeps -- (Sz, Sz) and the
charged pair (Sp, Sm), each with ``hermitian`` True and False and (``hermitian=False``) with the site subsets [1, 4, 6] x [0, 2, 4, 7]; spinless fermions
L = 8 with N conserved -- (Cd, C) with the Jordan-Wigner string the reference chose on its own (recorded as ``opstr`` = 'JW'), and a second
call with the string given explicitly and ``str_on_first=False``; the TFI chain L = 8 without a charge -- (Sx, Sz); and the XXZ state after
three complex TEBD steps (complex tensors)."""
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
from tenpy.models.fermions_spinless import FermionChain  # noqa: E402
from tenpy.models.spins import SpinChain  # noqa: E402
from tenpy.models.tf_ising import TFIChain  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402

L = 8
SUB1, SUB2 = [1, 4, 6], [0, 2, 4, 7]


def ground_state(M, init, chi=16):
    sites = M.lat.mps_sites()
    psi = MPS.from_product_state(sites, init * (len(sites) // 2), bc='finite')
    eng = dmrg.TwoSiteDMRGEngine(psi, M, {'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'mixer': True, 'max_sweeps': 4,
                                          'min_sweeps': 4})
    eng.run()
    return psi


def record(name, psi, op_names, expval, calls):
    site = psi.sites[0]
    ops = {n: site.get_op(n).copy().itranspose(['p', 'p*']).to_ndarray() for n in op_names}
    rec = dict(name=name, L=psi.L, chinfo_mod=np.array(psi.chinfo.mod), complex=bool(psi.dtype.kind == 'c'),
               Bs=[dense(psi.get_B(i, None), ['vL', 'p', 'vR']) for i in range(psi.L)], forms=[tuple(f) for f in psi.form],
               S=[np.array(psi.get_SL(i)) for i in range(psi.L)] + [np.array(psi.get_SR(psi.L - 1))], ops=ops,
               expval={n: np.array(psi.expectation_value(n)) for n in expval}, corr=[])
    for c in calls:
        c = dict(dict(sites1=None, sites2=None, opstr=None, str_on_first=True, hermitian=False, explicit=True), **c)
        kw = dict(sites1=c['sites1'], sites2=c['sites2'], str_on_first=c['str_on_first'], hermitian=c['hermitian'])
        if c['opstr'] is not None and c.pop('explicit'):
            kw['opstr'] = c['opstr']
        c.pop('explicit', None)
        c['result'] = np.array(psi.correlation_function(c['op1'], c['op2'], **kw))
        rec['corr'].append(c)
    print(name, 'chi', psi.chi, 'dtype', psi.dtype, 'calls', len(rec['corr']), 'max |C|', max(np.max(np.abs(c['result'])) for c in rec['corr']))
    return rec


def spin_calls():
    out = []
    for a, b in (('Sz', 'Sz'), ('Sp', 'Sm')):
        for herm in (True, False):
            out.append(dict(op1=a, op2=b, hermitian=herm))
        # (the reference cannot compare site lists of different lengths for ``hermitian=True``: the subsets go with False)
        out.append(dict(op1=a, op2=b, sites1=SUB1, sites2=SUB2))
    return out


def main():
    out = []
    hz = 0.5 * (-1.)**np.arange(L)
    xxz = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=hz, conserve='Sz', bc_MPS='finite', sort_charge=True))
    psi = ground_state(xxz, ['up', 'down'])
    assert np.max(np.abs(psi.expectation_value('Sz'))) > 0.05 and max(psi.chi) <= 16
    out.append(record('xxz', psi, ['Sz', 'Sp', 'Sm'], ['Sz'], spin_calls()))

    fer = FermionChain(dict(L=L, J=1., V=0.5, mu=0., conserve='N', bc_MPS='finite'))
    psi_f = ground_state(fer, ['full', 'empty'])
    # the first call lets the reference choose the string (autoJW); the tests hand the recorded dense 'JW' to the stand-alone class
    out.append(record('fermions', psi_f, ['Cd', 'C', 'JW', 'N'], ['N'],
                      [dict(op1='Cd', op2='C', opstr='JW', explicit=False), dict(op1='Cd', op2='C', opstr='JW', explicit=False, hermitian=True),
                       dict(op1='Cd', op2='C', opstr='JW', str_on_first=False),
                       dict(op1='Cd', op2='C', opstr='JW', explicit=False, sites1=SUB1, sites2=SUB2)]))

    tfi = TFIChain(dict(L=L, J=1., g=1.3, conserve=None, bc_MPS='finite'))
    psi_t = ground_state(tfi, ['up', 'up'])
    out.append(record('tfi', psi_t, ['Sx', 'Sz'], ['Sx', 'Sz'],
                      [dict(op1='Sx', op2='Sz'), dict(op1='Sx', op2='Sz', sites1=SUB1, sites2=SUB2), dict(op1='Sx', op2='Sx', hermitian=True)]))

    psi_c = psi.copy()           # a quench: the ground state in the staggered field evolves under the chain without it
    xxz0 = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=0., conserve='Sz', bc_MPS='finite', sort_charge=True))
    eng = tebd.TEBDEngine(psi_c, xxz0, {'dt': 0.1, 'order': 2, 'N_steps': 3, 'trunc_params': {'chi_max': 16, 'svd_min': 1.e-10}})
    eng.run()
    assert psi_c.dtype.kind == 'c'
    out.append(record('xxz_tebd', psi_c, ['Sz', 'Sp', 'Sm'], ['Sz'], spin_calls()))
    return out


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = main()
    path = os.path.join(HERE, 'measure.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote measure.pkl", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
