"""Generate the MPO-application fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its ``MPO.apply_zipup``
(networks/mpo.py:1679-1767) and ``MPO.apply`` with ``compression_method='zip_up'`` (:1562-1602) produce on time-evolution MPOs
``U_II`` (``make_U_II``).

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_mpo_apply.py

Output (committed): ``tests/golden/mpo_apply.pkl`` -- plain dict / list / numpy content only.

* ``percall``   the interior steps of ONE zip-up pass (the third application; the state is entangled by then) with ``svd_theta`` watched,
                for three models: the XXZ chain L = 8 with Sz (``U_II`` complex, dt = 0.1), the spin-1 chain L = 6 with Sz (``U_II`` real,
                imaginary time: MPO bond blocks wider than 1) and the TFI chain L = 8 without a charge (one dense cell per block).  Per
                call: ``VH_prev`` ([vL, wR, vR], scaled with S as the pass hands it on), ``B`` ([vL, p, vR]) and ``W`` ([wL, wR, p, p*])
                as dense arrays with the charges of every index and the block boundaries (``slices``) of every leg, the dense ``M`` with split legs ([vL, p, wR, vR]) and ALL singular
                values of ``M`` (not normalised).
* ``untruncated`` XXZ L = 8, chi_max = 16 (the largest Schmidt rank of 8 sites: nothing above svd_min is cut), 4 applications of ``U_II``:
                the dense W tensors of ``U_II`` with charges, IdL / IdR, the start state, the final dense state vector (norm 1), S at
                every bond, ``norm``.
* ``truncating`` the same chain with chi_max = 4, m_temp = 2, 8 applications: final state vector, S, ``norm``, the summed truncation error,
                and for every truncating cut whose first dropped normalised singular value exceeds 1e-10 the last kept and the first
                dropped value; ``n_cuts`` and ``g``, the smallest such gap (last kept - first dropped of the spectrum normalised to
                norm 1: the quantity that bounds the rotation of the kept subspace under a perturbation; asserted >= 1e-5)."""
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
from make_golden_mixer import dense as _dense  # noqa: E402
from tenpy.linalg import np_conserved as npc  # noqa: E402
from tenpy.linalg import truncation  # noqa: E402
from tenpy.models.spins import SpinChain  # noqa: E402
from tenpy.models.tf_ising import TFIChain  # noqa: E402
from tenpy.networks import mpo as ref_mpo  # noqa: E402
from tenpy.networks import mps as ref_mps  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402

G_MIN = 1.e-5
DROP_MIN = 1.e-10


def dense(A, labels):
    """``make_golden_mixer.dense`` plus the block structure of every leg (``slices``: the first index of every charge block and the
    length), so that the tests rebuild the legs block for block and not one block per index."""
    rec = _dense(A, labels)
    rec['slices'] = [np.array(l.slices) for l in A.copy().itranspose(labels).legs]
    return rec


def xxz(L=8):
    return SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=0.1, conserve='Sz', bc_MPS='finite', sort_charge=True))


MODELS = [('xxz', lambda: xxz(8), -0.1j, ['up', 'down']),
          ('spin1', lambda: SpinChain(dict(L=6, S=1., Jx=1., Jy=1., Jz=0.7, hz=0.1, conserve='Sz', bc_MPS='finite', sort_charge=True)),
           -0.1, ['up', 'down']),
          ('tfi', lambda: TFIChain(dict(L=8, J=1., g=1.3, conserve=None, bc_MPS='finite')), -0.1j, ['up', 'down'])]


def start(M, init):
    sites = M.lat.mps_sites()
    return MPS.from_product_state(sites, init * (len(sites) // 2), bc='finite')


def watched_pass(U, psi, options):
    """One ``apply_zipup`` with ``svd_theta`` of the reference's mpo module watched: the records of the interior steps."""
    calls, state = [], dict(i=0, VH=None)
    orig = ref_mpo.svd_theta

    def watch(M, *args, **kwargs):
        i = state['i']
        res = orig(M, *args, **kwargs)
        if 0 < i < psi.L - 1:
            S_all = np.sort(np.asarray(npc.svd(M, compute_uv=False)))[::-1]
            calls.append(dict(i=i, VH_prev=dense(state['VH'], ['vL', 'wR', 'vR']), B=dense(psi.get_B(i, 'B'), ['vL', 'p', 'vR']),
                              W=dense(U.get_W(i), ['wL', 'wR', 'p', 'p*']),
                              M=M.split_legs().itranspose(['vL', 'p', 'wR', 'vR']).to_ndarray(), S_all=S_all))
        if i < psi.L - 1:
            state['VH'] = res[2].split_legs().iscale_axis(res[1], 'vL')       # what the pass hands to the next site
        state['i'] = i + 1
        return res
    ref_mpo.svd_theta = watch
    try:
        U.apply_zipup(psi, options)
    finally:
        ref_mpo.svd_theta = orig
    return calls


def percall():
    out = []
    for name, make, dt, init in MODELS:
        M = make()
        U = M.H_MPO.make_U_II(dt)      # exp(dt H): dt = -0.1j is a real-time step of 0.1, dt = -0.1 an imaginary-time one
        if name == 'spin1':
            U.sort_legcharges()         # sorted and bunched MPO bond legs: blocks wider than 1
        psi = start(M, init)
        opts = dict(compression_method='zip_up', trunc_params=dict(chi_max=16, svd_min=1.e-12), m_temp=2)
        for _ in range(2):
            U.apply(psi, dict(opts))
        calls = watched_pass(U, psi, dict(opts))
        mid = psi.L // 2
        calls = [c for c in calls if c['i'] in (1, mid - 1, mid)]
        for c in calls:
            c.update(name=name, chinfo_mod=np.array(M.lat.unit_cell[0].leg.chinfo.mod), dt=complex(dt))
        print(name, 'U_II dtype', U.dtype, 'D', max(U.chi), 'calls', [(c['i'], c['M'].shape) for c in calls],
              'wR blocks', [int(b) for b in U.get_W(mid).get_leg('wR').get_block_sizes()])
        out += calls
    return out


def end_to_end(chi, m_temp, n_apply, record_mpo):
    M = xxz(8)
    U = M.H_MPO.make_U_II(-0.1j)
    psi = start(M, ['up', 'down'])
    cuts = []
    orig = truncation.svd_theta

    def watch(theta, trunc_par, *args, **kwargs):
        res = orig(theta, trunc_par, *args, **kwargs)
        S_all = np.sort(np.asarray(npc.svd(theta, compute_uv=False)))[::-1]
        S_all = S_all / np.linalg.norm(S_all)
        n = len(res[1])
        if n < len(S_all) and S_all[n] > DROP_MIN:
            cuts.append((float(S_all[n - 1]), float(S_all[n])))
        return res
    ref_mpo.svd_theta = ref_mps.svd_theta = watch
    err = truncation.TruncationError()
    try:
        for _ in range(n_apply):
            err = err + U.apply(psi, dict(compression_method='zip_up', trunc_params=dict(chi_max=chi, svd_min=1.e-12), m_temp=m_temp))
    finally:
        ref_mpo.svd_theta = ref_mps.svd_theta = orig
    sites = M.lat.mps_sites()
    vec = psi.get_theta(0, psi.L).to_ndarray().reshape(-1)
    res = dict(L=8, chi_max=chi, m_temp=m_temp, svd_min=1.e-12, n_apply=n_apply, dt=0.1, vec=vec,
               S=[np.array(psi.get_SL(i)) for i in range(1, psi.L)], norm=float(psi.norm), err_eps=float(err.eps),
               init=[int(sites[i].state_labels[l]) for i, l in enumerate(['up', 'down'] * (len(sites) // 2))],
               cuts=np.array(cuts).reshape(-1, 2), n_cuts=len(cuts),
               g=min((a - b for a, b in cuts), default=np.inf), norm_test=float(abs(psi.overlap(psi) - 1.)))
    if record_mpo:
        res['mpo'] = dict(W=[dense(U.get_W(i), ['wL', 'wR', 'p', 'p*']) for i in range(U.L)], IdL=list(U.IdL), IdR=list(U.IdR),
                          chinfo_mod=np.array(U.chinfo.mod), p_leg=(np.array(sites[0].leg.to_qflat()), int(sites[0].leg.qconj)))
    return res


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = dict(percall=percall(), untruncated=end_to_end(16, 2, 4, True), truncating=end_to_end(4, 2, 8, False))
    for k in ('untruncated', 'truncating'):
        r = out[k]
        print(k, 'chi', [len(s) for s in r['S']], 'norm', r['norm'], 'err', r['err_eps'], 'cuts', r['n_cuts'], 'g %.3g' % r['g'])
    assert out['untruncated']['n_cuts'] == 0, "chi_max = 16 must not truncate"
    assert out['truncating']['n_cuts'] > 0 and out['truncating']['g'] >= G_MIN, "a truncating cut is degenerate: g = %.3g" % out['truncating']['g']
    path = os.path.join(HERE, 'mpo_apply.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote mpo_apply.pkl", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
