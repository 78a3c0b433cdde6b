"""Generate the TDVP fixtures from the REFERENCE implementation (TeNPy, pure-Python path).

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_tdvp.py

Output (committed): ``tests/golden/tdvp.pkl`` -- plain dict / list / numpy content only, same dump format as ``make_golden.py``.

* ``operators``     per model (TFI L=10 parity, XXZ L=12 Sz; the state after 6 two-site TDVP steps from a product state, complex):
                    the tensors of the effective two- / one- / zero-site Hamiltonian at the middle of the chain, a vector, ``H vector``.
* ``evolutions``    ``LanczosEvolution(H, theta, opts).run(delta, normalize)`` through those operators: ``psi``, ``N``; plus, for
                    information, the reference's own round-trip error and norm drift at delta = -0.025j.
* ``trajectories``  two-site TDVP for 12 steps, then single-site TDVP for 4 steps: entropies, bond dimensions, local expectation
                    values and ``psi.norm`` per step.  Well-posedness is asserted here: every trajectory is run again with much
                    tighter Lanczos parameters and must give identical bond dimensions and entropies / expectation values equal
                    within 1e-12 -- otherwise the fixture would pin rounding noise and other parameters have to be chosen.
"""
import os
import pickle
import sys
import warnings

import numpy as np

sys.path.insert(0, '/root/reference')
os.environ.setdefault('TENPY_NO_CYTHON', '1')
import tenpy.linalg.np_conserved as npc  # noqa: E402
from tenpy.algorithms import tdvp  # noqa: E402
from tenpy.algorithms.mps_common import OneSiteH, TwoSiteH, ZeroSiteH  # noqa: E402
from tenpy.linalg import charges  # noqa: E402
from tenpy.linalg.krylov_based import LanczosEvolution  # noqa: E402
from tenpy.models.tf_ising import TFIChain  # noqa: E402
from tenpy.models.xxz_chain import XXZChain  # noqa: E402
from tenpy.networks.mpo import MPOEnvironment  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
DT, CHI, SVD_MIN = 0.05, 8, 1.e-10
DELTAS = [(-0.025j, None), (+0.025j, None), (-0.05, False), (-0.05, True)]
OPTS = [{}, {'N_min': 4, 'N_max': 4}]


def dump_leg(leg):
    d = dict(slices=np.array(leg.slices), charges=np.array(leg.charges), qconj=int(leg.qconj),
             mod=np.array(leg.chinfo.mod), sorted=bool(leg.sorted), bunched=bool(leg.bunched))
    if isinstance(leg, charges.LegPipe):
        d['pipe'] = dict(legs=[dump_leg(l) for l in leg.legs], q_map=np.array(leg.q_map),
                         q_map_slices=np.array(leg.q_map_slices))
    return d


def dump_array(a):
    return dict(legs=[dump_leg(l) for l in a.legs], qtotal=np.array(a.qtotal), qdata=np.array(a._qdata),
                qdata_sorted=bool(a._qdata_sorted), blocks=[np.array(b) for b in a._data], labels=list(a._labels),
                dtype=str(a.dtype), dense=a.to_ndarray())


def models():
    tfi = dict(L=10, J=1., g=1.5)
    xxz = dict(L=12, Jxx=1., Jz=0.5, hz=0.)
    return [
        ('tfi_parity', 'tfi', dict(tfi, conserve='parity'), ['up'] * 10, 'Sigmaz'),
        ('tfi_None', 'tfi', dict(tfi, conserve=None), ['up'] * 10, 'Sigmaz'),
        ('xxz_Sz', 'xxz', dict(xxz, conserve='Sz'), ['up', 'down'] * 6, 'Sz'),
    ]


def make_model(kind, par):
    if kind == 'tfi':
        return TFIChain(dict(par, bc_MPS='finite', sort_charge=True))
    return XXZChain({k: v for k, v in dict(par, bc_MPS='finite', sort_charge=True).items() if k != 'conserve'})


def trajectory(M, init, op, two_steps, one_steps, lanczos):
    psi = MPS.from_product_state(M.lat.mps_sites(), init, bc='finite')
    opts = {'dt': DT, 'N_steps': 1, 'trunc_params': {'chi_max': CHI, 'svd_min': SVD_MIN}, 'lanczos_params': dict(lanczos)}
    out = dict(S=[], chi=[], ev=[], norm=[])
    for cls, steps in ((tdvp.TwoSiteTDVPEngine, two_steps), (tdvp.SingleSiteTDVPEngine, one_steps)):
        if steps == 0:
            continue
        eng = cls(psi, M, dict(opts))
        for _ in range(steps):
            eng.run()
            out['S'].append(np.array(psi.entanglement_entropy()))
            out['chi'].append(list(psi.chi))
            out['ev'].append(np.real(np.array(psi.expectation_value(op))))
            out['norm'].append(float(psi.norm))
    return psi, {k: np.array(v) for k, v in out.items()}


def gen_trajectories():
    recs = []
    for name, kind, par, init, op in models():
        M = make_model(kind, par)
        _, a = trajectory(M, init, op, 12, 4, {})
        _, b = trajectory(M, init, op, 12, 4, {'P_tol': 1.e-20, 'N_max': 30})
        assert np.array_equal(a['chi'], b['chi']), name
        dS, dev = np.abs(a['S'] - b['S']).max(), np.abs(a['ev'] - b['ev']).max()
        print(name, 'chi', a['chi'][-1], 'max dS %.2e  max d<op> %.2e under tighter Lanczos parameters' % (dS, dev))
        assert dS < 1.e-12 and dev < 1.e-12, name
        assert np.max(a['chi']) == CHI, "the truncation is to be exercised"
        site = M.lat.mps_sites()[0]
        recs.append(dict(name=name, kind=kind, params=par, init=init, op=op, dt=DT, chi_max=CHI, svd_min=SVD_MIN, two_steps=12,
                         one_steps=4, S=a['S'], chi=a['chi'], ev=a['ev'], norm=a['norm'], sensitivity=dict(dS=dS, dev=dev),
                         state_labels=list(site.state_labels.items())))
    d = np.abs(recs[0]['S'] - recs[1]['S']).max()
    print('tfi parity vs no charges: max dS %.2e' % d)
    assert d < 1.e-12
    return recs


def gen_operators():
    ops_out, evo_out = [], []
    for name, kind, par, init, op in models():
        if par['conserve'] is None:
            continue
        M = make_model(kind, par)
        psi, _ = trajectory(M, init, op, 6, 0, {})
        env = MPOEnvironment(psi, M.H_MPO, psi)
        i = psi.L // 2
        th0 = npc.diag(psi.get_SL(i), psi.get_B(i, 'B').get_leg('vL'), labels=['vL', 'vR']).astype(np.complex128)
        hams = {'two': (TwoSiteH(env, i - 1, combine=False), psi.get_theta(i - 1, n=2)),
                'one': (OneSiteH(env, i, combine=False), psi.get_theta(i, n=1)),
                'zero': (ZeroSiteH(env, i), th0)}
        for k, (H, th) in hams.items():
            if k != 'zero':
                th = H.combine_theta(th)
            assert th.dtype == np.complex128 and H.LP.dtype == np.complex128
            rec = dict(model=name, op=k, i0=H.i0, LP=dump_array(H.LP), RP=dump_array(H.RP), theta=dump_array(th),
                       matvec=dump_array(H.matvec(th)))
            if k != 'zero':
                rec['W0'] = dump_array(M.H_MPO.get_W(H.i0))
            if k == 'two':
                rec['W1'] = dump_array(M.H_MPO.get_W(H.i0 + 1))
            d = -0.025j
            a, N1 = LanczosEvolution(H, th, {}).run(d, normalize=False)
            b, N2 = LanczosEvolution(H, a, {}).run(-d, normalize=False)
            n0 = npc.norm(th)
            rec['reference_round_trip'] = float(npc.norm(b - th) / n0)
            rec['reference_norm_drift'] = float(abs(npc.norm(a) - n0) / n0)
            rec['reference_N'] = (N1, N2)
            print(name, k, 'N', N1, N2, 'round trip %.2e norm drift %.2e' % (rec['reference_round_trip'], rec['reference_norm_drift']),
                  'size', th.size)
            ops_out.append(rec)
            for delta, normalize in DELTAS:
                for opts in OPTS:
                    res, N = LanczosEvolution(H, th, dict(opts)).run(delta, normalize)
                    evo_out.append(dict(model=name, op=k, delta=delta, normalize=normalize, opts=dict(opts), N=N, psi=dump_array(res)))
    return ops_out, evo_out


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        ops, evo = gen_operators()
        out = dict(operators=ops, evolutions=evo, trajectories=gen_trajectories())
    path = os.path.join(HERE, 'tdvp.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote tdvp.pkl", os.path.getsize(path), "bytes")
