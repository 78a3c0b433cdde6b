"""Generate the single-site DMRG fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its ``SubspaceExpansion``
(mps_common.py:2082-2201) produces inside its own runs of ``SingleSiteDMRGEngine`` (dmrg.py:955-1140).

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_1site.py

Output (committed): ``tests/golden/dmrg_1site.pkl`` -- plain dict / list / numpy content only.

* ``percall``  calls of ``mix_and_decompose_1site`` dumped from runs of the XXZ chain L = 8 with Sz (real) and the Peierls ladder 2 x 3
               with (N, 2Sz) (complex), both at chi_max = 8: two interior sites each, both directions, second sweep -- plus, per model,
               one call of the stacked form (the same right move repeated with ``IdL`` / ``IdR`` of that bond removed from the MPO; the
               run itself goes on with the natural MPO).  Per call: ``LP``, ``RP``, ``W0`` and ``theta`` ([vL, p0, vR]) as dense arrays
               with the charges of every index, the amplitude, ``IdL`` / ``IdR``, the direction, the truncation parameters; the results:
               dense ``theta_expand`` with split legs ([vL, p0, wR, vR] / [vL, wL, p0, vR]), its magnitude sums ``mag`` (the same
               contraction with absolute values throughout and |LP| |W| in place of |LHeff|; float32, rounded up), ALL singular values
               of ``theta_expand`` (normalised to norm 1) before truncation, the relative ``gap`` between the last kept and the first
               dropped one, and -- only where that gap is >= 1e-4 -- ``err.eps``, the kept ``S`` and dense ``U S VH`` (= the truncated
               theta, [vL, p0, vR]).
* ``dmrg``     the reference's own ``SingleSiteDMRGEngine`` run of the XXZ chain L = 12 (Jxx = 1, Jz = 0.7, hz = 0.1) from the product
               state up down ..., chi_max = 24, svd_min = 1e-8, mixer amplitude 1e-5, decay 2, disable_after 4, six sweeps, Lanczos
               always (``max_N_for_ED = 0``): per-sweep and per-update energies, bond dimensions, final entropies, the sweep after
               which the mixer is gone, the reference's MPO (dense tensors with charges, ``IdL`` / ``IdR`` per bond, the initial state:
               the perturbation depends on how the MPO distributes the couplings) and ``min_gap``, the smallest relative gap at the
               cut over all SVD calls of the run, with the mixer and after it (``n_svd_calls`` = 132; asserted >= 1e-4).  The ladder gets no sweep-by-sweep record: its single-site runs
               cut exactly degenerate pairs."""
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
from make_golden_plus_hc import make_model  # noqa: E402
from make_golden_mixer import dense  # noqa: E402
from tenpy.algorithms import dmrg, mps_common  # noqa: E402
from tenpy.linalg import np_conserved as npc  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402

CASES = [('xxz', 'xxz', dict(Jxx=1., Jz=0.7, hz=0.1), dict(L=8), 8),
         ('peierls_ladder', 'peierls_ladder', dict(t=1., U=4., mu=0., peierls=0.3), dict(L=3), 8)]
MIXER = {'amplitude': 1.e-5, 'decay': 2., 'disable_after': 4}
GAP = 1.e-4


def magnitude(eff, theta3, mix, keep, stacked, move_right):
    """sum |LP| |W| mix |theta| with the legs of the split ``theta_expand``; ``stacked``: |theta| in front of the kept indices."""
    lp = np.abs(eff.LP.copy().itranspose(['vR*', 'wR', 'vR']).to_ndarray())
    rp = np.abs(eff.RP.copy().itranspose(['wL', 'vL', 'vL*']).to_ndarray())
    w = np.abs(eff.W0.copy().itranspose(['wL', 'wR', 'p0', 'p0*']).to_ndarray())
    th = np.abs(theta3)
    if move_right:
        mag = np.einsum('awc,cqb,wxpq,x->apxb', lp, th, w, np.abs(mix), optimize=True)
        ax = 2
    else:
        mag = np.einsum('aqc,wcb,xwpq,x->axpb', th, rp, w, np.abs(mix), optimize=True)
        ax = 1
    if stacked:
        mag = np.concatenate([np.expand_dims(th, ax), np.compress(keep, mag, axis=ax)], axis=ax)
    return mag


def gap_at_cut(S_all, n_keep):
    if n_keep >= len(S_all) or S_all[n_keep - 1] == 0.:
        return np.inf
    return float((S_all[n_keep - 1] - S_all[n_keep]) / S_all[n_keep - 1])


def decompose(mixer, engine, theta, i0, move_right, chi, svd_min, name):
    """One call of the reference's method with its ``svd_theta`` watched: the record of the call and what it returned."""
    seen = {}
    orig_svd = mps_common.svd_theta

    def watch(theta_expand, *args, **kwargs):
        seen['expand'] = theta_expand.copy()
        return orig_svd(theta_expand, *args, **kwargs)
    mps_common.svd_theta = watch
    try:
        U, S, VH, err = ORIG(mixer, engine, theta, i0, move_right)
    finally:
        mps_common.svd_theta = orig_svd
    eff, H = engine.eff_H, engine.env.H
    bond = i0 if move_right else i0 - 1
    mix_L, mix_R, IdL, IdR, hc = mps_common._mix_LR(H, bond, np.sqrt(mixer.amplitude))
    assert not hc
    Id = IdL if move_right else IdR
    stacked = Id is None
    keep = np.ones(len(mix_L), bool)
    for k in (IdL, IdR):
        if k is not None:
            keep[k] = False
    mix = np.full(len(mix_L), np.sqrt(mixer.amplitude)) if stacked else (mix_L if move_right else mix_R)
    expand = seen['expand']
    theta3 = theta.split_legs().itranspose(['vL', 'p0', 'vR'])
    labels = ['vL', 'p0', 'wR', 'vR'] if move_right else ['vL', 'wL', 'p0', 'vR']
    S_all = np.sort(np.asarray(npc.svd(expand, compute_uv=False)))[::-1]
    S_all = S_all / np.linalg.norm(S_all)
    n_keep = len(S)
    gap = gap_at_cut(S_all, n_keep)
    rec = dict(name=name, i0=int(i0), sweep=int(engine.sweeps), move_right=bool(move_right), amplitude=float(mixer.amplitude),
               IdL=IdL, IdR=IdR, stacked=bool(stacked), explicit_plus_hc=False, trunc_params=dict(chi_max=chi, svd_min=svd_min),
               chinfo_mod=np.array(theta.chinfo.mod),
               LP=dense(eff.LP, ['vR*', 'wR', 'vR']), RP=dense(eff.RP, ['wL', 'vL', 'vL*']), W0=dense(eff.W0, ['wL', 'wR', 'p0', 'p0*']),
               theta=dense(theta3, ['vL', 'p0', 'vR']),
               theta_expand=expand.split_legs().itranspose(labels).to_ndarray(),
               mag=(magnitude(eff, theta3.to_ndarray(), mix, keep, stacked, move_right) * (1 + 1.e-6)).astype(np.float32),
               S_all=S_all, n_keep=int(n_keep), gap=gap)
    if gap >= GAP:
        SV = VH.iscale_axis(S, 'vL') if not isinstance(S, npc.Array) else npc.tensordot(S, VH, axes=['vR', 'vL'])
        usv = npc.tensordot(U, SV, axes=['vR', 'vL']).split_legs().itranspose(['vL', 'p0', 'vR'])
        rec.update(err_eps=float(err.eps), S=np.array(S), USV=usv.to_ndarray())
    return rec, gap


def run(name, kind, par, size, chi, n_sweeps, dump=None, svd_min=1.e-10):
    M = make_model(kind, dict(par, **size), False)
    sites = M.lat.mps_sites()
    psi = MPS.from_product_state(sites, ['up', 'down'] * (len(sites) // 2), bc='finite')
    eng = dmrg.SingleSiteDMRGEngine(psi, M, {'mixer': True, 'mixer_params': dict(MIXER), 'combine': False, 'max_N_for_ED': 0,
                                             'trunc_params': {'chi_max': chi, 'svd_min': svd_min}, 'lanczos_params': {}})
    eng.mixer_activate()          # (the reference does this in `run`; the sweeps are driven from here)
    assert isinstance(eng.mixer, mps_common.SubspaceExpansion)
    calls, gaps, stacked_done = [], [], []
    H = M.H_MPO

    def spy(self, engine, theta, i0, move_right):
        if dump is not None and (engine.sweeps, i0, bool(move_right)) in dump:
            if move_right and not stacked_done:       # the stacked form: the same call with IdL / IdR of the bond removed
                keepL, keepR = H.IdL[i0 + 1], H.IdR[i0 + 1]
                H.IdL[i0 + 1], H.IdR[i0 + 1] = None, None
                try:
                    rec, _ = decompose(self, engine, theta.copy(), i0, move_right, chi, svd_min, name)
                finally:
                    H.IdL[i0 + 1], H.IdR[i0 + 1] = keepL, keepR
                assert rec['stacked']
                calls.append(rec)
                stacked_done.append(True)
            rec, _ = decompose(self, engine, theta.copy(), i0, move_right, chi, svd_min, name)
            calls.append(rec)
        if dump is None:
            seen = {}
            orig_svd = mps_common.svd_theta

            def watch(theta_expand, *args, **kwargs):
                seen['expand'] = theta_expand.copy()
                return orig_svd(theta_expand, *args, **kwargs)
            mps_common.svd_theta = watch
            try:
                res = ORIG(self, engine, theta, i0, move_right)
            finally:
                mps_common.svd_theta = orig_svd
            S_all = np.sort(np.asarray(npc.svd(seen['expand'], compute_uv=False)))[::-1]
            gaps.append(gap_at_cut(S_all / np.linalg.norm(S_all), len(res[1])))
            return res
        return ORIG(self, engine, theta, i0, move_right)
    mps_common.SubspaceExpansion.mix_and_decompose_1site = spy
    plain_svd = dmrg.svd_theta

    def plain_watch(theta, *args, **kwargs):       # the updates after the mixer is gone: the engine's own svd_theta
        res = plain_svd(theta, *args, **kwargs)
        S_all = np.sort(np.asarray(npc.svd(theta, compute_uv=False)))[::-1]
        gaps.append(gap_at_cut(S_all / np.linalg.norm(S_all), len(res[1])))
        return res
    if dump is None:
        dmrg.svd_theta = plain_watch
    try:
        Es, chis, gone = [], [], None
        for s in range(n_sweeps):
            eng.sweep()
            Es.append(float(np.real(eng.update_stats['E_total'][-1])))
            chis.append(int(max(psi.chi)))
            if eng.mixer is None and gone is None:
                gone = s + 1
    finally:
        mps_common.SubspaceExpansion.mix_and_decompose_1site = ORIG
        dmrg.svd_theta = plain_svd
    mpo = dict(W=[dense(H.get_W(i), ['wL', 'wR', 'p', 'p*']) for i in range(H.L)], IdL=list(H.IdL), IdR=list(H.IdR),
               chinfo_mod=np.array(H.chinfo.mod), init=[int(sites[i].state_labels[l]) for i, l in enumerate(['up', 'down'] * (len(sites) // 2))])
    res = dict(mpo=mpo, svd_min=svd_min, min_gap=min(gaps) if gaps else None, n_svd_calls=len(gaps), E_sweeps=Es, chi_sweeps=chis,
               S_ent=np.array(psi.entanglement_entropy()) if eng.mixer is None else None, D_mpo=int(max(H.chi)), dtype=str(H.dtype),
               E_updates=[float(np.real(e)) for e in eng.update_stats['E_total']], mixer_gone_after=gone)
    return res, calls


ORIG = mps_common.SubspaceExpansion.mix_and_decompose_1site

if __name__ == '__main__':
    out = dict(percall=[], dmrg=[])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, kind, par, small, chi in CASES:
            n = 2 * small['L'] if kind != 'xxz' else small['L']
            sites = (n // 2 - 1, n // 2)
            dump = {(1, i, d) for i in sites for d in (True, False)}      # the second sweep: the bonds have grown to chi_max
            _, calls = run(name, kind, par, small, chi, 2, dump)
            got = sorted((c['i0'], c['move_right'], c['stacked']) for c in calls)
            print(name, 'percall: %d calls' % len(calls), got, 'gaps', ['%.2e' % c['gap'] for c in calls], 'kept', [c['n_keep'] for c in calls])
            assert {(c['i0'], c['move_right']) for c in calls if not c['stacked']} == {(i, d) for i in sites for d in (True, False)}
            assert sum(c['stacked'] for c in calls) == 1
            out['percall'] += calls
        name, kind, par = CASES[0][:3]
        res, _ = run(name, kind, par, dict(L=12), 24, 6, svd_min=1.e-8)
        print(name, 'SVD calls', res['n_svd_calls'], 'min gap %.2e' % res['min_gap'], 'dmrg E', res['E_sweeps'], 'chi', res['chi_sweeps'],
              'mixer gone after sweep', res['mixer_gone_after'])
        assert res['min_gap'] >= GAP and res['n_svd_calls'] == 6 * 2 * 11
        out['dmrg'].append(dict(name=name, kind=kind, params=par, chi=24, n_sweeps=6, mixer_params=dict(MIXER), L=12, **res))
    path = os.path.join(HERE, 'dmrg_1site.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote dmrg_1site.pkl", os.path.getsize(path), "bytes")
