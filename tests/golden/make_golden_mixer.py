"""Generate the density-matrix mixer fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its
``DensityMatrixMixer`` (mps_common.py:1962-2079) produces inside its own mixer-on runs of two-site DMRG.

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_mixer.py

Output (committed): ``tests/golden/mixer.pkl`` -- plain dict / list / numpy content only.

* ``percall``  calls of ``mixed_svd_2site`` dumped from runs of the XXZ chain L = 8 with Sz (real, chi_max = 8), the Fermi-Hubbard
               ladder 2 x 3 with (N, 2Sz) and a Peierls phase (complex, chi_max = 8) and the XXZ chain with ``explicit_plus_hc``
               (chi_max = 8): two interior bonds each, both sweep directions.  Per call: ``LP``, ``RP``, ``W0``, ``W1`` and ``theta`` as
               dense arrays with the charges of every index of every leg (the stand-alone side rebuilds block-sparse tensors and the
               effective Hamiltonian from them), the amplitude, ``IdL`` / ``IdR``, which sides are mixed, ``qtotal_LR``, the truncation
               parameters; the results: dense ``rho_L`` / ``rho_R`` (legs split: [vL, p0, vL*, p0*] / [p1, vR, p1*, vR*]), the magnitude
               sums their rounding error scales with (``mag_L`` / ``mag_R``: sum |mix| (|LP| |W| |theta|) (|LP| |W| |theta|)^T, the same
               products with absolute values throughout), the kept eigenvalues ``S_approx**2``, ``err.eps``, dense ``U S VH``
               ([vL, p0, p1, vR]).  Only calls where the relative gap between the last kept and the first dropped eigenvalue is >= 1e-4
               on both sides are taken (asserted, stored as ``gap``): ``U S VH`` is then well conditioned.
* ``dmrg``     mixer-on runs (amplitude 1e-5, decay 2, disable_after 4, six sweeps, Lanczos always: ``max_N_for_ED = 0``) of the same
               three models at L = 12 / 2 x 4 from product states: per-sweep energies and bond dimensions, per-update energies, final
               entropies, and the sweep after which the mixer was gone.  The XXZ records also hold the reference's MPO (dense tensors with
               charges, ``IdL`` / ``IdR`` per bond, the initial product state): the mixer's perturbation depends on how an MPO distributes
               the couplings over its tensors, and the stand-alone ``xxz_chain_mpo`` distributes them differently (the ladder MPOs agree)."""
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
from make_golden_plus_hc import make_model  # noqa: E402  (the two models of the H + h.c. fixtures, half or full MPO)
from tenpy.algorithms import dmrg, mps_common  # noqa: E402
from tenpy.linalg import np_conserved as npc  # noqa: E402
from tenpy.networks.mps import MPS  # noqa: E402

CASES = [('xxz', 'xxz', dict(Jxx=1., Jz=0.7, hz=0.1), False, dict(L=8), dict(L=12), 8),
         ('peierls_ladder', 'peierls_ladder', dict(t=1., U=4., mu=0., peierls=0.3), False, dict(L=3), dict(L=4), 8),
         ('xxz_plus_hc', 'xxz', dict(Jxx=1., Jz=0.7, hz=0.1), True, dict(L=8), dict(L=12), 8)]
MIXER = {'amplitude': 1.e-5, 'decay': 2., 'disable_after': 4}
GAP = 1.e-4
# The runs of the ``dmrg`` record cut at svd_min = 1e-6 (eigenvalues of rho >= 1e-12).  With the 1e-10 of the other fixtures the cut of
# the first sweeps from a product state falls among eigenvalues of 1e-17 ... 1e-22 that are rounding noise of the eigensolver: which of
# them are kept -- and, as extra directions of the bond, change the energies of the first sweep by 1e-3 -- differs from one correct
# implementation to the next.  The mixer's own eigenvalues (amplitude 1e-5 times couplings squared, >= 1e-9) stay above the cut.
# Recorded as ``min_gap``: the smallest relative gap between the last kept and the first dropped eigenvalue over all updates (the
# ladder has exactly degenerate pairs -- exchange of its legs with complex conjugation -- which chi_max splits at equal weight).
SVD_MIN_DMRG = 1.e-6


def dense(A, labels):
    """(dense array in the order ``labels``, per leg: the charges of every index and qconj)."""
    A = A.copy().itranspose(labels)
    return dict(data=A.to_ndarray(), labels=list(labels), qtotal=np.array(A.qtotal),
                legs=[(np.array(l.to_qflat()), int(l.qconj)) for l in A.legs])


def gap_of(rho, n_keep):
    """Relative gap between the last kept and the first dropped eigenvalue of a density matrix (inf: nothing dropped)."""
    val, _ = npc.eigh(rho)
    val = np.sort(np.clip(val, 0., None) / np.sum(np.clip(val, 0., None)))[::-1]
    if n_keep >= len(val) or val[n_keep] == 0.:
        return np.inf
    return float((val[n_keep - 1] - val[n_keep]) / val[n_keep - 1])


def run(kind, par, plus_hc, size, chi, n_sweeps, dump=None, svd_min=1.e-10):
    M = make_model(kind, dict(par, **size), plus_hc)
    sites = M.lat.mps_sites()
    psi = MPS.from_product_state(sites, ['up', 'down'] * (len(sites) // 2), bc='finite')
    eng = dmrg.TwoSiteDMRGEngine(psi, M, {'mixer': True, 'mixer_params': dict(MIXER), 'combine': True, 'max_N_for_ED': 0,
                                          'trunc_params': {'chi_max': chi, 'svd_min': svd_min}, 'lanczos_params': {}})
    eng.mixer_activate()          # (the reference does this in `run`; the sweeps are driven from here)
    assert eng.mixer is not None
    calls, gaps = [], []
    orig = mps_common.DensityMatrixMixer.mixed_svd_2site

    def spy(self, engine, theta, i0, mix_left, mix_right, qtotal_LR=[None, None]):
        rho_L, rho_R = self.mix_rho(engine, theta, i0, mix_left, mix_right)
        rec = None
        if dump is not None and (engine.sweeps, i0, bool(mix_left)) in dump:
            eff, H = engine.eff_H, engine.env.H
            mix_L, mix_R, IdL, IdR, hc = mps_common._mix_LR(H, i0, self.amplitude)
            # magnitude sums in the order of the SPLIT legs (the pipes permute their indices): [vL, p0 | vL*, p0*], [p1, vR | p1*, vR*]
            th = np.abs(theta.split_legs().itranspose(['vL', 'p0', 'p1', 'vR']).to_ndarray())
            # |LP| |W0| and |W1| |RP| rather than |LHeff|, |RHeff|: sums over the MPO bond may cancel
            lp, rp = (np.abs(t.copy().itranspose(l).to_ndarray()) for t, l in ((eff.LP, ['vR*', 'wR', 'vR']), (eff.RP, ['wL', 'vL', 'vL*'])))
            w0 = np.abs(eff.W0.copy().itranspose(['wL', 'wR', 'p0', 'p0*']).to_ndarray())
            w1 = np.abs(eff.W1.copy().itranspose(['wL', 'wR', 'p1', 'p1*']).to_ndarray())
            aL = np.einsum('aub,uwpq->apwbq', lp, w0)                              # vR* p0 wR vR p0*
            aR = np.einsum('wupq,ubr->wqbpr', w1, rp)                              # wL p1* vL p1 vL*
            f = 2. if hc else 1.
            nl, nr = th.shape[0] * th.shape[1], th.shape[2] * th.shape[3]
            plain_L, plain_R = th.reshape(nl, nr) @ th.reshape(nl, nr).T, th.reshape(nl, nr).T @ th.reshape(nl, nr)
            if mix_left:
                X = np.tensordot(aL, th, ([3, 4], [0, 1]))                          # a p0 w p1 c
                Xw = (X * np.abs(mix_L)[None, None, :, None, None]).reshape(nl, -1)
                mag_L = f * Xw @ X.reshape(nl, -1).T + (plain_L if IdL is None else 0)
            else:
                mag_L = plain_L
            if mix_right:
                X = np.tensordot(th, aR, ([2, 3], [1, 2]))                          # a p0 w p1 r
                Xw = (X * np.abs(mix_R)[None, None, :, None, None]).reshape(-1, nr)
                mag_R = f * Xw.T @ X.reshape(-1, nr) + (plain_R if IdR is None else 0)
            else:
                mag_R = plain_R
            rec = dict(i0=int(i0), sweep=int(engine.sweeps), mix_left=bool(mix_left), mix_right=bool(mix_right), amplitude=float(self.amplitude),
                       IdL=IdL, IdR=IdR, explicit_plus_hc=bool(hc), qtotal_L=None if qtotal_LR[0] is None else np.array(qtotal_LR[0]),
                       trunc_params=dict(chi_max=chi, svd_min=svd_min), chinfo_mod=np.array(theta.chinfo.mod),
                       LP=dense(eff.LP, ['vR*', 'wR', 'vR']), RP=dense(eff.RP, ['wL', 'vL', 'vL*']),
                       W0=dense(eff.W0, ['wL', 'wR', 'p0', 'p0*']), W1=dense(eff.W1, ['wL', 'wR', 'p1', 'p1*']),
                       theta=dense(theta.split_legs(), ['vL', 'p0', 'p1', 'vR']),
                       rho_L=rho_L.copy().itranspose(['(vL.p0)', '(vL*.p0*)']).split_legs().to_ndarray(),
                       rho_R=rho_R.copy().itranspose(['(p1.vR)', '(p1*.vR*)']).split_legs().to_ndarray(),
                       mag_L=(mag_L * (1 + 1.e-6)).astype(np.float32), mag_R=(mag_R * (1 + 1.e-6)).astype(np.float32))      # (float32, rounded up)
        U, S, VH, err, S_a = self.svd_from_rho(engine, rho_L.copy(), rho_R.copy(), theta, qtotal_LR)
        if dump is None:
            gaps.append(min(gap_of(rho_L, U.shape[1]), gap_of(rho_R, VH.shape[0])))
        if rec is not None:
            gap = min(gap_of(rho_L, U.shape[1]), gap_of(rho_R, VH.shape[0]))
            if gap >= GAP and np.isfinite(gap):
                usv = npc.tensordot(npc.tensordot(U, S, axes=['vR', 'vL']), VH, axes=['vR', 'vL'])
                rec.update(S_approx_sq=np.array(S_a)**2, err_eps=float(err.eps), gap=gap, n_keep_L=int(U.shape[1]), n_keep_R=int(VH.shape[0]),
                           USV=usv.split_legs().itranspose(['vL', 'p0', 'p1', 'vR']).to_ndarray())
                calls.append(rec)
        return U, S, VH, err, S_a
    mps_common.DensityMatrixMixer.mixed_svd_2site = spy
    try:
        Es, chis, gone = [], [], None
        for s in range(n_sweeps):
            eng.sweep()
            Es.append(float(np.real(eng.update_stats['E_total'][-1])))
            chis.append(int(max(psi.chi)))
            if eng.mixer is None and gone is None:
                gone = s + 1
    finally:
        mps_common.DensityMatrixMixer.mixed_svd_2site = orig
    H = M.H_MPO
    mpo = None
    if dump is None and kind == 'xxz':      # the mixer's perturbation depends on how the MPO distributes the couplings over its tensors:
        mpo = dict(W=[dense(H.get_W(i), ['wL', 'wR', 'p', 'p*']) for i in range(H.L)], IdL=list(H.IdL), IdR=list(H.IdR),      # the reference's own MPO
                   chinfo_mod=np.array(H.chinfo.mod), init=[int(sites[i].state_labels[l]) for i, l in enumerate(['up', 'down'] * (len(sites) // 2))])
    res = dict(mpo=mpo, svd_min=svd_min, min_gap=min(gaps) if gaps else None, E_sweeps=Es, chi_sweeps=chis, S_ent=np.array(psi.entanglement_entropy()) if eng.mixer is None else None, D_mpo=int(max(M.H_MPO.chi)),
               dtype=str(M.H_MPO.dtype), E_updates=[float(np.real(e)) for e in eng.update_stats['E_total']], mixer_gone_after=gone)
    return res, calls


if __name__ == '__main__':
    out = dict(percall=[], dmrg=[])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, kind, par, hc, small, large, chi in CASES:
            n = 2 * small['L'] if kind != 'xxz' else small['L']
            bonds = (n // 2 - 1, n // 2)
            dump = {(1, b, d) for b in bonds for d in (True, False)}      # the second sweep: the bonds have grown to chi_max
            _, calls = run(kind, par, hc, small, chi, 2, dump)
            got = {(c['i0'], c['mix_left']) for c in calls}
            print(name, 'percall: %d calls' % len(calls), sorted(got), 'gaps', ['%.2e' % c['gap'] for c in calls],
                  'kept', [(c['n_keep_L'], c['n_keep_R']) for c in calls])
            assert got == {(b, d) for b in bonds for d in (True, False)}, "a wanted call has no gap >= 1e-4: choose other bonds"
            assert all(c['gap'] >= GAP for c in calls)
            for c in calls:
                c['name'] = name
            out['percall'] += calls
            res, _ = run(kind, par, hc, large, 24, 6, svd_min=SVD_MIN_DMRG)
            print(name, 'min gap %.2e' % res['min_gap'], 'dmrg E', res['E_sweeps'], 'chi', res['chi_sweeps'], 'mixer gone after sweep', res['mixer_gone_after'])
            out['dmrg'].append(dict(name=name, kind=kind, params=par, explicit_plus_hc=hc, chi=24, n_sweeps=6, mixer_params=dict(MIXER), **large, **res))
    path = os.path.join(HERE, 'mixer.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote mixer.pkl", os.path.getsize(path), "bytes")
