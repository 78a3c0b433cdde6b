"""The factored matvec for an MPO whose charge blocks are small matrices (Hubbard ladder, N-only physical leg: sectors 1, 2, 1) on a
seeded synthetic bond of chi states:
  (a) ms per matvec: LP . theta . (W0 W1) . RP with the MPO step as tpa_mpo_apply_batch  vs  LHeff . theta . RHeff (the route without it);
  (b) the MPO step alone, its bytes by the traffic model itemsize (sum_terms pre d_in post + sum_jobs pre d_out post) as GB/s, next to
      tpa_lincomb_batch for the scalar MPO -- the (N, 2Sz) ladder -- on a theta of the same size, measured in the same run;
  (c) one bond's Lanczos run of N steps: one native call vs the step-by-step route.
Every figure is the median of ``reps`` timed calls after ``warm`` warm-up calls, each call ended by a device synchronise.

    python scripts/heff_blocks_bench.py [chi ...] [--reps 21] [--warm 5] [--complex]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tenpy_amd.algorithms import mps_common as mc
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import LegCharge
from tenpy_amd.models.hubbard import hubbard_ladder_mpo


def bond_leg(chinfo, chi, conserve, n_sec=9, N0=20):
    """A bond leg of ``chi`` states over ``n_sec`` particle-number sectors around N0 with binomial weights; with 2Sz conserved every N
    sector is split evenly over the 2Sz values of its parity (|2Sz| <= 2)."""
    from math import comb
    w = np.array([float(comb(n_sec - 1, k)) for k in range(n_sec)])
    sizes = np.maximum(1, np.floor(chi * w / w.sum()).astype(int))
    sizes[n_sec // 2] += chi - int(sizes.sum())
    charges, widths = [], []
    for k, n in enumerate(sizes):
        N = N0 - n_sec // 2 + k
        if len(conserve) == 1:
            charges.append([N])
            widths.append(int(n))
        else:
            szs = [-2, 0, 2] if N % 2 == 0 else [-1, 1]
            part = [int(n) // len(szs)] * len(szs)
            part[0] += int(n) - sum(part)
            for sz, m in zip(szs, part):
                if m > 0:
                    charges.append([N, sz])
                    widths.append(m)
    order = np.lexsort(np.array(charges).T[::-1])
    charges, widths = np.array(charges)[order], np.array(widths)[order]
    return LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(widths)]), charges, qconj=+1)


def operator(chi, conserve, cplx, seed, factored):
    H = hubbard_ladder_mpo(4, 1., 4., 0., conserve=conserve, peierls=0.3 if cplx else 0.)
    W0, W1 = H.get_W(3), H.get_W(4)
    rng = np.random.default_rng(seed)
    dtype = np.complex128 if cplx else np.float64

    def rnd(size):
        x = rng.standard_normal(size)
        return x + 1j * rng.standard_normal(size) if cplx else x
    bond = bond_leg(W0.chinfo, chi, conserve)
    LP = npc.Array.from_func(rnd, [bond, W0.get_leg('wL').conj(), bond.conj()], dtype=dtype, shape_kw='size', labels=['vR*', 'wR', 'vR'])
    RP = npc.Array.from_func(rnd, [bond, W1.get_leg('wR').conj(), bond.conj()], dtype=dtype, shape_kw='size', labels=['vL', 'wL', 'vL*'])
    eff = mc.TwoSiteH(None, 3, tensors=(LP, RP, W0, W1), factored=factored)
    p = W0.get_leg('p')
    theta = npc.Array.from_func(rnd, [bond, p, p, bond.conj()], dtype=dtype, shape_kw='size', labels=['vL', 'p0', 'p1', 'vR'])
    return eff, theta, int(np.max(bond.get_block_sizes()))


def median_ms(fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('chi', nargs='*', type=int, default=[256, 1024])
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--complex', action='store_true')
    ap.add_argument('--lanczos-steps', type=int, default=10)
    args = ap.parse_args()
    for chi in args.chi:
        rec = dict(chi=chi, dtype='complex128' if args.complex else 'float64', reps=args.reps, warm=args.warm)
        fac, theta, largest = operator(chi, ('N',), args.complex, 7, True)
        fus, _, _ = operator(chi, ('N',), args.complex, 7, False)
        assert fac.factored and not fus.factored
        rec['largest_sector'] = largest
        rec['auto_rule_picks_factored'] = bool(largest >= mc.FACTORED_MIN_SECTOR)
        x4, x2 = fac.combine_theta(theta), fus.combine_theta(theta)
        y4, y2 = fac.matvec(x4), fus.matvec(x2)
        rec['rel_diff_factored_vs_fused'] = float(npc.norm(fac.prepare_svd(y4) - y2) / npc.norm(y2))
        rec['n_theta'] = int(x4._arena.numel())
        # (a), alternating the two routes
        a1 = median_ms(lambda: fac.matvec(x4), args.reps, args.warm)
        a2 = median_ms(lambda: fus.matvec(x2), args.reps, args.warm)
        a1b = median_ms(lambda: fac.matvec(x4), args.reps, args.warm)
        a2b = median_ms(lambda: fus.matvec(x2), args.reps, args.warm)
        rec['matvec_ms_factored_block'] = [a1[0], a1b[0]]
        rec['matvec_ms_fused_heff'] = [a2[0], a2b[0]]
        # (b) the MPO step alone
        fp = fac._fplans
        T1 = fp['p1'].apply(fac._LPf, x4)
        a01 = fp['a01']
        b1 = median_ms(lambda: a01.apply(T1), args.reps, args.warm)
        rec['mpo_step'] = dict(kernel='tpa_mpo_apply_batch', ms=b1[0], bytes=a01.bytes, GBps=a01.bytes / b1[0] / 1e6, n_jobs=a01.n_jobs,
                               n_terms=int(len(a01.terms_host)), max_d=a01.max_d)
        sfac, stheta, _ = operator(chi, ('N', '2*Sz'), args.complex, 7, True)
        assert sfac.factored
        sx4 = sfac.combine_theta(stheta)
        sfac.matvec(sx4)
        sp = sfac._fplans
        sT1 = sp['p1'].apply(sfac._LPf, sx4)
        s01 = sp['a01']
        b2 = median_ms(lambda: s01.apply(sT1), args.reps, args.warm)
        rec['mpo_step_scalar_yardstick'] = dict(kernel='tpa_lincomb_batch', ms=b2[0], bytes=s01.bytes, GBps=s01.bytes / b2[0] / 1e6,
                                                n_jobs=s01.n_jobs, n_terms=int(len(s01.terms_host)), n_theta=int(sx4._arena.numel()))
        # (c) one bond's Lanczos run, native call vs step by step
        n = args.lanczos_steps
        opts = {'N_min': n, 'N_max': n, 'E_tol': 0., 'P_tol': 0.}
        res = {}
        for native in (True, False):
            kb.NATIVE = native
            lz = kb.LanczosGroundState(fac, x4, dict(opts))
            if native:
                assert lz._native_program() is not None
            res[native] = median_ms(lambda: kb.LanczosGroundState(fac, x4, dict(opts)).run(), max(5, args.reps // 3), 2)
        kb.NATIVE = True
        rec['lanczos_%d_steps_ms' % n] = dict(native=res[True][0], step_by_step=res[False][0])
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
