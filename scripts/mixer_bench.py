"""Times one ``mix_rho`` (left side mixed, right side plain: a right-moving update) on a Heisenberg chi = 2048-shaped bond three ways:

  (a) the generic statements through ``LHeff`` (``mixer.generic_mix_rho``: what a mixer update cost before the device route);
  (b) X by the same calls as (c) (``LP . theta`` by the GEMM plan, ``W0`` by ``MpoApplyPlan``), a pre-scaled copy (and, complex data,
      a conjugated one), and the FULL product on ``tpa_gemm_chain``: (b) and (c) differ in the product stage only;
  (c) the device route (``mixer.device_mix_rho``: the same X, one ``tpa_herk_chain`` launch per side).

The bond: random ``LP``, ``RP``, ``theta`` on a bond leg whose Sz sectors follow a steep binomial profile as on a saturated chi = 2048 bond of
the spin-1/2 chain (``--chi`` changes the size), around the bulk MPO tensors of the Heisenberg chain.  Protocol: warm-up calls, then
repeated timed calls between device events; median, minimum and maximum per route.  ``--sweep``: additionally the time per sweep of
the stand-alone driver at chi_max = 512 (L = 64) with the mixer on and off.

    python scripts/mixer_bench.py [--chi 2048] [--reps 10] [--warmup 3] [--sweep]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


PROFILE = (1, 8, 45, 148, 450, 744, 450, 148, 45, 8, 1)      # of 2048: a steep binomial profile, the central sectors hold most states


def sector_sizes(chi):
    """Sizes of the Sz sectors of the bond leg: ``PROFILE`` scaled to ``chi`` states."""
    w = np.array(PROFILE, float)
    s = np.maximum(1, np.floor(chi * w / w.sum()).astype(int))
    s[len(s) // 2] += chi - s.sum()
    return s


def make_bond(chi, rng):
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.linalg.charges import LegCharge
    from tenpy_amd.models.spin_chains import xxz_chain_mpo
    H = xxz_chain_mpo(8, 1., 1., 0.)
    W0, W1 = H.get_W(3), H.get_W(4)
    sizes = sector_sizes(chi)
    n = len(sizes)
    leg = LegCharge.from_qind(W0.chinfo, np.concatenate([[0], np.cumsum(sizes)]), [[2 * (i - n // 2)] for i in range(n)], qconj=+1)
    rnd = rng.standard_normal
    LP = npc.Array.from_func(rnd, [leg, W0.get_leg('wL').conj(), leg.conj()], labels=['vR*', 'wR', 'vR'])
    RP = npc.Array.from_func(rnd, [leg, W1.get_leg('wR').conj(), leg.conj()], labels=['vL', 'wL', 'vL*'])
    theta = npc.Array.from_func(rnd, [leg, W0.get_leg('p'), W1.get_leg('p'), leg.conj()], labels=['vL', 'p0', 'p1', 'vR'])
    theta /= theta.norm()
    return H, (LP, RP, W0, W1), theta


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chi', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sweep', action='store_true')
    args = ap.parse_args()
    import torch
    from tenpy_amd.algorithms import mixer, mps_common
    from tenpy_amd.linalg import np_conserved as npc
    rng = np.random.default_rng(1)
    H, tensors, theta4 = make_bond(args.chi, rng)
    i0 = 3
    fac = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=True)
    fus = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=False)
    assert fac.factored and not fus.factored
    theta2 = fus.combine_theta(theta4)
    w = mixer.mix_weights(H, i0, 1.e-5)
    mix_L = w[0]
    print("bond: chi = %d, sectors of the bond leg %s, largest sector of (vL.p0): %d rows" % (
        args.chi, sector_sizes(args.chi).tolist(), int(np.max(fac.pipeL.get_block_sizes()))))

    def route_a():
        return mixer.generic_mix_rho(fus, H, theta2, i0, 1.e-5, True, False, weights=w)

    def route_b():
        T1 = npc.tensordot(fac._LPf, theta4, axes=['vR', 'vL'])            # X exactly as (c) builds it: the GEMM plan, then MpoApplyPlan
        X = mixer._apply_mpo(T1, fac.W0, True, ('vR*', 'p0', 'wR', 'p1', 'vR'))
        rho_L = npc.tensordot(X.scale_axis(mix_L, 'wR'), X.conj(), axes=[['wR', 'p1', 'vR'], ['wR*', 'p1*', 'vR*']])
        rho_R = npc.tensordot(theta2.conj(), theta2, axes=['(vL*.p0*)', '(vL.p0)'])
        return rho_L, rho_R

    def route_c():
        return mixer.device_mix_rho(fac, H, theta4, i0, 1.e-5, True, False, weights=w)

    got_a, got_c = route_a()[0].to_ndarray(), route_c()[0].to_ndarray()
    print("max |rho_L(c) - rho_L(a)| = %.3g, max |rho_L| = %.3g" % (np.abs(got_a - got_c).max(), np.abs(got_a).max()))
    plan = fac._mixplans['L']
    print("HERK launch (c), left side: %d tasks, %d tiles, %.3f GFLOP on the scheduled tiles of %.3f GFLOP of the full product" % (
        plan.launches[0][0].shape[0], plan.launches[0][3], plan.flops_tiles / 1e9, plan.flops / 1e9))
    res = {}
    for name, fn in (('a generic statements (LHeff prebuilt)', route_a), ('b factored X + full product on tpa_gemm_chain', route_b),
                     ('c factored X + tpa_herk_chain', route_c)):
        med, lo, hi = timed(fn, args.reps, args.warmup)
        res[name[0]] = (med, lo, hi)
        print("(%s: median %.3f ms, min %.3f, max %.3f  (%d timed calls after %d warm-up calls)" % (
            name.replace(' ', ') ', 1), med, lo, hi, args.reps, args.warmup))
    spread_b = res['b'][2] - res['b'][1]
    verdict = "not slower" if res['c'][0] <= res['b'][0] + spread_b else "SLOWER"
    print("(c) against (b): %.3f ms against %.3f ms, run-to-run spread of (b) %.3f ms -> (c) is %s than (b)" % (
        res['c'][0], res['b'][0], spread_b, verdict))
    fus._LHeff = fus._RHeff = None
    torch.cuda.synchronize()
    t0 = time.time()
    fus.combine_Heff(None)
    torch.cuda.synchronize()
    print("building LHeff and RHeff (what (a) needs from a factored operator once per bond): %.3f ms" % (1e3 * (time.time() - t0)))
    if args.sweep:
        from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        from tenpy_amd.networks.mps import MPS
        L = 64
        Hs = xxz_chain_mpo(L, 1., 1., 0.)
        p = spin_half_leg('Sz')[1]
        for mix in (True, None):
            psi = MPS.from_product_state([p] * L, [1, 0] * (L // 2))
            eng = TwoSiteDMRGEngine(psi, Hs, {'trunc_params': {'chi_max': 512, 'svd_min': 1.e-12}, 'mixer': mix,
                                              'mixer_params': {'amplitude': 1.e-5, 'decay': 1., 'disable_after': None}})
            for _ in range(6):
                eng.sweep()
            torch.cuda.synchronize()
            print("stand-alone driver, Heisenberg L = %d, chi_max = 512, mixer %s: sweep times %s s, max chi %d, E = %.10f" % (
                L, 'on' if mix else 'off', ['%.2f' % t for t in eng.sweep_stats['time']], eng.sweep_stats['max_chi'][-1],
                eng.sweep_stats['E'][-1]))


if __name__ == '__main__':
    main()
