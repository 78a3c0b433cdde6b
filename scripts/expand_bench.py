"""Times one subspace expansion of single-site DMRG (a right move: ``theta_expand [(vL.p0), (wR.vR)]``) on the Heisenberg chi = 2048-shaped
site that ``scripts/mixer_bench.py`` builds, three ways:

  (a) the generic statements as a one-site update issues them (``mixer.generic_expand_1site``): the ``LHeff`` build from ``LP`` and ``W0``,
      the scaling pass, the tensordot over the fused leg of length d chi, ``combine_legs`` -- what every mixer update of the reference's
      single-site engine executes on the mirror;
  (b) the same without the ``LHeff`` build (a prebuilt ``LHeff``; the scaling works on a copy);
  (c) the device route (``mixer.device_expand_1site``): ``T1 = LP . theta`` by the GEMM plan over chi and ONE ``tpa_mpo_expand_batch`` launch.

Also the new kernel alone on the tables of (c): time, the bytes its tables account for -- itemsize (sum_terms pre post + sum_rows pre
post) -- and the bandwidth that corresponds to.  Protocol: warm-up calls, then timed calls between device events; median, minimum and
maximum per route.  ``--sweep``: additionally the sweep times of the stand-alone single-site driver with the mixer on (Heisenberg
L = 64, chi_max = 512), to put beside the two-site figure of ``profiles/mixer.txt``.

    python scripts/expand_bench.py [--chi 2048] [--reps 10] [--warmup 3] [--sweep]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mixer_bench import make_bond, sector_sizes, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chi', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sweep', action='store_true')
    args = ap.parse_args()
    import torch
    from tenpy_amd.algorithms import mixer, mps_common
    from tenpy_amd.linalg import _device as dev
    from tenpy_amd.linalg import np_conserved as npc
    rng = np.random.default_rng(1)
    H, (LP, _, W0, _), theta4 = make_bond(args.chi, rng)
    i0, amplitude = 3, 1.e-5
    # one site instead of two: the right bond leg carries the charges of the left one shifted by the site's (2 Sz = +-1)
    from tenpy_amd.linalg.charges import LegCharge
    vL = theta4.get_leg('vL')
    vR = LegCharge.from_qind(W0.chinfo, vL.slices, vL.charges + 1, qconj=+1)
    RP = npc.Array.from_func(rng.standard_normal, [vR, W0.get_leg('wR').conj(), vR.conj()], labels=['vL', 'wL', 'vL*'])
    eff = mps_common.OneSiteH.from_LP_W0_RP(LP, W0, RP, i0)
    assert eff.factored
    theta = npc.Array.from_func(rng.standard_normal, [vL, W0.get_leg('p'), vR.conj()], labels=['vL', 'p0', 'vR'])
    assert theta.stored_blocks > 0
    theta /= theta.norm()
    theta2 = theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0)
    w = mixer.mix_weights(H, i0, np.sqrt(amplitude))
    print("site: chi = %d, sectors of the bond leg %s, d = %d, D = %d" % (args.chi, sector_sizes(args.chi).tolist(), theta.shape[1],
                                                                          W0.get_leg('wR').ind_len))
    LHeff = mixer._heff_1site(eff, True)

    def route_a():
        return mixer.generic_expand_1site(eff, H, theta2, i0, amplitude, True, weights=w)[0]

    def route_b():
        E = npc.tensordot(LHeff.scale_axis(w[0], 'wR'), theta2, axes=['(vR.p0*)', '(vL.p0)'])
        return E.combine_legs(['wR', 'vR'], qconj=-1)

    def route_c():
        return mixer.device_expand_1site(eff, H, theta2, i0, amplitude, True, weights=w)[0]

    got_a, got_c = route_a(), route_c()
    da, dc = (x.split_legs().transpose(['vL', 'p0', 'wR', 'vR']).to_ndarray() for x in (got_a, got_c))
    print("max |(c) - (a)| = %.3g, max |theta_expand| = %.3g; matrix %s, %d blocks, %.1f MB; LHeff %.1f MB" % (
        np.abs(da - dc).max(), np.abs(da).max(), got_c.shape, got_c.stored_blocks, got_c._arena.numel() * 8 / 1e6, LHeff._arena.numel() * 8 / 1e6))
    del da, dc, got_a
    plan = eff._expandplans[True]
    print("tpa_mpo_expand_batch launch (c): %d jobs, %d rows, %d terms; tables account for %.1f MB and %.3f GFLOP" % (
        plan.n_jobs, len(plan.rows_host), len(plan.term_w), plan.bytes / 1e6, plan.flops / 1e9))
    res = {}
    for name, fn in (('a generic statements with the LHeff build', route_a), ('b generic statements, LHeff prebuilt', route_b),
                     ('c LP . theta + tpa_mpo_expand_batch', route_c)):
        med, lo, hi = timed(fn, args.reps, args.warmup)
        res[name[0]] = (med, lo, hi)
        print("(%s: median %.3f ms, min %.3f, max %.3f  (%d timed calls after %d warm-up calls)" % (
            name.replace(' ', ') ', 1), med, lo, hi, args.reps, args.warmup))
    print("(c) against (a): %.3f ms against %.3f ms; against (b): %.3f ms -> the device route is %s than the generic route" % (
        res['c'][0], res['a'][0], res['b'][0], "not slower" if res['c'][0] <= res['a'][0] else "SLOWER"))
    # the kernel alone, on the tables and operands of (c)
    T1 = npc.tensordot(eff._LPf, theta, axes=['vR', 'vL'])
    out = dev.empty(plan.total, plan.dtype)
    L = dev.lib()

    def kernel():
        dev.check(L.tpa_mpo_expand_batch(dev.code(plan.dtype), plan.jobs_dev.data_ptr(), plan.n_jobs, plan.rows_dev.data_ptr(),
                                         plan.terms_dev.data_ptr(), plan.max_cols, T1._arena.data_ptr(), None, out.data_ptr(), dev.stream()),
                  "mpo_expand")
    med, lo, hi = timed(kernel, args.reps, args.warmup)
    print("tpa_mpo_expand_batch alone: median %.3f ms, min %.3f, max %.3f; %.1f MB by its tables -> %.0f GB/s at the median "
          "(bytes moved by hardware counters: not measured)" % (med, lo, hi, plan.bytes / 1e6, plan.bytes / med / 1e6))
    med, lo, hi = timed(lambda: npc.tensordot(eff._LPf, theta, axes=['vR', 'vL']), args.reps, args.warmup)
    print("T1 = LP . theta alone: median %.3f ms, min %.3f, max %.3f" % (med, lo, hi))
    if args.sweep:
        from tenpy_amd.algorithms.dmrg import SingleSiteDMRGEngine
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        from tenpy_amd.networks.mps import MPS
        n = 64
        Hs = xxz_chain_mpo(n, 1., 1., 0.)
        p = spin_half_leg('Sz')[1]
        for route in ('1', '0'):
            os.environ['TPA_EXPAND_DEVICE'] = route
            psi = MPS.from_product_state([p] * n, [1, 0] * (n // 2))
            eng = SingleSiteDMRGEngine(psi, Hs, {'trunc_params': {'chi_max': 512, 'svd_min': 1.e-12}, 'mixer': True,
                                                 'mixer_params': {'amplitude': 1.e-5, 'decay': 1., 'disable_after': None}})
            for _ in range(6):
                eng.sweep()
            torch.cuda.synchronize()
            print("stand-alone single-site driver, Heisenberg L = %d, chi_max = 512, mixer on, TPA_EXPAND_DEVICE=%s: sweep times %s s, "
                  "max chi %d, E = %.10f" % (n, route, ['%.2f' % t for t in eng.sweep_stats['time']], eng.sweep_stats['max_chi'][-1],
                                             eng.sweep_stats['E'][-1]))
        os.environ.pop('TPA_EXPAND_DEVICE', None)


if __name__ == '__main__':
    main()
