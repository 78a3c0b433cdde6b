"""Stand-alone two-site DMRG on models built with ``explicit_plus_hc=True`` (the MPO holds half of H, the effective Hamiltonian is
``H_eff + H_eff^dagger``): the XXZ chain L = 100 at chi = 512 (BASELINE config 2) and the Fermi-Hubbard ladder 2 x 40 at chi = 1024
(config 4), three legs each:

  full     the full MPO (``explicit_plus_hc=False``);
  plus_hc  the half MPO, ``H_eff + H_eff^dagger`` as one operator on the direct sum along the MPO bond (``mps_common.PlusHcH``);
  old      the half MPO with ``TPA_PLUS_HC=0``: ``SumNpcLinearOperator(eff_H, generic adjoint)``, the routing before the doubled
           operator existed -- the yardstick.

Protocol (``bench.py``): from the Neel product state an untimed chi ramp of single sweeps chi = 64, 64, 128, ..., chi / 2 (run once, on
the full MPO; every leg starts from a copy of that state), then per leg ``--warmup`` sweeps at the target chi and ``--steps`` timed
ones.  Reported per leg: seconds per timed sweep (each), the energy, launches per matvec (ops of the launch program of the middle
bond; the old route has no program: two plain matvecs and an axpy per step, enqueued from Python), and for ``plus_hc`` the time to
build the doubled environments of a bond (median over the middle bonds, synchronised, caches bypassed).

    python scripts/plus_hc_bench.py [--models xxz,hubbard] [--chi-xxz 512] [--chi-hubbard 1024] [--L-xxz 100] [--Lx 40] [--steps 2] [--warmup 2]
"""
import argparse
import os
import pickle
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tenpy_amd.algorithms import mps_common as mc
from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine, _plus_hc
from tenpy_amd.linalg import _device as dev
from tenpy_amd.networks.mps import MPS


def make(model, n, plus_hc):
    if model == 'xxz':
        from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
        return xxz_chain_mpo(n, 1., 1., 0., explicit_plus_hc=plus_hc), spin_half_leg('Sz')[1], [1, 0]
    from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
    return hubbard_ladder_mpo(n // 2, 1., 8., 0., explicit_plus_hc=plus_hc), spinful_fermion_leg()[1], [1, 2]


def sync():
    dev.torch().cuda.synchronize()


def engine(psi, H, chi):
    return TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': chi, 'svd_min': 1.e-10}, 'lanczos_params': {'N_min': 2, 'N_max': 8}})


def timed_sweep(eng):
    sync()
    t0 = time.time()
    eng.sweep()
    sync()
    return time.time() - t0


def program_ops(eng, route):
    i0 = eng.psi.L // 2 - 1
    eff = mc.TwoSiteH(eng.env, i0)
    theta = eff.combine_theta(eng.psi.get_theta(i0, n=2))
    if route != 'full':
        eff = _plus_hc(eff)
    got = eff.native_input(theta) if hasattr(eff, 'native_input') else None
    return None if got is None else int(len(got[1][0]))


def doubled_build_ms(eng):
    L = eng.psi.L
    times = []
    for i0 in range(max(1, L // 2 - 5), min(L - 2, L // 2 + 5)):
        LP, RP = eng.env.get_LP(i0), eng.env.get_RP(i0 + 1)
        sync()
        t0 = time.time()
        a, b = mc._plus_hc_env(LP, True), mc._plus_hc_env(RP, False)
        sync()
        times.append(1e3 * (time.time() - t0))
        mb = (a._arena.numel() + b._arena.numel()) * a._arena.element_size() / 1e6
    return float(np.median(times)), mb


def run_model(model, n, chi, args):
    print("== %s: L = %d, chi = %d, %d warm-up + %d timed sweeps per leg" % (model, n, chi, args.warmup, args.steps), flush=True)
    H_full, p, cell = make(model, n, False)
    psi = MPS.from_product_state([p] * n, cell * (n // 2))
    eng = engine(psi, H_full, 64)
    ramp = [64]
    while ramp[-1] * 2 <= chi // 2:
        ramp.append(ramp[-1] * 2)
    for c in [64] + ramp:
        eng.trunc_params['chi_max'] = c
        t = timed_sweep(eng)
        print("   ramp chi = %4d: %.2f s, E = %.10f" % (c, t, eng.sweep_stats['E'][-1]), flush=True)
    start = pickle.dumps(psi, protocol=4)
    del eng
    res = {}
    for route in ('full', 'plus_hc', 'old'):
        mc.PLUS_HC = route != 'old'
        H = H_full if route == 'full' else make(model, n, True)[0]
        eng = engine(pickle.loads(start), H, chi)
        for _ in range(args.warmup):
            timed_sweep(eng)
        ts = [timed_sweep(eng) for _ in range(args.steps)]
        ops = program_ops(eng, route)
        line = "   %-8s MPO D = %2d: s per sweep %s, E = %.10f, launches per matvec: %s" % (
            route, max(H.chi), ' '.join('%.3f' % t for t in ts), eng.sweep_stats['E'][-1],
            ops if ops is not None else "no program (2 x plain matvec + axpy per step, enqueued from Python)")
        if route == 'plus_hc':
            ms, mb = doubled_build_ms(eng)
            line += "; doubled LP + RP of a middle bond: %.2f ms (%.1f MB written), cache: %r" % (ms, mb, mc.plus_hc_stats)
        print(line, flush=True)
        res[route] = min(ts)
        del eng
    mc.PLUS_HC = True
    print("   plus_hc / old = %.2f, plus_hc / full = %.2f (best sweeps)" % (res['plus_hc'] / res['old'], res['plus_hc'] / res['full']), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='xxz,hubbard')
    ap.add_argument('--chi-xxz', type=int, default=512)
    ap.add_argument('--chi-hubbard', type=int, default=1024)
    ap.add_argument('--L-xxz', type=int, default=100)
    ap.add_argument('--Lx', type=int, default=40)
    ap.add_argument('--steps', type=int, default=2)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    for model in args.models.split(','):
        if model == 'xxz':
            run_model('xxz', args.L_xxz, args.chi_xxz, args)
        else:
            run_model('hubbard', 2 * args.Lx, args.chi_hubbard, args)
