"""Times ``MPO.expectation_value`` and ``MPO.variance`` of the Heisenberg chain on the device for a chi-shaped Sz-conserving spin-1/2
chain (outer bonds of dimension 1, every bond inside with the sector profile of a sweep).  The tensors are seeded random tensors, NOT
isometries: the values grow along the chain (the differences between the routes are printed relative to the value), which does not
change what is launched or moved:

  (a) statements  ``TPA_MPO_MOMENTS=0``: the reference's statements on the mirror (``MPOEnvironment.full_contraction``; the loop of
                  ``MPO.variance``: four generic ``tensordot`` per site) -- the route before the walk, the yardstick;
  (b) product     the walk of ``networks/moments.py`` with the product table of the pair step (one launch per site);
  (c) two_pass    the walk with the two single-layer passes.

All routes alternate in one process after a first call of each, every timed call ends with a device synchronisation.  The first call
of every route is timed too and printed on its own: it builds the host tables (the pair tensors of every site, the plans of the MPO
step, the GEMM plans) that the warm calls replay, and ``variance`` is typically called once after a run.  ``--range K`` replaces the
Heisenberg MPO (D = 5) by a long-range XXZ chain of K exponentials (D = 3 K + 2).  The file written
(``--out``) ends with the verdict for this shape: the walk counts as faster only if its slowest run beats the fastest run of the
statements (a difference beyond the run-to-run spread).  ``--profile MODE`` runs one warm ``variance`` call of one route (``off``,
``product``, ``two_pass``) after a warm-up and nothing else: the run to put under ``rocprofv3 --kernel-trace --stats``.

    python scripts/moments_bench.py [--L 100] [--chi 2048] [--range 0] [--reps 3] [--out profiles/mpo_moments.txt] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mixer_bench import sector_sizes  # noqa: E402


def make_chain(L, chi, rng, k=0):
    """``(psi, H, sector sizes)``: L even; the bonds alternate between two legs of the same sector sizes whose charges differ by one."""
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.linalg.charges import LegCharge
    from tenpy_amd.models.spin_chains import long_range_xxz_mpo, spin_half_leg, xxz_chain_mpo
    from tenpy_amd.networks.mps import MPS
    assert L % 2 == 0
    chinfo, p = spin_half_leg('Sz')
    sizes = sector_sizes(chi)
    n = len(sizes)
    leg = LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(sizes)]), [[2 * (i - n // 2)] for i in range(n)], qconj=+1)
    leg1 = LegCharge.from_qind(chinfo, leg.slices, leg.charges + 1, qconj=+1)
    end = LegCharge.from_qflat(chinfo, [[0]], qconj=+1)
    rnd = lambda shape: rng.standard_normal(shape) / np.sqrt(shape[0] * shape[1])      # noqa: E731
    bonds = [end] + [(leg1 if i % 2 == 1 else leg) for i in range(1, L)] + [end]
    made = {}
    Bs = []
    for i in range(L):
        key = (id(bonds[i]), id(bonds[i + 1]))
        if key not in made:
            made[key] = npc.Array.from_func(rnd, [bonds[i], p, bonds[i + 1].conj()], labels=['vL', 'p', 'vR'])
        Bs.append(made[key])
    S = [np.full(b.ind_len, 1. / np.sqrt(b.ind_len)) for b in bonds]
    return MPS([p] * L, Bs, S, form='B'), (long_range_xxz_mpo(L, k) if k else xxz_chain_mpo(L, 1., 1., 0.)), sizes


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


ROUTES = {'statements': ('0', 'auto'), 'product': ('1', 'product'), 'two_pass': ('1', 'two_pass')}


def route(name):
    os.environ['TPA_MPO_MOMENTS'], os.environ['TPA_MPO_MOMENTS_PAIR'] = ROUTES[name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=100)
    ap.add_argument('--chi', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--range', type=int, default=0, dest='k')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mpo_moments.txt'))
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--profile', choices=['off', 'product', 'two_pass'])
    args = ap.parse_args()
    import torch
    from tenpy_amd.networks import moments
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    psi, H, sizes = make_chain(args.L, args.chi, np.random.default_rng(7), args.k)
    if args.profile:
        route({'off': 'statements'}.get(args.profile, args.profile))
        H.variance(psi)
        t, _ = wall(lambda: H.variance(psi))
        print("moments_bench --profile %s: chi = %d, one warm variance call %.3f s" % (args.profile, args.chi, t), flush=True)
        return
    say("moments_bench: %s, %s, L = %d, chi = %d (Sz sectors %s), D = %d, d = 2, float64"
        % (torch.cuda.get_device_properties(0).gcnArchName.split(':')[0], "long-range XXZ chain" if args.k else "Heisenberg chain", args.L,
           args.chi, sizes.tolist(), max(H.chi)))
    calls = {'expectation_value': lambda: H.expectation_value(psi), 'variance': lambda: H.variance(psi)}
    verdict = True
    for cname, fn in calls.items():
        names = ['statements', 'product'] + (['two_pass'] if cname == 'variance' else [])
        first, t_first = {}, {}
        for name in names:                  # the first call of every route (pair tensors, plans, tables, allocator)
            route(name)
            t_first[name], first[name] = wall(fn)
        times = {name: [] for name in names}
        for _ in range(args.reps):
            for name in names:
                route(name)
                times[name].append(wall(fn)[0])
        route('product')
        moments.reset_stats()
        fn()
        st = dict(moments.moments_stats)
        say("%s: %s" % (cname, ", ".join("%s %.15g" % (n, first[n]) for n in names)))
        for name in names:
            label = {'statements': '(a) statements', 'product': '(b) product   ', 'two_pass': '(c) two_pass  '}[name]
            rel = abs(first[name] - first['statements']) / abs(first['statements'])
            say("  %s first call %.3f s, then %s s   (median %.3f)   relative difference to (a) %.2g"
                % (label, t_first[name], " ".join("%.3f" % t for t in times[name]), np.median(times[name]), rel))
        say("  walk: %d grouped GEMMs, %d MPO-step launches, %d device-to-host copy%s"
            % (st['gemms'], st['step_launches'], st['d2h'], "" if st['device'] else "   DECLINED: %r" % (st['why'],)))
        for name in names[1:]:
            faster = max(times[name]) < min(times['statements'])
            say("  %s faster beyond the spread of this call: %s (slowest %.3f s, fastest statements %.3f s, ratio of medians %.2f)"
                % (name, faster, max(times[name]), min(times['statements']), np.median(times['statements']) / np.median(times[name])))
            if name == 'product':
                verdict = verdict and faster
    say("chi = %d: the walk (product table) is faster than the statements for both calls: %s" % (args.chi, verdict))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a' if args.append else 'w') as f:
        f.write("\n".join(lines) + "\n\n")


if __name__ == '__main__':
    main()
