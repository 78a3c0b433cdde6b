"""Times ``correlation_function`` rows on the device for a chi-shaped Sz-conserving spin-1/2 chain.  The tensors are seeded random
tensors with the block structure of a sweep, NOT isometries: the values grow along the chain (the differences between the routes are
printed next to max |C|), which does not change what is launched or moved:

  (a) rows     the row-by-row statements (``measure.corr_up_generic``: per start site a walk of generic ``tensordot`` pairs, per value
               ``tensordot(op2, C)`` + ``inner`` and one host read) -- what the device path could do before the stacked route;
  (b) stacked  ``measure.device_corr_up``: one walk, the started rows as a stack, one ``tpa_site_inner_batch`` launch per closing site,
               one device-to-host copy;
  (c) kernel   ``tpa_site_inner_batch`` alone on one stacked X, with the bytes of the header's traffic formula and the bandwidth that
               corresponds to, against the pair it replaces: ``tensordot(op, X)`` + ``inner`` (with the host read of the value) on
               the X of ONE row, times the number of rows.

(a) and (b) alternate in one process after a warm-up of both, each timed with a device synchronisation inside the timer.  The file
written (``--out``, default profiles/measure.txt) ends with the default of ``TPA_MEASURE`` that follows: on only if the slowest stacked
run is faster than the fastest row-by-row run of the same call (a difference beyond the run-to-run spread), off otherwise.

    python scripts/measure_bench.py [--L 100] [--chi 2048] [--reps 3] [--stack 64] [--out profiles/measure.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mixer_bench import sector_sizes, timed  # noqa: E402


def make_state(L, chi, rng):
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
    from tenpy_amd.networks.mps import MPS
    chinfo = ChargeInfo([1])
    p = LegCharge.from_qflat(chinfo, [[1], [-1]], qconj=+1)
    sizes = sector_sizes(chi)
    n = len(sizes)
    leg = LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(sizes)]), [[2 * (i - n // 2)] for i in range(n)], qconj=+1)
    leg1 = LegCharge.from_qind(chinfo, leg.slices, leg.charges + 1, qconj=+1)
    rnd = lambda shape: rng.standard_normal(shape) / np.sqrt(shape[0])      # noqa: E731
    even = npc.Array.from_func(rnd, [leg, p, leg1.conj()], labels=['vL', 'p', 'vR'])
    odd = npc.Array.from_func(rnd, [leg1, p, leg.conj()], labels=['vL', 'p', 'vR'])
    Bs = [(even if i % 2 == 0 else odd) for i in range(L)]
    S = [np.full(chi, 1. / np.sqrt(chi))] * (L + 1)
    return MPS([p] * L, Bs, S, form='B'), sizes


def wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=100)
    ap.add_argument('--chi', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--stack', type=int, default=64)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'measure.txt'))
    args = ap.parse_args()
    import torch
    from tenpy_amd.linalg import _device as dev
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.networks import measure
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(7)
    psi, sizes = make_state(args.L, args.chi, rng)
    say("measure_bench: %s, L = %d, chi = %d (Sz sectors %s), d = 2, float64" % (torch.cuda.get_device_properties(0).gcnArchName.split(':')[0], args.L, args.chi, sizes.tolist()))
    Sz, Sp, Sm = np.diag([0.5, -0.5]), np.array([[0., 1.], [0., 0.]]), np.array([[0., 0.], [1., 0.]])
    sites = list(range(args.L))
    verdict = True
    for name, A, Bm in (('Sz Sz', Sz, Sz), ('Sp Sm', Sp, Sm)):
        hosts = {}
        a, b = psi._site_ops(A, hosts), psi._site_ops(Bm, hosts)
        rows = lambda: measure.corr_up(psi, a, b, sites, sites, None, True, True, why='bench')      # noqa: E731
        stacked = lambda: measure.corr_up(psi, a, b, sites, sites, None, True, True, why=None, hosts=hosts)      # noqa: E731
        r0, s0 = rows(), stacked()          # warm-up of both (plans, tables, allocator)
        scale = max(np.max(np.abs(r0)), 1e-300)
        say("%s: upper triangle, %d values; stacked against rows: max abs difference %.3g of max |C| %.3g"
            % (name, args.L * (args.L - 1) // 2, np.max(np.abs(r0 - s0)), scale))
        t_rows, t_stack = [], []
        for _ in range(args.reps):
            t_rows.append(wall(rows))
            t_stack.append(wall(stacked))
        measure.reset_stats()
        stacked()
        st = dict(measure.measure_stats)
        say("  (a) rows     %s s   (median %.3f)" % (" ".join("%.3f" % t for t in t_rows), np.median(t_rows)))
        say("  (b) stacked  %s s   (median %.3f)   launches %d, transfer tensordots %d, d2h %d, empty slots %.1f %%"
            % (" ".join("%.3f" % t for t in t_stack), np.median(t_stack), st['kernel_launches'], st['transfer_tensordots'], st['d2h'],
               100. * (1. - st['filled'] / max(st['capacity'], 1))))
        faster = max(t_stack) < min(t_rows)
        say("  stacked faster beyond the spread of this call: %s (slowest stacked %.3f s, fastest rows %.3f s, ratio of medians %.2f)"
            % (faster, max(t_stack), min(t_rows), np.median(t_rows) / np.median(t_stack)))
        verdict = verdict and faster
    # (c) the kernel alone
    r = args.L // 2
    op = psi._site_ops(Sp)[r]
    stack = None
    for s in range(args.stack):
        stack = measure._push(stack, measure._start_matrix(psi, op, r - 1), s)
    B = psi.get_B(r, 'B')
    X = npc.tensordot(stack, B, axes=['vR', 'vL'])
    O = psi._site_ops(Sm)[r]
    plan = measure.SiteInnerPlan.get(B, X, [Sm])
    out = dev.zeros(2 * plan.n_stack, np.float64)
    ms = timed(lambda: plan.launch(B, X, out.data_ptr(), n_stack=args.stack), 10, 3)
    X1 = npc.tensordot(measure._start_matrix(psi, op, r - 1), B, axes=['vR', 'vL'])      # the X of one row: 'vR*', 'p', 'vR'

    def pair():         # the two statements the kernel replaces, for one row (the value is read by the host, as in the row-by-row route)
        Cij = npc.tensordot(O, X1, axes=['p*', 'p'])
        Cij.ireplace_labels(['vR*'], ['vL'])
        return npc.inner(B, Cij, axes='labels', do_conj=True)
    ms_pair = timed(pair, 10, 3)
    j = plan.jobs_host
    nbytes = 8 * int(np.sum(j[:, 7] * j[:, 8] * (args.stack * j[:, 6] + -(-args.stack // 8) * j[:, 2])))
    say("(c) kernel: stack of %d rows (capacity %d), %d jobs, %.1f MB by the traffic formula: tpa_site_inner_batch %.3f ms (min %.3f, max %.3f)"
        " = %.2f TB/s; tensordot(op, X) + inner (with its host read) for ONE row %.3f ms (min %.3f, max %.3f), times %d rows = %.1f ms"
        % (args.stack, plan.n_stack, plan.n_jobs, nbytes / 1e6, ms[0], ms[1], ms[2], nbytes / ms[0] / 1e9, ms_pair[0], ms_pair[1], ms_pair[2],
           args.stack, ms_pair[0] * args.stack))
    say("TPA_MEASURE default that follows: %s" % ('on' if verdict else 'off'))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
