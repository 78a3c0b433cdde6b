"""Times ``mutinf_two_site`` on the device for the chi-shaped Sz-conserving spin-1/2 chain of ``scripts/measure_bench.py`` (seeded
random tensors with the block structure of a sweep, NOT isometries: the "density matrices" are not normalised and grow along the chain,
which does not change what is launched or moved; the difference between the routes is printed next to the largest entry):

  (a) generic  ``rho.mutinf_generic``: the reference's statement sequence on ``npc`` -- per pair three ``tensordot`` s, a
               ``combine_legs``, a block ``eigvalsh`` and its host read; it uses only entry points the parent commit has;
  (b) stacked  ``rho.mutinf_two_site`` with the stacked walk: per site and charge difference one GEMM pair and one
               ``tpa_site_rho_batch`` launch, one device-to-host copy per walk, eigenvalues on the host;
  (c) kernel   ``tpa_site_rho_batch`` alone on one stacked X, with the bytes of the header's traffic formula, against those bytes
               divided by the measured HBM bandwidth of the MI355X (6.29 TB/s, float4 copy).

(a) and (b) alternate in one process after a warm-up of both, each timed with a device synchronisation inside the timer; all times of
all repetitions are printed (the run-to-run spread).  The file written (``--out``, default profiles/mutinf.txt) ends with the default of
``TPA_MUTINF`` that follows: on only if, for every ``max_range``, the slowest stacked run is faster than the fastest generic run.

    python scripts/mutinf_bench.py [--L 100] [--chi 2048] [--reps 3] [--ranges 8,32] [--out profiles/mutinf.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from measure_bench import make_state, wall  # noqa: E402
from mixer_bench import timed  # noqa: E402

HBM_TBS = 6.29      # measured float4 copy on the MI355X (8.0 TB/s spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--L', type=int, default=100)
    ap.add_argument('--chi', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--ranges', default='8,32')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mutinf.txt'))
    args = ap.parse_args()
    import torch
    from tenpy_amd.linalg import _device as dev
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.networks import measure, rho
    lines = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def say(text):
        print(text, flush=True)
        lines.append(text)
        with open(args.out, 'w') as f:          # (rewritten after every line: a run that is cut short leaves what it measured)
            f.write("\n".join(lines) + "\n")

    rng = np.random.default_rng(7)
    psi, sizes = make_state(args.L, args.chi, rng)
    say("mutinf_bench: %s, L = %d, chi = %d (Sz sectors %s), d = 2, float64" % (torch.cuda.get_device_properties(0).gcnArchName.split(':')[0], args.L, args.chi, sizes.tolist()))
    verdict = True
    for max_range in [int(r) for r in args.ranges.split(',')]:
        generic = lambda: rho.mutinf_generic(psi, max_range, 1)      # noqa: E731
        stacked = lambda: rho.mutinf_two_site(psi, max_range, 1, why=None)      # noqa: E731
        g0, s0 = rho.two_site_rho_generic(psi, max_range), rho.device_two_site_rho(psi, max_range)      # warm-up of both (plans, tables, allocator)
        assert np.array_equal(g0[0], s0[0])
        dev_, top = max(float(np.max(np.abs(a - b))) for a, b in zip(g0[1], s0[1])), max(float(np.max(np.abs(a))) for a in g0[1])
        say("max_range = %d: %d pairs; density matrices stacked against generic: max abs difference %.3g of max |rho| %.3g" % (max_range, len(g0[0]), dev_, top))
        del g0, s0
        generic(), stacked()
        t_gen, t_stack = [], []
        for _ in range(args.reps):
            t_gen.append(wall(generic))
            t_stack.append(wall(stacked))
        rho.reset_stats()
        stacked()
        st = dict(rho.rho_stats)
        say("  (a) generic  %s s   (median %.3f)" % (" ".join("%.3f" % t for t in t_gen), np.median(t_gen)))
        say("  (b) stacked  %s s   (median %.3f)   walks %d, launches %d, transfer steps %d, d2h %d, slots %d of %d, rows per stack %d"
            % (" ".join("%.3f" % t for t in t_stack), np.median(t_stack), st['walks'], st['kernel_launches'], st['transfer_steps'], st['d2h'],
               st['slots'], st['slots_full'], st['ring_rows']))
        faster = max(t_stack) < min(t_gen)
        say("  stacked faster beyond the spread of this call: %s (slowest stacked %.3f s, fastest generic %.3f s, ratio of medians %.2f)"
            % (faster, max(t_stack), min(t_gen), np.median(t_gen) / np.median(t_stack)))
        verdict = verdict and faster
    # (c) the closing launch alone: the neutral stack (two slots per row) of 32 rows
    r = args.L // 2
    leg = psi.p_legs[r - 1]
    made, stack, n_rows = {}, None, 32
    n_slots = 2 * n_rows
    for s in range(n_slots):
        C = measure._start_matrix(psi, rho._unit(leg, s % 2, s % 2, made), r - 1)
        stack = C.add_leg(measure._stack_leg(C.chinfo, n_slots), s, axis=1, label='s') if stack is None else measure._push(stack, C, s)
    B = psi.get_B(r, 'B')
    X = npc.tensordot(stack, B, axes=['vR', 'vL'])
    plan = rho.SiteRhoPlan.get(B, X)
    out = dev.zeros(2 * plan.n_stack * plan.out_size, np.float64)
    ms = timed(lambda: plan.launch(B, X, out.data_ptr()), 10, 3)
    floor_ms = plan.bytes / (HBM_TBS * 1e12) * 1e3
    say("(c) kernel: stack of %d slots (%d rows), %d jobs, %.1f MB by the traffic formula: tpa_site_rho_batch %.3f ms (min %.3f, max %.3f)"
        " = %.2f TB/s; the bytes at %.2f TB/s: %.3f ms (%.0f %% of it)"
        % (plan.n_stack, n_rows, plan.n_jobs, plan.bytes / 1e6, ms[0], ms[1], ms[2], plan.bytes / ms[0] / 1e9, HBM_TBS, floor_ms,
           100. * floor_ms / ms[0]))
    say("TPA_MUTINF default that follows: %s" % ('on' if verdict else 'off'))


if __name__ == '__main__':
    main()
