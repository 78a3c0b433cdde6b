"""Times projective sampling of a chi-shaped Sz-conserving spin-1/2 chain on the device.  The state is synthetic: seeded random
ISOMETRIES with the block structure of a sweep (the leg construction of ``scripts/measure_bench.py``; every site tensor is
right-canonical, so the state is normalised site by site as ``sample_measurements`` demands), a first site with a 'vL' leg of width 1,
and one more site than is sampled (the last sampled bond keeps its full width):

  (a) generic  ``sample.sample_generic``: the reference's statements, sample by sample -- per (sample, site) a ``tensordot`` of a vector
               with ``B``, ``tensordot(theta.conj(), theta)``, a host read, ``take_slice``, ``norm`` (a host read) and a division; what
               the device path does without the batched route.  For n = 1024 a subset of 64 samples is timed and scaled by 16 (said
               on the line);
  (b) batched  ``sample.device_sample``: one walk for the whole batch, per site one GEMM, one ``tpa_sample_select_batch`` and one
               ``tpa_sample_gather_batch`` launch and one device-to-host copy;
  (c) shares   one walk of (b) with a device synchronisation around the GEMM, the select launch and the gather launch: their shares
               of the walk, the rest being host work (tables, the sort, uploads, the copies of ``out``);
  (d) kernels  the two kernels alone at the middle site, with the bytes of the header's traffic formulas and the bandwidth that
               corresponds to.

(a) and (b) alternate in one process after a warm-up of both, each timed with a device synchronisation inside the timer.  The file
written (``--out``, default profiles/sample.txt) ends with what follows for a single-sample call (``sample.SINGLE``): the device route
only if the slowest batched run with n = 1 is faster than the fastest generic run (a difference beyond the run-to-run spread).

    python scripts/sample_bench.py [--L 100] [--chi 2048] [--reps 3] [--out profiles/sample.txt]
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


def isometry(vL, p, vR, rng):
    """A right-canonical tensor ['vL', 'p', 'vR'] on the given legs: for every sector of 'vL' the rows of its (p, vR) blocks are
    orthonormal (QR of a random matrix on the host)."""
    from tenpy_amd.linalg import np_conserved as npc
    dense = np.zeros((vL.ind_len, p.ind_len, vR.ind_len))
    for a in range(vL.block_number):
        cols = []
        for b in range(p.block_number):
            for c in range(vR.block_number):
                if np.all(vL.chinfo.make_valid(vL.qconj * vL.charges[a] + p.qconj * p.charges[b] + vR.qconj * vR.charges[c]) == 0):
                    cols.append((b, c))
        rows = vL.slices[a + 1] - vL.slices[a]
        width = sum((p.slices[b + 1] - p.slices[b]) * (vR.slices[c + 1] - vR.slices[c]) for b, c in cols)
        assert rows <= width, "a sector of the left leg is wider than what it connects to"
        q, _ = np.linalg.qr(rng.standard_normal((width, rows)))
        at = 0
        for b, c in cols:
            w = vR.slices[c + 1] - vR.slices[c]
            dense[vL.slices[a]:vL.slices[a + 1], p.slices[b], vR.slices[c]:vR.slices[c + 1]] = q[at:at + w].T      # (one state per sector of p)
            at += w
    return npc.Array.from_ndarray(dense, [vL, p, vR], labels=['vL', 'p', 'vR'])


def make_state(n_sites, chi, rng):
    from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
    from tenpy_amd.networks.mps import MPS
    chinfo = ChargeInfo([1])
    p = LegCharge.from_qflat(chinfo, [[1], [-1]], qconj=+1)
    sizes = sector_sizes(chi)
    n = len(sizes)
    leg = LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(sizes)]), [[2 * (i - n // 2)] for i in range(n)], qconj=+1)
    leg1 = LegCharge.from_qind(chinfo, leg.slices, leg.charges + 1, qconj=+1)
    first = LegCharge.from_qflat(chinfo, [[0]], qconj=+1)
    even, odd = isometry(leg, p, leg1.conj(), rng), isometry(leg1, p, leg.conj(), rng)
    Bs = [isometry(first, p, leg1.conj(), rng)] + [(even if i % 2 == 0 else odd) for i in range(1, n_sites)]
    S = [np.ones(1)] + [np.full(chi, 1. / np.sqrt(chi))] * n_sites
    return MPS([p] * n_sites, Bs, S, form='B'), sizes


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
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sample.txt'))
    args = ap.parse_args()
    import torch
    from tenpy_amd.linalg import _device as dev
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.networks import sample
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(7)
    L = args.L
    psi, sizes = make_state(L + 1, args.chi, rng)
    last = L - 1
    say("sample_bench: %s, %d sites sampled of a chain of %d, chi = %d (Sz sectors %s), d = 2, float64"
        % (torch.cuda.get_device_properties(0).gcnArchName.split(':')[0], L, L + 1, args.chi, sizes.tolist()))
    single = None
    for n, n_gen in ((1, 1), (64, 64), (1024, 64)):
        u = np.random.default_rng(100 + n).random((n, L))
        generic = lambda: [sample.sample_generic(psi, 0, last, u=u[s]) for s in range(n_gen)]      # noqa: E731
        batched = lambda: sample.device_sample(psi, n, last, u)      # noqa: E731
        g0, b0 = generic(), batched()          # warm-up of both (plans, tables, allocator)
        same = all(list(g0[s][0]) == b0[0][s].tolist() for s in range(n_gen))
        w_gen = np.array([g0[s][1] for s in range(n_gen)])
        w_dev = np.prod(b0[2][:n_gen], axis=1)
        say("n = %d: outcomes of the first %d samples equal on both routes: %s; max rel difference of a weight %.3g"
            % (n, n_gen, same, np.max(np.abs(w_gen - w_dev) / np.abs(w_gen))))
        t_gen, t_dev = [], []
        for _ in range(args.reps):
            t_gen.append(wall(generic) * n / n_gen)
            t_dev.append(wall(batched))
        sample.reset_stats()
        batched()
        st = dict(sample.sample_stats)
        say("  (a) generic  %s s   (median %.3f)%s" % (" ".join("%.3f" % t for t in t_gen), np.median(t_gen),
                                                        "" if n == n_gen else "   [%d samples timed, scaled by %d]" % (n_gen, n // n_gen)))
        say("  (b) batched  %s s   (median %.4f)   walks %d, tensordots %d, select %d, gather %d, d2h %d"
            % (" ".join("%.4f" % t for t in t_dev), np.median(t_dev), st['walks'], st['tensordots'], st['select_launches'], st['gather_launches'],
               st['d2h']))
        faster = max(t_dev) < min(t_gen)
        say("  batched faster beyond the spread of this call: %s (slowest batched %.4f s, fastest generic %.3f s, ratio of medians %.1f)"
            % (faster, max(t_dev), min(t_gen), np.median(t_gen) / np.median(t_dev)))
        if n == 1:
            single = faster
    # (c) shares of a walk, n = 1024
    n = 1024
    u = np.random.default_rng(100 + n).random((n, L))
    spent = {'gemm': 0., 'select': 0., 'gather': 0.}
    keep = (npc.tensordot, sample.SamplePlan.launch, sample._gather)

    def clocked(name, fn):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*a, **kw)
            torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            return res
        return run
    npc.tensordot, sample.SamplePlan.launch, sample._gather = clocked('gemm', keep[0]), clocked('select', keep[1]), clocked('gather', keep[2])
    try:
        t_all = wall(lambda: sample.device_sample(psi, n, last, u))
    finally:
        npc.tensordot, sample.SamplePlan.launch, sample._gather = keep
    rest = t_all - sum(spent.values())
    say("(c) one walk with n = %d and a device synchronisation around every step: %.4f s = GEMM %.4f (%.0f %%) + select %.4f (%.0f %%) + gather %.4f"
        " (%.0f %%) + host tables, sort, uploads and copies %.4f (%.0f %%)"
        % (n, t_all, spent['gemm'], 100 * spent['gemm'] / t_all, spent['select'], 100 * spent['select'] / t_all, spent['gather'],
           100 * spent['gather'] / t_all, rest, 100 * rest / t_all))
    # (d) the kernels alone at the middle site: the stack of the n samples spread over the sectors like the Schmidt weights
    counts = np.maximum(1, np.round(n * sizes / sizes.sum()).astype(int))
    B = psi.get_B(L // 2, 'B')
    vleg = B.get_leg('vL').conj()
    V = sample._new_stack(vleg, np.arange(len(sizes)), counts, np.float64)
    V._arena.copy_(dev.to_device(np.random.default_rng(3).standard_normal(V._arena.numel())))
    X = npc.tensordot(V, B, axes=['vR', 'vL'])
    rows_n = int(counts.sum())
    plan = sample.SamplePlan.get(X)
    u_dev, out = dev.to_device(np.random.default_rng(4).random(rows_n)), dev.empty(4 * rows_n, np.float64)
    ms = timed(lambda: plan.launch(X, u_dev, out), 10, 3)
    say("(d) tpa_sample_select_batch alone: %d rows, %d segs, %.1f MB by the traffic formula (itemsize sum rows d post): %.3f ms (min %.3f, max %.3f)"
        " = %.2f TB/s" % (rows_n, plan.n_segs, plan.bytes / 1e6, ms[0], ms[1], ms[2], plan.bytes / ms[0] / 1e9))
    host = dev.to_host(out).reshape(rows_n, 4)
    sig = host[:, 0].astype(np.int64)
    seg = plan.seg_of[plan.row_group, sig]
    S = plan.segs_host[seg]
    gr = np.zeros((rows_n, 4), dtype=np.int64)
    gr[:, 0] = S[:, 0] + (np.arange(rows_n) - plan.groups_host[plan.row_group, 2]) * S[:, 1] + (sig - S[:, 4]) * S[:, 3]
    gr[:, 1] = S[:, 3]
    gr[:, 2] = np.concatenate([[0], np.cumsum(S[:-1, 3])])
    gr[:, 3] = np.arange(rows_n)
    dst = dev.empty(int(np.sum(S[:, 3])), np.float64)
    rows_dev = dev.to_device(gr)
    L_ = dev.lib()
    ms = timed(lambda: dev.check(L_.tpa_sample_gather_batch(0, rows_dev.data_ptr(), rows_n, X._arena.data_ptr(), out.data_ptr(), dst.data_ptr(),
                                                            dev.stream()), "gather"), 10, 3)
    gbytes = 2 * 8 * int(np.sum(S[:, 3]))
    say("    tpa_sample_gather_batch alone: %d rows, %.1f MB (2 itemsize sum len): %.3f ms (min %.3f, max %.3f) = %.2f TB/s"
        % (rows_n, gbytes / 1e6, ms[0], ms[1], ms[2], gbytes / ms[0] / 1e9))
    say("single-sample calls (n_samples=None) that follow: %s" % ('device route' if single else 'generic statements'))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write("\n".join(lines) + "\n")


if __name__ == '__main__':
    main()
