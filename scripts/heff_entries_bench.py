"""The factored matvec with the entry-by-entry MPO step (``MpoEntryApplyPlan``, tpa_mpo_entry_apply_batch) on seeded synthetic bonds
of chi states, for the two kinds of MPO it serves:
  * 'ladder' : the (N, 2Sz) Hubbard ladder with its MPO bond legs sorted and bunched (blocks wider than 1);
  * 'bosons' : a Bose-Hubbard chain with Nmax = 9 and parity conserved (sectors 5 and 5: two-site product 25 > TPA_MPO_APPLY_MAXD).
Figures:
  (a) ms per matvec of the new route against the route ``TPA_MPO_ENTRY_APPLY=0`` takes for the same bond (LHeff . theta . RHeff),
      alternating, and whether the new route is the slower one;
  (b) the MPO step alone, its bytes by the traffic model itemsize (sum_terms pre post + sum_jobs pre n_rows post) as GB/s, next to
      the SAME tables run through tpa_lincomb_batch with one job per destination row, in the same run; both timed the same way, as
      bare library calls into one preallocated destination: per call ended by a synchronise, and per launch of ``--batch`` launches
      back to back between two device events.
Every figure is the median of ``reps`` timed calls after ``warm`` warm-up calls, each call ended by a device synchronise.

    python scripts/heff_entries_bench.py [chi ...] [--reps 21] [--warm 5] [--batch 50] [--complex]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from heff_blocks_bench import bond_leg, median_ms
from tenpy_amd.algorithms import mps_common as mc
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.models.hubbard import hubbard_ladder_mpo
from tenpy_amd.networks.mpo import mpo_from_dense


def sorted_pair(W0, W1):
    """W0, W1 with their three MPO bond legs sorted by charge and bunched (the same permutation on both sides of the common bond)."""
    chinfo = W0.chinfo
    legs = [W0.get_leg('wL'), W1.get_leg('wL'), W1.get_leg('wR').conj()]
    perms = [np.lexsort(l.to_qflat().T) for l in legs]
    new = [LegCharge.from_qflat(chinfo, l.to_qflat()[p], qconj=l.qconj).bunch()[1] for l, p in zip(legs, perms)]
    out = []
    for k, W in enumerate((W0, W1)):
        dense = W.transpose(['wL', 'wR', 'p', 'p*']).to_ndarray()[perms[k]][:, perms[k + 1]]
        out.append(npc.Array.from_ndarray(dense, [new[k], new[k + 1].conj(), W.get_leg('p'), W.get_leg('p*')], dtype=W.dtype,
                                          qtotal=W.qtotal, labels=['wL', 'wR', 'p', 'p*']))
    return out


def boson_pair(Nmax=9, t=1., U=2., mu=0.5):
    chinfo = ChargeInfo([2], ['parity_N'])
    occ = [n for n in range(Nmax + 1) if n % 2 == 0] + [n for n in range(Nmax + 1) if n % 2 == 1]
    d = Nmax + 1
    p = LegCharge.from_qind(chinfo, [0, (Nmax + 2) // 2, d], [[0], [1]])
    b = np.zeros((d, d))
    for k, n in enumerate(occ):
        if n > 0:
            b[occ.index(n - 1), k] = np.sqrt(n)
    n_op = np.diag(np.array(occ, dtype=float))
    W = np.zeros((4, 4, d, d))
    W[0, 0] = W[3, 3] = np.eye(d)
    W[0, 1], W[0, 2] = b.T, b
    W[0, 3] = 0.5 * U * n_op @ (n_op - np.eye(d)) - mu * n_op
    W[1, 3], W[2, 3] = -t * b, -t * b.T
    H = mpo_from_dense([W[0:1], W, W, W[:, 3:4]], [p] * 4, chinfo)
    return H.get_W(1), H.get_W(2)


def parity_leg(chinfo, chi):
    return LegCharge.from_qind(chinfo, [0, chi // 2, chi], [[0], [1]], qconj=+1)


def operator(model, chi, cplx, seed):
    if model == 'ladder':
        H = hubbard_ladder_mpo(4, 1., 4., 0., conserve=('N', '2*Sz'), peierls=0.3 if cplx else 0.)
        W0, W1 = sorted_pair(H.get_W(3), H.get_W(4))
        bond = bond_leg(W0.chinfo, chi, ('N', '2*Sz'))
    else:
        W0, W1 = boson_pair()
        bond = parity_leg(W0.chinfo, chi)
    rng = np.random.default_rng(seed)
    dtype = np.complex128 if cplx else np.float64

    def rnd(size):
        x = rng.standard_normal(size)
        return x + 1j * rng.standard_normal(size) if cplx else x
    LP = npc.Array.from_func(rnd, [bond, W0.get_leg('wL').conj(), bond.conj()], dtype=dtype, shape_kw='size', labels=['vR*', 'wR', 'vR'])
    RP = npc.Array.from_func(rnd, [bond, W1.get_leg('wR').conj(), bond.conj()], dtype=dtype, shape_kw='size', labels=['vL', 'wL', 'vL*'])
    p = W0.get_leg('p')
    theta = npc.Array.from_func(rnd, [bond, p, p, bond.conj()], dtype=dtype, shape_kw='size', labels=['vL', 'p0', 'p1', 'vR'])
    new = mc.TwoSiteH(None, 3, tensors=(LP, RP, W0, W1), factored=True)
    keep = mc.ENTRY_APPLY
    mc.ENTRY_APPLY = 0
    try:
        old = mc.TwoSiteH(None, 3, tensors=(LP, RP, W0, W1), factored=True)
    finally:
        mc.ENTRY_APPLY = keep
    return new, old, theta, int(np.max(bond.get_block_sizes()))


def event_ms(fn, batch, rounds):
    """ms per launch: ``batch`` calls back to back between two device events; the median over ``rounds`` such rounds."""
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / batch)
    return float(np.median(ts))


def lincomb_tables(plan):
    """The plan's rows and terms as tpa_lincomb_batch tables: one job per destination row (pre x post slab, row stride dst_ld)."""
    jobs = []
    for dst_off, pre, n_rows, post, row_begin, dst_ld, _, _ in plan.jobs_host.tolist():
        for o in range(n_rows):
            t0, nt = plan.rows_host[row_begin + o].tolist()
            jobs.append([dst_off + o * post, pre, post, dst_ld or n_rows * post, t0, nt, 0, 0])
    return np.array(jobs, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('chi', nargs='*', type=int, default=[256, 1024])
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--warm', type=int, default=5)
    ap.add_argument('--complex', action='store_true')
    ap.add_argument('--models', default='ladder,bosons')
    ap.add_argument('--batch', type=int, default=50)
    args = ap.parse_args()
    for model in args.models.split(','):
        for chi in args.chi:
            rec = dict(model=model, chi=chi, dtype='complex128' if args.complex else 'float64', reps=args.reps, warm=args.warm)
            new, old, theta, largest = operator(model, chi, args.complex, 7)
            assert new.factored and not old.factored
            rec['largest_sector'] = largest
            x4, x2 = new.combine_theta(theta), old.combine_theta(theta)
            y4, y2 = new.matvec(x4), old.matvec(x2)
            rec['rel_diff_new_vs_old'] = float(npc.norm(new.prepare_svd(y4) - y2) / npc.norm(y2))
            rec['n_theta'] = int(x4._arena.numel())
            a1 = median_ms(lambda: new.matvec(x4), args.reps, args.warm)
            a2 = median_ms(lambda: old.matvec(x2), args.reps, args.warm)
            a1b = median_ms(lambda: new.matvec(x4), args.reps, args.warm)
            a2b = median_ms(lambda: old.matvec(x2), args.reps, args.warm)
            rec['matvec_ms_entry_route'] = [a1[0], a1b[0]]
            rec['matvec_ms_switch_0_route'] = [a2[0], a2b[0]]
            rec['entry_route_slower'] = bool(min(a1[0], a1b[0]) > min(a2[0], a2b[0]))
            fp = new._fplans
            a01 = fp['a01']
            assert isinstance(a01, mc.MpoEntryApplyPlan)
            T1 = fp['p1'].apply(new._LPf, x4)
            # both entry points as bare library calls into one preallocated destination: (i) a call ended by a synchronise,
            # (ii) `--batch` calls back to back between two device events (the kernel with the host out of the picture)
            T3 = a01.apply(T1)
            ref = dev.to_host(T3._arena).copy()
            L = dev.lib()
            code, src_p, dst_p = dev.code(a01.dtype), T1._arena.data_ptr(), T3._arena.data_ptr()

            def entry():
                dev.check(L.tpa_mpo_entry_apply_batch(code, a01.jobs_dev.data_ptr(), a01.n_jobs, a01.rows_dev.data_ptr(),
                                                      a01.terms_dev.data_ptr(), a01.max_cols, src_p, dst_p, dev.stream()), "mpo_entry_apply")
            ljobs = lincomb_tables(a01)
            rec['mpo_step_bytes'] = a01.bytes
            rec['mpo_step_tables'] = dict(n_jobs=a01.n_jobs, n_rows=int(len(a01.rows_host)), n_terms=int(len(a01.terms_host)),
                                          lincomb_jobs=int(len(ljobs)))
            if len(ljobs) > 60000:
                rec['mpo_step_as_lincomb'] = 'more than 60000 jobs (one per row): not one launch'
                print(json.dumps(rec), flush=True)
                continue
            jd = dev.to_device(ljobs)
            max_elems = int(np.max(ljobs[:, 1] * ljobs[:, 2]))

            def lincomb():
                dev.check(L.tpa_lincomb_batch(code, jd.data_ptr(), len(ljobs), a01.terms_dev.data_ptr(), max_elems, src_p, dst_p,
                                              dev.stream()), "lincomb")
            T3._arena.zero_()
            lincomb()
            rec['lincomb_max_abs_diff'] = float(np.abs(dev.to_host(T3._arena) - ref).max())
            T3._arena.zero_()
            entry()
            rec['entry_raw_call_max_abs_diff'] = float(np.abs(dev.to_host(T3._arena) - ref).max())
            sync = {'entry': [], 'lincomb': []}
            events = {'entry': [], 'lincomb': []}
            for _ in range(2):                      # alternating, two rounds
                for name, fn in (('entry', entry), ('lincomb', lincomb)):
                    sync[name].append(median_ms(fn, args.reps, args.warm)[0])
                    events[name].append(event_ms(fn, args.batch, max(3, args.reps // 3)))
            for name, kernel in (('entry', 'tpa_mpo_entry_apply_batch'), ('lincomb', 'tpa_lincomb_batch')):
                ev = min(events[name])
                rec['mpo_step_' + name] = dict(kernel=kernel, ms_call_and_sync=sync[name], ms_per_launch_by_events=events[name],
                                               GBps_by_events=a01.bytes / ev / 1e6)
            rec['entry_kernel_beats_lincomb_by_events'] = bool(min(events['entry']) < min(events['lincomb']))
            rec['entry_over_lincomb_by_events'] = min(events['entry']) / min(events['lincomb'])
            print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
