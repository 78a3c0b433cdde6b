"""Times one interior step of the zip-up MPO application (``M [(vL.p), (wR.vR)]`` from ``VH_prev``, ``B`` and ``W``) on a chi = 1024-shaped
Sz-conserving spin-1/2 site with seeded synthetic tensors, for three MPO tensors:

  nn     the 4-wide structure of ``U_II`` of a nearest-neighbour chain: bond charges (0, +2, -2, 0), every entry the charge rule
         allows, complex;
  dense  a dense complex W of bond dimension 24 with sorted and bunched bond legs (charge sectors 12, 6 and 6 wide);
  wide   the same with bond dimension 48 (sectors 24, 12 and 12 wide: cells of 24 rows, the 32-accumulator kernel).

and three routes:

  entry    ``T1 = VH_prev . B`` and the entry-by-entry launch ``tpa_mpo_expand_batch``           (TPA_MPO_CELL=0)
  cell     ``T1`` and the cell-dense launch ``tpa_mpo_cell_apply_batch``                        (TPA_MPO_CELL=2)
  rule     ``T1`` and the launches ``MpoZipupPlan._cell_rule`` selects                           (TPA_MPO_CELL=1)
  generic  the reference's statements in its order: tensordot(B, W), tensordot(VH, .), combine_legs -- where the intermediate of
           chi^2 D^2 d elements fits in ``--generic-gb``

Per route the whole step and the MPO step alone (the launches on a prepared ``T1``); for the launches the bytes their tables account
for and the bandwidth that corresponds to.  Then one full ``MPO.apply`` (zip-up pass and ``compress_svd``) of the stand-alone driver on
an L = 32 XXZ chain with the ``U_II`` tensors of tests/golden/mpo_apply.pkl (bulk tensor repeated), after warm-up applications from the
Neel state, under TPA_MPO_CELL = 0 and 2.  Protocol: warm-up calls, then timed calls between device events on the stream; median,
minimum and maximum.

    python scripts/zipup_bench.py [--chi 1024] [--reps 10] [--warmup 3] [--no-apply] [--real]
"""
import argparse
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mixer_bench import sector_sizes, timed  # noqa: E402


def make_site(chi, bond_q, rng, real=False):
    """``VH_prev [vL, wR, vR]``, ``B [vL, p, vR]``, ``W [wL, wR, p, p*]`` (complex, or real) with the bond charges ``bond_q`` (2 Sz) on both MPO legs."""
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
    chinfo = ChargeInfo([1])
    p = LegCharge.from_qflat(chinfo, [[1], [-1]], qconj=+1)
    sizes = sector_sizes(chi)
    n = len(sizes)
    leg = LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(sizes)]), [[2 * (i - n // 2)] for i in range(n)], qconj=+1)
    leg1 = LegCharge.from_qind(chinfo, leg.slices, leg.charges + 1, qconj=+1)
    wL = LegCharge.from_qflat(chinfo, [[q] for q in bond_q], qconj=+1)
    dt = np.float64 if real else np.complex128
    rnd = lambda shape: rng.standard_normal(shape) + (0. if real else 1j * rng.standard_normal(shape))      # noqa: E731
    W = npc.Array.from_func(rnd, [wL, wL.conj(), p, p.conj()], dtype=dt, labels=['wL', 'wR', 'p', 'p*'])
    _, W = W.sort_legcharge(sort=[True, True, False, False], bunch=[True, True, False, False])
    VH = npc.Array.from_func(rnd, [leg, W.get_leg('wL').conj(), leg.conj()], dtype=dt, labels=['vL', 'wR', 'vR'])
    B = npc.Array.from_func(rnd, [leg, p, leg1.conj()], dtype=dt, labels=['vL', 'p', 'vR'])
    return VH, B, W


def step_bench(name, bond_q, args, rng):
    import torch
    from tenpy_amd.algorithms import mps_common
    from tenpy_amd.linalg import np_conserved as npc
    VH, B, W = make_site(args.chi, bond_q, rng, args.real)
    item = 8 if args.real else 16
    D = W.get_leg('wL').ind_len
    print("== %s: chi = %d, sectors %s, d = 2, D = %d, blocks of the MPO bond leg %s, %d stored blocks of W" % (
        name, args.chi, sector_sizes(args.chi).tolist(), D, W.get_leg('wR').get_block_sizes().tolist(), W.stored_blocks))
    T1 = npc.tensordot(VH, B, axes=['vR', 'vL'])
    plan = mps_common.MpoZipupPlan.get(T1, W)
    assert plan.ordered
    cj = plan.cell_jobs_host
    fill = plan.cell_nnz.sum() / max(1, (plan.jobs_host[:, 2] * plan.cell_n_src).sum())
    print("plan: %d cells (%d cell-dense jobs), rows per cell max %d, sources per cell max %d, fill %.2f; the rule takes %d cells; "
          "entry tables %.1f MB, cell tables %.1f MB, M %.1f MB, T1 %.1f MB"
          % (len(plan.jobs_host), len(cj), plan.jobs_host[:, 2].max(), plan.cell_n_src.max(), fill,
             int(plan._cell_rule(plan.cell_n_src, plan.jobs_host[:, 2], plan.cell_nnz).sum()), plan.bytes / 1e6, plan.cell_bytes / 1e6,
             plan.total * item / 1e6, T1._arena.numel() * item / 1e6))
    got = {m: plan.apply(T1, mode=m).to_ndarray() for m in (0, 2)}
    print("entry route == cell route: %s" % np.array_equal(got[0], got[2]))
    del got
    res = {}
    for label, mode in (('entry', 0), ('cell', 2), ('rule', 1)):
        os.environ['TPA_MPO_CELL'] = str(mode)
        whole = timed(lambda: mps_common.device_zipup_step(VH, B, W), args.reps, args.warmup)
        alone = timed(lambda: plan.apply(T1, mode=mode), args.reps, args.warmup)
        nbytes = plan.bytes if mode == 0 else plan.cell_bytes
        res[label] = (whole, alone)
        print("(%s) whole step: median %.3f ms, min %.3f, max %.3f; MPO step alone: median %.3f ms, min %.3f, max %.3f%s  (%d timed calls after %d warm-up calls)"
              % (label, *whole, *alone, "" if mode == 1 else "; %.1f MB by its tables -> %.0f GB/s at the median" % (nbytes / 1e6, nbytes / alone[0] / 1e6),
                 args.reps, args.warmup))
    os.environ.pop('TPA_MPO_CELL', None)
    med = timed(lambda: npc.tensordot(VH, B, axes=['vR', 'vL']), args.reps, args.warmup)
    print("T1 = VH_prev . B alone: median %.3f ms, min %.3f, max %.3f" % med)
    inter = B._arena.numel() * item * W._arena.numel() / 4        # |B| x (entries of W per physical pair): upper estimate of tensordot(B, W)
    if inter <= args.generic_gb * 1e9:
        def generic():
            X = npc.tensordot(B, W, axes=('p', 'p*'))
            X = npc.tensordot(VH, X, axes=(['wR', 'vR'], ['wL', 'vL']))
            return X.combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1])
        g = timed(generic, args.reps, args.warmup)
        print("(generic) whole step: median %.3f ms, min %.3f, max %.3f; intermediate tensordot(B, W) about %.2f GB" % (*g, inter / 1e9))
    else:
        print("(generic) not run: the intermediate tensordot(B, W) is estimated at %.1f GB (limit %.1f GB)" % (inter / 1e9, args.generic_gb))
    torch.cuda.synchronize()
    npc.clear_device_caches()
    return res


def apply_bench(args):
    import torch
    from tenpy_amd.linalg import np_conserved as npc
    from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
    from tenpy_amd.networks.mpo import MPO
    from tenpy_amd.networks.mps import MPS
    with open(os.path.join(ROOT, 'tests', 'golden', 'mpo_apply.pkl'), 'rb') as f:
        rec = pickle.load(f)['untruncated']['mpo']
    chinfo = ChargeInfo([int(m) for m in rec['chinfo_mod']])

    def array(r):
        legs = [LegCharge.from_qind(chinfo, sl, np.asarray(q).reshape(len(q), -1)[sl[:-1]], qconj=qc) for (q, qc), sl in zip(r['legs'], r['slices'])]
        return npc.Array.from_ndarray(r['data'].astype(np.complex128), legs, dtype=np.complex128, qtotal=r['qtotal'], labels=r['labels'], cutoff=0.)
    L = 32
    Ws = [array(rec['W'][0])] + [array(rec['W'][3]) for _ in range(L - 2)] + [array(rec['W'][-1])]
    p = LegCharge.from_qflat(chinfo, rec['p_leg'][0], qconj=rec['p_leg'][1])
    U = MPO([p] * L, Ws, IdL=rec['IdL'][0], IdR=rec['IdR'][-1])
    opts = dict(compression_method='zip_up', trunc_params=dict(chi_max=args.apply_chi, svd_min=1.e-10), m_temp=2)
    for mode in ('0', '2'):
        os.environ['TPA_MPO_CELL'] = mode
        psi = MPS.from_product_state([p] * L, [0, 1] * (L // 2))
        for _ in range(args.apply_warm):
            U.apply(psi, dict(opts))
        med = timed(lambda: U.apply(psi, dict(opts)), args.reps, 0)
        torch.cuda.synchronize()
        print("full MPO.apply, XXZ L = %d, U_II (dt = 0.1), chi_max = %d, after %d applications, TPA_MPO_CELL=%s: median %.1f ms, min %.1f, max %.1f "
              "(%d timed applications; max chi %d)" % (L, args.apply_chi, args.apply_warm, mode, *med, args.reps, max(psi.chi)))
    os.environ.pop('TPA_MPO_CELL', None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chi', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--generic-gb', type=float, default=6.)
    ap.add_argument('--apply-chi', type=int, default=64)
    ap.add_argument('--apply-warm', type=int, default=12)
    ap.add_argument('--no-apply', action='store_true')
    ap.add_argument('--real', action='store_true', help="real tensors in the step legs (the f64 kernels)")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {'nn': step_bench('nn', [0, 2, -2, 0], args, rng),
           'dense': step_bench('dense', [0, 2, -2, 0] * 6, args, rng),
           'wide': step_bench('wide', [0, 2, -2, 0] * 12, args, rng)}
    for name, r in res.items():
        e, c = r['entry'][1], r['cell'][1]
        print("%s: MPO step alone, cell against entry: %.3f ms against %.3f ms (spreads %.3f-%.3f and %.3f-%.3f) -> the cell route is %s"
              % (name, c[0], e[0], c[1], c[2], e[1], e[2], "not slower" if c[0] <= e[0] else "SLOWER"))
        u = r['rule'][1]
        print("%s: MPO step alone, rule against entry: %.3f ms against %.3f ms (spreads %.3f-%.3f and %.3f-%.3f)"
              % (name, u[0], e[0], u[1], u[2], e[1], e[2]))
    if not args.no_apply:
        apply_bench(args)


if __name__ == '__main__':
    main()
