"""Cost of the fused projection ``tpa_project_out`` and of a projected native Lanczos run on the device.

(a) kernel: ``n`` real elements (default 3.5e6 = the chi = 2048 two-site wave function, 28 MB), m in {1, 4, 16, 63}, in place with
    the norm: achieved bytes/s by the traffic model of DESIGN section 3, ``8 n (2 m + ceil(m / 8) + 2)``, beside the sequence it
    replaces -- m x (``tpa_dot`` + ``tpa_axpy``), enqueued without host reads (a fixed alpha: only the cost matters), ``5 m 8 n``.
(b) one ``LanczosGroundState`` run on a TwoSiteH of the XXZ chi = 512 block structure (``gemm_bench.sectors``; seeded random
    symmetric-free environments: the numbers of the run mean nothing, only its cost does) wrapped in ``OrthogonalNpcLinearOperator``
    with one vector, N fixed by N_min = N_max: the native route against the step-by-step route of the same tree (``kb.NATIVE`` off),
    which is what every commit before this one runs for such an input.

Convention of ``gemm_bench.py`` / ``evolve_bench.py``: at least 40 timed repetitions after at least 10 ms of the same load, HIP events
around each call, medians.

    python scripts/project_bench.py [--n 3500000] [--m 1 4 16 63] [--chi 512] [--N 12] [--reps 40]

One JSON line per measurement (kept in profiles/excited_states.txt)."""
import argparse
import json
import logging
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch
from tenpy_amd import _lib
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import LegCharge
from tenpy_amd.linalg.sparse import OrthogonalNpcLinearOperator
from tenpy_amd.models.spin_chains import xxz_chain_mpo
from gemm_bench import sectors

J = 8


def timed(call, reps):
    """Median HIP-event milliseconds of ``call`` over ``reps`` repetitions, after >= 10 ms (and >= 3 calls) of the same load."""
    t0 = time.perf_counter()
    k = 0
    while k < 3 or time.perf_counter() - t0 < 0.010:
        call()
        torch.cuda.synchronize()
        k += 1
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def kernel(n, m, reps):
    L, st = dev.lib(), dev.stream()
    gen = torch.Generator(device='cuda').manual_seed(m)
    basis = torch.randn(m * n, dtype=torch.float64, device='cuda', generator=gen) * (1. / np.sqrt(n))
    w = torch.randn(n, dtype=torch.float64, device='cuda', generator=gen)
    coeff = dev.empty(2 * m + 2, np.float64)
    work = dev.empty(_lib.PROJECT_WORK, np.float64)
    red, scr = dev.reduction_buffers()

    def fused():
        dev.check(L.tpa_project_out(0, n, basis.data_ptr(), m, n, w.data_ptr(), w.data_ptr(), coeff.data_ptr(),
                                    coeff.data_ptr() + 16 * m, work.data_ptr(), st), "project_out")

    def sequence():
        for j in range(m):
            b = basis.data_ptr() + 8 * j * n
            dev.check(L.tpa_dot(0, n, b, w.data_ptr(), 1, red.data_ptr(), scr.data_ptr(), st), "dot")
            dev.check(L.tpa_axpy(0, n, -1e-3, 0., b, w.data_ptr(), st), "axpy")
    f_ms, f_lo, f_hi = timed(fused, reps)
    s_ms, s_lo, s_hi = timed(sequence, reps)
    f_bytes, s_bytes = 8 * n * (2 * m + -(-m // J) + 2), 5 * m * 8 * n
    return dict(bench='project_out', n=n, m=m, fused_ms=f_ms, fused_min_ms=f_lo, fused_max_ms=f_hi, fused_model_bytes=f_bytes,
                fused_bytes_per_s=f_bytes / (f_ms * 1e-3),
                sequence_ms=s_ms, sequence_min_ms=s_lo, sequence_max_ms=s_hi, sequence_model_bytes=s_bytes,
                sequence_bytes_per_s=s_bytes / (s_ms * 1e-3), speedup=s_ms / f_ms)


def operator(chi, seed=0):
    H = xxz_chain_mpo(8, 1., 1., 0.)
    W0, W1 = H.get_W(3), H.get_W(4)
    q, n = sectors(chi)
    bond = LegCharge.from_qind(W0.chinfo, np.concatenate([[0], np.cumsum(n)]), q.reshape(-1, 1), qconj=+1)
    rng = np.random.default_rng(seed)

    def rnd(sh):
        return rng.standard_normal(sh) / np.sqrt(chi)
    LP = npc.Array.from_func(rnd, [bond, W0.get_leg('wL').conj(), bond.conj()], labels=['vR*', 'wR', 'vR'])
    RP = npc.Array.from_func(rnd, [bond, W1.get_leg('wR').conj(), bond.conj()], labels=['vL', 'wL', 'vL*'])
    p = W0.get_leg('p')
    two = mps_common.TwoSiteH(None, 3, tensors=(LP, RP, W0, W1))

    def vec():
        t = npc.Array.from_func(rnd, [bond, p, p, bond.conj()], labels=['vL', 'p0', 'p1', 'vR'])
        return two.combine_theta(t * (1. / npc.norm(t)))
    return two, vec(), vec()


def lanczos(chi, N, reps):
    H, theta, other = operator(chi)
    opts = {'N_min': N, 'N_max': N}
    out = dict(bench='lanczos_orthogonal', chi=chi, n=int(theta._arena.numel()), N=N, m=1)
    for native in (True, False):
        kb.NATIVE = native
        Ho = OrthogonalNpcLinearOperator(H, [other.copy(deep=True)])
        before = kb.stats['n_native_ortho']
        state = {}

        def run():
            state['N'] = kb.LanczosGroundState(Ho, theta, dict(opts)).run()[2]
        ms, lo, hi = timed(run, reps)
        key = 'native' if native else 'stepwise'
        out.update({key + '_ms': ms, key + '_min_ms': lo, key + '_max_ms': hi, key + '_N_run': state['N'],
                    key + '_took_native_route': kb.stats['n_native_ortho'] > before})
    kb.NATIVE = True
    out['speedup'] = out['stepwise_ms'] / out['native_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=3500000)
    ap.add_argument('--m', type=int, nargs='+', default=[1, 4, 16, 63])
    ap.add_argument('--chi', type=int, nargs='*', default=[512])
    ap.add_argument('--N', type=int, default=12)
    ap.add_argument('--reps', type=int, default=40)
    a = ap.parse_args()
    _lib.require_gpu()
    logging.disable(logging.WARNING)
    head = dict(date=time.strftime('%Y-%m-%d'), reps=a.reps)
    for m in a.m:
        print(json.dumps(dict(head, **kernel(a.n, m, a.reps))), flush=True)
    for chi in a.chi:
        print(json.dumps(dict(head, **lanczos(chi, a.N, a.reps))), flush=True)


if __name__ == '__main__':
    main()
