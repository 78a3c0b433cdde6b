"""Time of one Krylov time-evolution ``LanczosEvolution(H, theta, opts).run(delta)`` on the device, N fixed by N_min = N_max.

Synthetic Sz block structures (``gemm_bench.sectors``, as ``lanczos_bench.py``) with seeded complex environments and vectors:
the two-site operator always; the one- and zero-site operators where the classes exist, so that the script runs unchanged on
commits before they did.  Per leg: median over ``reps`` evolutions after warm-up of (a) the time between two HIP events around
the call, (b) the wall clock around the call plus a device synchronise.  With ``tpa_krylov_combine_z`` in the library, also the
combination pass alone: achieved bytes/s = 16 n (N + 1) over its HIP-event time, against the 6.29 TB/s copy rate of the MI355X.

    python scripts/evolve_bench.py [--chi 512 2048] [--reps 20] [--N 10] [--label NAME]

One JSON line per (chi, leg).  The random environments are not Hermitian: the numbers of the evolution mean nothing, only its
cost does (the Krylov loop and the combination do the same work for any tridiagonal matrix)."""
import argparse
import json
import logging
import os
import subprocess
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
from tenpy_amd.models.spin_chains import xxz_chain_mpo
from gemm_bench import sectors

HBM_COPY_RATE = 6.29e12       # bytes/s, measured copy rate (MI355X micro-architecture notes)


def commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=root, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


def operators(chi, seed=0):
    H = xxz_chain_mpo(8, 1., 1., 0.)
    W0, W1 = H.get_W(3), H.get_W(4)
    q, n = sectors(chi)
    bond = LegCharge.from_qind(W0.chinfo, np.concatenate([[0], np.cumsum(n)]), q.reshape(-1, 1), qconj=+1)
    rng = np.random.default_rng(seed)

    def rnd(sh):
        return (rng.standard_normal(sh) + 1j * rng.standard_normal(sh)) / np.sqrt(chi)
    cplx = dict(dtype=np.complex128)
    LP = npc.Array.from_func(rnd, [bond, W0.get_leg('wL').conj(), bond.conj()], labels=['vR*', 'wR', 'vR'], **cplx)
    RP2 = npc.Array.from_func(rnd, [bond, W1.get_leg('wR').conj(), bond.conj()], labels=['vL', 'wL', 'vL*'], **cplx)
    RP1 = npc.Array.from_func(rnd, [bond, W0.get_leg('wR').conj(), bond.conj()], labels=['vL', 'wL', 'vL*'], **cplx)
    RP0 = npc.Array.from_func(rnd, [bond, W0.get_leg('wL'), bond.conj()], labels=['vL', 'wL', 'vL*'], **cplx)
    p = W0.get_leg('p')
    W0c, W1c = W0.astype(np.complex128), W1.astype(np.complex128)

    def vec(legs, labels, qtotal=None):
        t = npc.Array.from_func(rnd, legs, labels=labels, qtotal=qtotal, **cplx)
        return t * (1. / npc.norm(t))
    out = {}
    two = mps_common.TwoSiteH(None, 3, tensors=(LP, RP2, W0c, W1c))
    out['two'] = (two, two.combine_theta(vec([bond, p, p, bond.conj()], ['vL', 'p0', 'p1', 'vR'])))
    if hasattr(mps_common, 'OneSiteH'):
        out['one'] = (mps_common.OneSiteH.from_LP_W0_RP(LP, W0c, RP1), vec([bond, p, bond.conj()], ['vL', 'p0', 'vR'], qtotal=[1]))      # (one spin between two odd-2Sz bonds)
        out['zero'] = (mps_common.ZeroSiteH.from_LP_RP(LP, RP0), vec([bond, bond.conj()], ['vL', 'vR']))
    return out


def time_evolve(H, theta, opts, delta, reps, warmup=3):
    for _ in range(warmup):
        kb.LanczosEvolution(H, theta, dict(opts)).run(delta)
    torch.cuda.synchronize()
    ev_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        psi, N = kb.LanczosEvolution(H, theta, dict(opts)).run(delta)
        e1.record()
        torch.cuda.synchronize()
        wall_ms.append(1e3 * (time.perf_counter() - t0))
        ev_ms.append(e0.elapsed_time(e1))
    return float(np.median(ev_ms)), float(np.median(wall_ms)), float(np.min(wall_ms)), float(np.max(wall_ms)), N


def time_combine(n, N, reps):
    """``tpa_krylov_combine_z`` alone on a complex basis of N vectors of n elements."""
    L = dev.lib()
    rng = np.random.default_rng(1)
    V = torch.from_numpy(rng.standard_normal(2 * n * N)).cuda().view(torch.complex128)
    out = dev.empty(n, np.complex128)
    red, scr = dev.reduction_buffers()
    c = np.ascontiguousarray(rng.standard_normal((N, 2)))
    nrm = np.zeros(1)

    def call():
        dev.check(L.tpa_krylov_combine_z(1, n, V.data_ptr(), N, c.ctypes.data, 1., out.data_ptr(), red.data_ptr(), scr.data_ptr(),
                                         nrm.ctypes.data, dev.stream()), "krylov_combine_z")
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = float(np.median(ms)) * 1e-3
    nbytes = 16 * n * (N + 1)
    return dict(n=n, N=N, ms=t * 1e3, bytes=nbytes, bytes_per_s=nbytes / t, fraction_of_copy_rate=nbytes / t / HBM_COPY_RATE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chi', type=int, nargs='+', default=[512, 2048])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--N', type=int, default=10)
    ap.add_argument('--label', default='')
    a = ap.parse_args()
    _lib.require_gpu()
    logging.disable(logging.WARNING)
    opts = {'N_min': a.N, 'N_max': a.N}
    head = dict(label=a.label, commit=commit(), date=time.strftime('%Y-%m-%d'), N=a.N, reps=a.reps)
    for chi in a.chi:
        for leg, (H, theta) in operators(chi).items():
            before = kb.stats.get('n_native_evolve', 0)
            ev, wall, lo, hi, N = time_evolve(H, theta, opts, -0.025j, a.reps)
            native = kb.stats.get('n_native_evolve', 0) - before
            print(json.dumps(dict(head, bench='evolve', chi=chi, leg=leg, n=int(theta._arena.numel()), N_run=N, event_ms=ev, wall_ms=wall,
                                  wall_min_ms=lo, wall_max_ms=hi, native_route=bool(native))), flush=True)
        if hasattr(_lib.load(), 'tpa_krylov_combine_z') and 'tpa_krylov_combine_z' in _lib.exported_symbols():
            n = int(operators(chi)['two'][1]._arena.numel())
            print(json.dumps(dict(head, bench='combine_z', chi=chi, **time_combine(n, a.N, a.reps))), flush=True)


if __name__ == '__main__':
    main()
