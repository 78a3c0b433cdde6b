"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_herk_chain`` (the weighted Hermitian rank-k update of the density-matrix mixer),
on top of ``mock_mpo_entry`` (and through it ``mock_mpo_apply``, ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h`` (K1h); set as an attribute of the ``MockLib`` instance, because names that instance
does not have are forwarded to the real shared library, which would be handed host pointers.  ``calls`` counts the calls of the
entry point.  ``DEFECT`` (None in every test but the mutation test of tests/test_conformance_herk.py) switches ONE deliberate
defect on: 'no_weight', 'no_conj', 'one_triangle', 'w_inner_ignored', 'mirror_rounded_again' (the mirror one ulp off: inside every
error bound, only the bit comparison sees it), 'diagonal_not_real' (a rounding-size imaginary part left on the diagonal)."""
import ctypes

import numpy as np

import mock_mpo_entry
from mock_device import REG, _npdt, _strided
from tenpy_amd import _lib

calls = {'tpa_herk_chain': 0}
DEFECT = None
DEFECTS = ('no_weight', 'no_conj', 'one_triangle', 'w_inner_ignored', 'mirror_rounded_again', 'diagonal_not_real')
LINK_W, TASK_W = 12, 10


def tpa_herk_chain(code, tasks_p, links_p, tiles_p, n_tiles, A_p, B_p, w_p, C_p, stream):
    calls['tpa_herk_chain'] += 1
    if code not in (0, 1):
        return _lib.E_BADARG
    if n_tiles <= 0:
        return 0
    dt = _npdt(code)
    tiles = REG.view(tiles_p, np.int32)[:4 * n_tiles].reshape(n_tiles, 4)
    tasks_all, links_all = REG.view(tasks_p, np.int64), REG.view(links_p, np.int64)
    A, B, C = REG.view(A_p, dt), REG.view(B_p, dt), REG.view(C_p, dt)
    W = REG.view(w_p, np.float64) if w_p else None
    bt = ctypes.c_int()
    _lib.load().tpa_herk_tile_shape(code, ctypes.byref(bt))
    bt = bt.value
    for t, tr, tc, _ in tiles.tolist():
        c_off, m, n, ldc, lb, lc, acc, herm, m_off, m_ld = tasks_all[TASK_W * t:TASK_W * (t + 1)].tolist()
        if herm and tr < tc:
            continue
        r0, r1 = tr * bt, min(m, (tr + 1) * bt)
        c0, c1 = tc * bt, min(n, (tc + 1) * bt)
        assert r0 < m and c0 < n, "tile outside of task"
        out = np.zeros((r1 - r0, c1 - c0), dtype=dt)
        for l in range(lb, lb + lc):
            a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off, w_len, w_inner, _, _ = links_all[LINK_W * l:LINK_W * (l + 1)].tolist()
            if k <= 0:
                continue
            Am = _strided(A, a_off + r0 * a_rs, (r1 - r0, k), (a_rs, a_ks))
            Bm = _strided(B, b_off + c0 * b_rs, (c1 - c0, k), (b_rs, b_ks))
            if w_off >= 0 and DEFECT != 'no_weight':
                inner = 1 if DEFECT == 'w_inner_ignored' else w_inner
                idx = w_off + (np.arange(k) // inner) % w_len
                assert idx.max() < len(W)
                Am = Am * W[idx][None, :]           # the weight goes into A first (one rounding), as in the kernel
            out += Am @ (Bm.T if DEFECT == 'no_conj' else Bm.conj().T)
        Cm = _strided(C, c_off + r0 * ldc + c0, out.shape, (ldc, 1), writeable=True)
        if acc:
            out = out + Cm
        if herm:
            keep = (r0 + np.arange(r1 - r0))[:, None] >= (c0 + np.arange(c1 - c0))[None, :]
            if tr == tc:
                d = np.arange(r1 - r0)
                out[d, d] = out[d, d].real + (1j * np.abs(out[d, d].real) * 2.0**-52 if DEFECT == 'diagonal_not_real' and code == 1 else 0)
            Cm[keep] = out[keep]
            if DEFECT != 'one_triangle':
                Mm = _strided(C, c_off + c0 * ldc + r0, (c1 - c0, r1 - r0), (ldc, 1), writeable=True)
                strict = (r0 + np.arange(r1 - r0))[:, None] > (c0 + np.arange(c1 - c0))[None, :]
                Mm[strict.T] = out.conj().T[strict.T]
                if DEFECT == 'mirror_rounded_again':
                    Mm[strict.T] = Mm[strict.T] * (1 + 2.0**-52)
        else:
            Cm[...] = out
            if m_off >= 0 and DEFECT != 'one_triangle':
                Mm = _strided(C, m_off + c0 * m_ld + r0, (c1 - c0, r1 - r0), (m_ld, 1), writeable=True)
                Mm[...] = out.conj().T
    return 0


def install(monkeypatch):
    """``mock_mpo_entry.install`` plus the emulation of this file; returns the ``MockLib`` instance."""
    mock = mock_mpo_entry.install(monkeypatch)
    mock.tpa_herk_chain = tpa_herk_chain
    return mock
