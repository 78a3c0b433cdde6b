"""TEST INFRASTRUCTURE ONLY: numpy emulation of the device entry points that came with the projected Lanczos runs
(``tpa_project_out``, ``tpa_lanczos_run_ex``), on top of ``mock_evolve`` (and through it ``mock_device``).

Written from the contract in ``include/tenpy_amd.h`` (argument errors, edge cases, what is written where), like the two modules below
it; set as attributes of the ``MockLib`` instance, because names that instance does not have are forwarded to the real shared
library, which would be handed host pointers.  ``calls`` counts the calls of the two entry points (the "unchanged path" tests)."""
import numpy as np

import mock_evolve
from mock_device import REG, _host, _npdt
from tenpy_amd import _lib

calls = {'tpa_project_out': 0, 'tpa_lanczos_run_ex': 0}


def tpa_project_out(code, n, basis_p, m, stride, src_p, dst_p, coeff_p, nrm2_p, work_p, stream):
    calls['tpa_project_out'] += 1
    if code not in (0, 1) or m < 0 or m > _lib.PROJECT_MAX:
        return _lib.E_BADARG
    if m > 0 and (not coeff_p or (n > 0 and (not basis_p or stride < n))):
        return _lib.E_BADARG
    if n > 0 and not (src_p and dst_p and work_p):
        return _lib.E_BADARG
    coeff = REG.view(coeff_p, np.float64) if m > 0 else None
    nrm2 = REG.view(nrm2_p, np.float64) if nrm2_p else None
    if n <= 0:
        if m > 0:
            coeff[:2 * m] = 0.
        if nrm2 is not None:
            nrm2[:2] = 0.
        return 0
    dt = _npdt(code)
    isz = np.dtype(dt).itemsize
    if m > 0 and not (dst_p + n * isz <= basis_p or basis_p + ((m - 1) * stride + n) * isz <= dst_p):
        return _lib.E_BADARG
    src = REG.view(src_p, dt)[:n].copy()
    acc = src.copy()
    if m > 0:
        B = REG.view(basis_p, dt)
        for j in range(m):
            b = B[j * stride:j * stride + n]
            c = np.vdot(b, src)
            coeff[2 * j], coeff[2 * j + 1] = np.real(c), np.imag(c)
            acc -= c * b
    REG.view(dst_p, dt)[:n] = acc
    if nrm2 is not None:
        nrm2[0], nrm2[1] = float(np.real(np.vdot(acc, acc))), 0.
    return 0


def install(monkeypatch):
    """``mock_evolve.install`` plus the emulations of this file; returns the ``MockLib`` instance."""
    mock = mock_evolve.install(monkeypatch)

    def tpa_lanczos_run_ex(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                           scal_p, scr_p, cb, user, time_gemms, info_p, flags, pw_p, stream):
        """The loop of ``MockLib.tpa_lanczos_run`` with op kind 4 and flag bit 0 as the header states them."""
        calls['tpa_lanczos_run_ex'] += 1
        if flags & ~1 or (flags & 1 and (not pw_p or N_max > _lib.PROJECT_MAX)):
            return _lib.E_BADARG
        dt = _npdt(code)
        isz = np.dtype(dt).itemsize
        ops = _host(ops_p, (n_ops, 12))
        bufs = _host(bufs_p, (n_bufs,)) if n_bufs else np.zeros(0, np.int64)
        info = _host(info_p, (4,), np.float64)
        psi0 = REG.view(psi0_p, dt)[:n]
        V = lambda k: krylov_p + k * n * isz
        beta0 = float(np.sqrt(np.real(np.vdot(psi0, psi0))))
        info[3] = beta0
        if not beta0 >= cutoff:
            info[0], info[1], info[2] = 0., 1., 0.
            return 0
        REG.view(V(0), dt)[:n] = psi0 / beta0
        hist = {}

        def slot(s, vin, w):
            return vin if s == -1 else (w if s == -2 else int(bufs[s]))
        N, n_mv, stopped = 0, 0, False
        for k in range(N_max):
            vin, w = V(k), V(k + 1)
            for op in ops:
                a, b, c = slot(op[6], vin, w), slot(op[7], vin, w), slot(op[8], vin, w)
                if op[0] == 0:
                    mock.tpa_gemm_chain(code, int(op[1]), int(op[2]), int(op[3]), int(op[4]), int(op[5]), a, b, c, stream)
                elif op[0] == 1:
                    mock.tpa_lincomb_batch(code, int(op[2]), int(op[5]), int(op[3]), int(op[9]), a, c, stream)
                elif op[0] == 2:
                    mock.tpa_copy_batch(code, int(op[2]), int(op[5]), int(op[9]), a, c, stream)
                elif op[0] == 4:
                    p0, cnt = int(op[2]), int(op[5])
                    rc = mock.tpa_project_out(code, n, a, cnt, int(op[3]), b, c, p0, None, p0 + 8 * (2 * cnt + 2), stream)
                    if rc:
                        return rc
                else:
                    return _lib.E_BADARG        # (collectives: out of scope of the projected runs)
            n_mv += 1
            if has_shift:
                mock.tpa_axpy(code, n, E_shift, 0., vin, w, stream)
            ab_p = scal_p + 8 * 2 * k
            if flags & 1 and k > 0:
                wv, vk = REG.view(w, dt)[:n], REG.view(vin, dt)[:n]
                ab = REG.view(ab_p, np.float64)
                alpha = float(np.real(np.vdot(wv, vk)))
                wv -= alpha * vk
                ab[0] = alpha
                rc = mock.tpa_project_out(code, n, krylov_p, k, n, w, w, pw_p, ab_p + 8, pw_p + 8 * (2 * _lib.PROJECT_MAX + 2), stream)
                if rc:
                    return rc
                if ab[1] > 0.:
                    wv *= 1. / np.sqrt(ab[1])
            else:
                mock.tpa_lanczos_step(code, n, w, vin, V(k - 1) if k > 0 else None, scal_p + 8 * (2 * (k - 1) + 1) if k > 0 else None,
                                      ab_p, scr_p, stream)
            ab = REG.view(ab_p, np.float64)
            hist[k] = (float(ab[0]), float(ab[1]))
            if k > 0 and cb(k - 1, hist[k - 1][0], hist[k - 1][1], user):
                N, stopped = k, True
                break
            N = k + 1
        if not stopped:
            cb(N_max - 1, hist[N_max - 1][0], hist[N_max - 1][1], user)
        info[0], info[1], info[2] = N, n_mv, 0.
        return 0

    mock.tpa_project_out = tpa_project_out
    mock.tpa_lanczos_run_ex = tpa_lanczos_run_ex
    return mock
