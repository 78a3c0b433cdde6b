"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_mpo_entry_apply_batch`` (the MPO step of the factored effective Hamiltonians entry
by entry: MPO bond legs with wide blocks, wide physical sectors) and of ``tpa_lanczos_run`` / ``tpa_lanczos_run_ex`` with op kind 6, on
top of ``mock_mpo_apply`` (and through it ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h``; set as attributes of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
these attributes).  ``calls`` counts the calls of the entry point."""
import numpy as np

import mock_mpo_apply
from mock_device import REG, _host, _npdt
from tenpy_amd import _lib

calls = {'tpa_mpo_entry_apply_batch': 0}


def tpa_mpo_entry_apply_batch(code, jobs_p, n_jobs, rows_p, terms_p, max_cols, src_p, dst_p, stream):
    calls['tpa_mpo_entry_apply_batch'] += 1
    if code not in (0, 1):
        return _lib.E_BADARG
    if n_jobs <= 0 or n_jobs > 65535:      # one job per blockIdx.y: the grid limit is an argument error
        return 0 if n_jobs <= 0 else _lib.E_BADARG
    dt = _npdt(code)
    jobs = REG.view(jobs_p, np.int64)[:8 * n_jobs].reshape(n_jobs, 8)
    live = jobs[(jobs[:, 1] > 0) & (jobs[:, 2] > 0) & (jobs[:, 3] > 0)]
    if len(live) == 0:
        return 0
    n_rows = int(np.max(live[:, 4] + live[:, 2]))
    rows = REG.view(rows_p, np.int64)[:2 * n_rows].reshape(n_rows, 2)
    terms = REG.view(terms_p, np.int64) if terms_p else np.zeros(0, np.int64)
    src, dst = REG.view(src_p, dt), REG.view(dst_p, dt)
    for dst_off, pre, nr, post, r0, dst_ld, _, _ in live.tolist():
        assert pre * post <= max_cols, "max_job_cols too small"
        dst_ld = dst_ld or nr * post
        ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
        for o in range(nr):
            t0, nt = rows[r0 + o].tolist()
            acc = np.zeros((pre, post), dtype=dt)
            for src_off, src_ld, a_re, a_im in terms[4 * t0:4 * (t0 + nt)].reshape(nt, 4).tolist():      # terms in table order
                alpha = complex(*np.array([a_re, a_im], dtype=np.int64).view(np.float64))
                acc = acc + (alpha if code == 1 else alpha.real) * src[src_off + ii * src_ld + jj]
            dst[dst_off + ii * dst_ld + o * post + jj] = acc
    return 0


def install(monkeypatch):
    """``mock_mpo_apply.install`` plus the emulations of this file; returns the ``MockLib`` instance."""
    mock = mock_mpo_apply.install(monkeypatch)
    run_ex_below = mock.tpa_lanczos_run_ex

    def tpa_lanczos_run_ex(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                           scal_p, scr_p, cb, user, time_gemms, info_p, flags, pw_p, stream):
        """The loop of ``mock_mpo_apply``'s emulation with op kind 6 as the header states it, for programs that hold one; programs
        without kind 6 run the emulation below unchanged."""
        ops = _host(ops_p, (n_ops, 12))
        if not np.any(ops[:, 0] == 6):
            return run_ex_below(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                                scal_p, scr_p, cb, user, time_gemms, info_p, flags, pw_p, stream)
        if flags & ~1 or (flags & 1 and (not pw_p or N_max > _lib.PROJECT_MAX)):
            return _lib.E_BADARG
        dt = _npdt(code)
        isz = np.dtype(dt).itemsize
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
                a, c = slot(op[6], vin, w), slot(op[8], vin, w)
                rc = 0
                if op[0] == 0:
                    rc = mock.tpa_gemm_chain(code, int(op[1]), int(op[2]), int(op[3]), int(op[4]), int(op[5]), a, slot(op[7], vin, w), c, stream)
                elif op[0] == 1:
                    rc = mock.tpa_lincomb_batch(code, int(op[2]), int(op[5]), int(op[3]), int(op[9]), a, c, stream)
                elif op[0] == 2:
                    rc = mock.tpa_copy_batch(code, int(op[2]), int(op[5]), int(op[9]), a, c, stream)
                elif op[0] == 4:
                    p0, cnt = int(op[2]), int(op[5])
                    rc = mock.tpa_project_out(code, n, a, cnt, int(op[3]), slot(op[7], vin, w), c, p0, None, p0 + 8 * (2 * cnt + 2), stream)
                elif op[0] == 5:            # (op[7] holds max_d, not a slot)
                    rc = mock.tpa_mpo_apply_batch(code, int(op[2]), int(op[5]), int(op[3]), int(op[4]), int(op[7]), int(op[9]), a, c, stream)
                elif op[0] == 6:            # (p1 = rows, p2 = terms)
                    rc = mock.tpa_mpo_entry_apply_batch(code, int(op[2]), int(op[5]), int(op[3]), int(op[4]), int(op[9]), a, c, stream)
                else:
                    return _lib.E_BADARG        # (collectives: out of scope of the entry-MPO programs)
                if rc:
                    return rc
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

    run_below = mock.tpa_lanczos_run

    def tpa_lanczos_run(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                        scal_p, scr_p, cb, user, time_gemms, info_p, stream):
        """``tpa_lanczos_run`` is ``tpa_lanczos_run_ex`` with flags = 0 (header); programs without kind 6 run the emulation below."""
        if not np.any(_host(ops_p, (n_ops, 12))[:, 0] == 6):
            return run_below(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                             scal_p, scr_p, cb, user, time_gemms, info_p, stream)
        return tpa_lanczos_run_ex(code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                                  scal_p, scr_p, cb, user, time_gemms, info_p, 0, None, stream)

    mock.tpa_mpo_entry_apply_batch = tpa_mpo_entry_apply_batch
    mock.tpa_lanczos_run_ex = tpa_lanczos_run_ex
    mock.tpa_lanczos_run = tpa_lanczos_run
    return mock
