"""TEST INFRASTRUCTURE ONLY: ``MockLib`` (tests/mock_device.py) with numpy emulations of the entry points that came after it --
``tpa_gemm_chain_ex``, ``tpa_unit_defect_batch`` and op kind 7 of ``tpa_lanczos_run`` -- following the contract of
``include/tenpy_amd.h``.  ``install(monkeypatch)`` installs the plain emulation and then puts this one in its place, so the planner
of ``TwoSiteH._skip_program`` runs in ``-m "not gpu"`` tests."""
import numpy as np

from tenpy_amd.linalg import _device as dev

import mock_device
from mock_device import REG, MockLib, _host, _npdt, _strided

LINK_A2, LINK_UNIT = 4, 8


class MockLibEx(MockLib):
    n_ex_launches = 0
    last_ex_tiles = 0

    def tpa_gemm_chain_ex(self, code, cfg, tasks_p, links_p, tiles_p, n_tiles, A_p, A2_p, B_p, C_p, alphas_p, stream):
        assert code == 0, "extended links: real data only"
        import ctypes
        dt = _npdt(code)
        type(self).n_ex_launches += 1
        type(self).last_ex_tiles = n_tiles
        tiles = REG.view(tiles_p, np.int32)[:4 * n_tiles].reshape(n_tiles, 4)
        tasks_all, links_all = REG.view(tasks_p, np.int64), REG.view(links_p, np.int64)
        A, A2, B, C = REG.view(A_p, dt), REG.view(A2_p, dt), REG.view(B_p, dt), REG.view(C_p, dt)
        alphas = REG.view(alphas_p, np.float64)
        bm, bn = ctypes.c_int(), ctypes.c_int()
        self.real.tpa_gemm_tile_shape(code, cfg, ctypes.byref(bm), ctypes.byref(bn))
        bm, bn = bm.value, bn.value
        for t, tr, tc, _ in tiles:
            c_off, m, n, ldc, lb, lc, acc, _ = tasks_all[8 * t:8 * t + 8]
            r0, r1 = tr * bm, min(m, (tr + 1) * bm)
            c0, c1 = tc * bn, min(n, (tc + 1) * bn)
            assert r0 < m and c0 < n, "tile outside of task"
            out = np.zeros((r1 - r0, c1 - c0), dtype=dt)
            units = np.zeros_like(out)
            for l in range(lb, lb + lc):
                a_off, b_off, k, a_rs, a_ks, b_ks, b_ns, flags = links_all[8 * l:8 * l + 8]
                src = A2 if flags & LINK_A2 else A
                ia = (int(flags) >> 16) & 0xffff
                al = alphas[2 * ia] if ia else 1.0
                if flags & LINK_UNIT:
                    assert k == 0, "unit-factor links are stored with k = 0"
                    units += al * _strided(src, a_off + r0 * a_rs + c0 * a_ks, out.shape, (a_rs, a_ks))
                    continue
                if k <= 0:
                    continue
                Am = _strided(src, a_off + r0 * a_rs, (r1 - r0, k), (a_rs, a_ks))
                if ia:
                    Am = al * Am
                Bm = _strided(B, b_off + c0 * b_ns, (k, c1 - c0), (b_ks, b_ns))
                out += Am @ Bm
            out += units
            Cm = _strided(C, c_off + r0 * ldc + c0, out.shape, (ldc, 1), writeable=True)
            if acc:
                Cm += out
            else:
                Cm[...] = out
        return 0

    def tpa_unit_defect_batch(self, code, jobs_p, n_jobs, src_p, out_p, stream):
        out = REG.view(out_p, np.float64)
        out[0] = 0.
        if n_jobs == 0:
            return 0
        dt = _npdt(code)
        jobs = REG.view(jobs_p, np.int64)[:4 * n_jobs].reshape(n_jobs, 4)
        src = REG.view(src_p, dt)
        worst = 0.
        for off, n, ld, _ in jobs:
            blk = _strided(src, off, (n, n), (ld, 1))
            d = np.abs(blk - np.eye(n))
            worst = np.inf if np.any(np.isnan(d)) else max(worst, float(np.max(d)))
        out[0] = worst
        return 0

    def tpa_lanczos_run(self, code, n, ops_p, n_ops, bufs_p, n_bufs, krylov_p, psi0_p, N_max, cutoff, has_shift, E_shift,
                        scal_p, scr_p, cb, user, time_gemms, info_p, stream):
        """A COPY of ``mock_device.MockLib.tpa_lanczos_run`` (that file is not edited) with one more branch, op kind 7 = kind 0 through
        ``tpa_gemm_chain_ex`` (field 9 = slot of A2, field 10 = alphas).  Everything else mirrors the original line by line: a change
        there has to be repeated here."""
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
                    self.tpa_gemm_chain(code, int(op[1]), int(op[2]), int(op[3]), int(op[4]), int(op[5]), a, b, c, stream)
                elif op[0] == 7:
                    self.tpa_gemm_chain_ex(code, int(op[1]), int(op[2]), int(op[3]), int(op[4]), int(op[5]), a, slot(op[9], vin, w), b, c,
                                           int(op[10]), stream)
                elif op[0] == 1:
                    self.tpa_lincomb_batch(code, int(op[2]), int(op[5]), int(op[3]), int(op[9]), a, c, stream)
                elif op[0] == 2:
                    self.tpa_copy_batch(code, int(op[2]), int(op[5]), int(op[9]), a, c, stream)
                else:
                    assert op[0] == 3 and self._collective is not None
                    assert self._collective(int(op[1]), None) == 0
            n_mv += 1
            if has_shift:
                self.tpa_axpy(code, n, E_shift, 0., vin, w, stream)
            self.tpa_lanczos_step(code, n, w, vin, V(k - 1) if k > 0 else None, scal_p + 8 * (2 * (k - 1) + 1) if k > 0 else None,
                                  scal_p + 8 * 2 * k, scr_p, stream)
            ab = REG.view(scal_p + 8 * 2 * k, np.float64)
            hist[k] = (float(ab[0]), float(ab[1]))
            if k > 0 and cb(k - 1, hist[k - 1][0], hist[k - 1][1], user):
                N, stopped = k, True
                break
            N = k + 1
        if not stopped:
            cb(N_max - 1, hist[N_max - 1][0], hist[N_max - 1][1], user)
        info[0], info[1], info[2] = N, n_mv, 0.
        return 0


def install(monkeypatch):
    """``mock_device.install`` with ``MockLibEx`` as the library."""
    mock_device.install(monkeypatch)
    mock = MockLibEx()
    monkeypatch.setattr(dev, "lib", lambda: mock)
    return mock
