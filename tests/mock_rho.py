"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_site_rho_batch`` (the closing step of a reduced density matrix with the physical
index pair left open, for a whole stack of rows in one call), on top of ``mock_measure`` (and through it ``mock_mpo_cell``,
``mock_expand``, ``mock_mixer``, ``mock_mpo_entry``, ``mock_mpo_apply``, ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h``; set as an attribute of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
this attribute).  ``tpa_site_rho_work`` touches no memory and is forwarded.  ``calls`` counts the calls of the entry point."""
import numpy as np

import mock_measure
from mock_device import REG, _npdt
from tenpy_amd import _lib

calls = {'tpa_site_rho_batch': 0}


def tpa_site_rho_batch(code, jobs_p, n_jobs, max_d, n_stack, out_size, max_cols, b_p, x_p, out_p, work_p, stream):
    calls['tpa_site_rho_batch'] += 1
    if code not in (0, 1) or not 1 <= max_d <= _lib.SITE_RHO_MAXD or n_stack < 1 or out_size < 1 or not out_p:
        return _lib.E_BADARG
    if n_stack * out_size > 0x7fffffff:
        return _lib.E_BADARG
    out = REG.view(out_p, np.float64)
    if n_jobs <= 0:
        out[:2 * n_stack * out_size] = 0.
        return 0
    if n_jobs > 65535 or not (jobs_p and b_p and x_p and work_p):
        return _lib.E_BADARG
    dt = _npdt(code)
    jobs = REG.view(jobs_p, np.int64)[:12 * n_jobs].reshape(n_jobs, 12)
    b, x = REG.view(b_p, dt), REG.view(x_p, dt)
    res = np.zeros((n_stack, out_size), dtype=np.complex128)
    ss = np.arange(n_stack)
    tile = min(16, out_size)
    for b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, out_off, out_ld, _ in jobs.tolist():
        if min(d_b, d_x, pre, post) <= 0 or out_ld <= 0:
            continue
        assert pre * post <= max_cols, "max_job_cols too small"
        nb, nx = min(d_b, max_d), min(d_x, max_d)
        ii, jj = np.arange(pre)[:, None, None], np.arange(post)[None, None, :]
        bb = b[b_off + ii * b_ld + np.arange(nb)[None, :, None] * post + jj]                                  # (pre, nb, post)
        xx = x[x_off + ii[None] * x_ld + ss[:, None, None, None] * x_ss + np.arange(nx)[None, None, :, None] * post + jj[None]]
        # (slot by slot, so that a slot's bits do not depend on how many slots the launch has: the walks of a split call agree)
        t = np.stack([np.einsum('ioj,icj->oc', bb.conj(), xx[s]) for s in range(n_stack)])
        for o in range(nb):
            for c in range(nx):
                e = out_off + o * out_ld + c
                if 0 <= e < out_size and o * nx + c < tile:
                    res[:, e] += t[:, o, c]
    flat = out[:2 * n_stack * out_size].reshape(n_stack, out_size, 2)
    flat[:, :, 0], flat[:, :, 1] = res.real, (res.imag if code == 1 else 0.)
    return 0


def install(monkeypatch):
    """``mock_measure.install`` plus the emulation of this file; returns the ``MockLib`` instance."""
    mock = mock_measure.install(monkeypatch)
    mock.tpa_site_rho_batch = tpa_site_rho_batch
    return mock
