"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_site_inner_batch`` (the closing values <b| op |x_s> of a whole stack of rows of a
correlation function in one call), on top of ``mock_mpo_cell`` (and through it ``mock_expand``, ``mock_mixer``, ``mock_mpo_entry``,
``mock_mpo_apply``, ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h``; set as an attribute of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
this attribute).  ``tpa_site_inner_work`` touches no memory and is forwarded.  ``calls`` counts the calls of the entry point."""
import numpy as np

import mock_mpo_cell
from mock_device import REG, _npdt
from tenpy_amd import _lib

calls = {'tpa_site_inner_batch': 0}


def tpa_site_inner_batch(code, jobs_p, n_jobs, coeff_p, max_d, n_stack, n_out, max_cols, b_p, x_p, out_p, work_p, stream):
    calls['tpa_site_inner_batch'] += 1
    if code not in (0, 1) or not 1 <= max_d <= _lib.MPO_APPLY_MAXD or n_stack < 1 or n_out < 1 or not out_p:
        return _lib.E_BADARG
    out = REG.view(out_p, np.float64)
    if n_jobs <= 0:
        out[:2 * n_stack * n_out] = 0.
        return 0
    if n_jobs > 65535 or not (jobs_p and coeff_p and b_p and x_p and work_p):
        return _lib.E_BADARG
    dt = _npdt(code)
    jobs = REG.view(jobs_p, np.int64)[:12 * n_jobs].reshape(n_jobs, 12)
    coeff, b, x = REG.view(coeff_p, dt), REG.view(b_p, dt), REG.view(x_p, dt)
    res = np.zeros((n_stack, n_out), dtype=np.complex128)
    ss = np.arange(n_stack)
    for b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, c_off, col, _ in jobs.tolist():
        if not 0 <= col < n_out or min(d_b, d_x, pre, post) <= 0:
            continue
        assert pre * post <= max_cols, "max_job_cols too small"
        nb, nx = min(d_b, max_d), min(d_x, max_d)
        ii, jj = np.arange(pre)[:, None, None], np.arange(post)[None, None, :]
        bb = b[b_off + ii * b_ld + np.arange(nb)[None, :, None] * post + jj]                                  # (pre, nb, post)
        xx = x[x_off + ii[None] * x_ld + ss[:, None, None, None] * x_ss + np.arange(nx)[None, None, :, None] * post + jj[None]]
        A = coeff[c_off + np.arange(nb)[:, None] * d_x + np.arange(nx)[None, :]]                               # (nb, nx)
        t = np.einsum('ioj,oc->icj', bb.conj(), A)
        res[:, col] += np.einsum('icj,sicj->s', t, xx)
    flat = out[:2 * n_stack * n_out].reshape(n_stack, n_out, 2)
    flat[:, :, 0], flat[:, :, 1] = res.real, (res.imag if code == 1 else 0.)
    return 0


def install(monkeypatch):
    """``mock_mpo_cell.install`` plus the emulation of this file; returns the ``MockLib`` instance."""
    mock = mock_mpo_cell.install(monkeypatch)
    mock.tpa_site_inner_batch = tpa_site_inner_batch
    return mock
