"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_mpo_cell_apply_batch`` (a cell of the fused matrix of the zip-up MPO application
as one small dense product: every source row is read once for all rows of the cell), on top of ``mock_expand`` (and through it
``mock_mixer``, ``mock_mpo_entry``, ``mock_mpo_apply``, ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h``; set as an attribute of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
this attribute).  ``calls`` counts the calls of the entry point."""
import numpy as np

import mock_expand
from mock_device import REG, _npdt
from tenpy_amd import _lib

MAXROWS = 32
calls = {'tpa_mpo_cell_apply_batch': 0}


def tpa_mpo_cell_apply_batch(code, jobs_p, n_jobs, rows_p, srcs_p, coeff_p, max_rows, max_cols, src_p, dst_p, stream):
    calls['tpa_mpo_cell_apply_batch'] += 1
    if code not in (0, 1) or not 1 <= max_rows <= MAXROWS:
        return _lib.E_BADARG
    if n_jobs <= 0 or n_jobs > 65535:      # one job per blockIdx.y: the grid limit is an argument error
        return 0 if n_jobs <= 0 else _lib.E_BADARG
    dt = _npdt(code)
    jobs = REG.view(jobs_p, np.int64)[:10 * n_jobs].reshape(n_jobs, 10)
    live = jobs[(jobs[:, 1] > 0) & (jobs[:, 2] > 0) & (jobs[:, 3] > 0)]
    if len(live) == 0:
        return 0
    rows = REG.view(rows_p, np.int64).reshape(-1, 2)
    srcs = REG.view(srcs_p, np.int64).reshape(-1, 2) if srcs_p else np.zeros((0, 2), np.int64)
    coeff = REG.view(coeff_p, dt) if coeff_p else np.zeros(0, dt)
    src, dst = REG.view(src_p, dt), REG.view(dst_p, dt)
    for dst_off, pre, nr, post, dst_ld, r0, s0, ns, c0, _ in live.tolist():
        assert pre * post <= max_cols, "max_job_cols too small"
        ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
        xs = [src[off + ii * ld + jj] for off, ld in srcs[s0:s0 + ns].tolist()]        # every source row once
        for o in range(min(nr, max_rows)):                                             # rows beyond max_rows are not written
            acc = np.zeros((pre, post), dtype=dt)
            for k in range(ns):                                                        # k ascending, zero coefficients included
                acc = acc + coeff[c0 + k * nr + o] * xs[k]
            dst[dst_off + ii * dst_ld + int(rows[r0 + o, 0]) + jj] = acc
    return 0


def install(monkeypatch):
    """``mock_expand.install`` plus the emulation of this file; returns the ``MockLib`` instance."""
    mock = mock_expand.install(monkeypatch)
    mock.tpa_mpo_cell_apply_batch = tpa_mpo_cell_apply_batch
    return mock
