"""TEST INFRASTRUCTURE ONLY: numpy emulation of ``tpa_mpo_expand_batch`` (the fused matrix of the subspace expansion of single-site
DMRG: ``tpa_mpo_entry_apply_batch`` with a destination offset per row and a second source), on top of ``mock_mixer`` (and through it
``mock_mpo_entry``, ``mock_mpo_apply``, ``mock_ortho``, ``mock_evolve`` and ``mock_device``).

Written from the contract in ``include/tenpy_amd.h``; set as an attribute of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
this attribute).  ``calls`` counts the calls of the entry point."""
import numpy as np

import mock_mixer
from mock_device import REG, _npdt
from tenpy_amd import _lib

calls = {'tpa_mpo_expand_batch': 0}


def tpa_mpo_expand_batch(code, jobs_p, n_jobs, rows_p, terms_p, max_cols, src_p, src2_p, dst_p, stream):
    calls['tpa_mpo_expand_batch'] += 1
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
    rows = REG.view(rows_p, np.int64)[:4 * n_rows].reshape(n_rows, 4)
    terms = REG.view(terms_p, np.int64) if terms_p else np.zeros(0, np.int64)
    src, dst = REG.view(src_p, dt), REG.view(dst_p, dt)
    src2 = None                            # looked up only when a row selects it: src2_base may be NULL otherwise
    for dst_off, pre, nr, post, r0, dst_ld, _, _ in live.tolist():
        assert pre * post <= max_cols, "max_job_cols too small"
        ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
        for o in range(nr):
            t0, nt, row_off, sel = rows[r0 + o].tolist()
            if sel and src2 is None:
                src2 = REG.view(src2_p, dt)
            x = src2 if sel else src
            acc = np.zeros((pre, post), dtype=dt)
            for src_off, src_ld, a_re, a_im in terms[4 * t0:4 * (t0 + nt)].reshape(nt, 4).tolist():      # terms in table order
                alpha = complex(*np.array([a_re, a_im], dtype=np.int64).view(np.float64))
                acc = acc + (alpha if code == 1 else alpha.real) * x[src_off + ii * src_ld + jj]
            dst[dst_off + ii * dst_ld + row_off + jj] = acc
    return 0


def install(monkeypatch):
    """``mock_mixer.install`` plus the emulation of this file; returns the ``MockLib`` instance."""
    mock = mock_mixer.install(monkeypatch)
    mock.tpa_mpo_expand_batch = tpa_mpo_expand_batch
    return mock
