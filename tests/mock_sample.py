"""TEST INFRASTRUCTURE ONLY: numpy emulations of ``tpa_sample_select_batch`` (Born probabilities and the outcome of every row of a
stack) and ``tpa_sample_gather_batch`` (the chosen slices, divided by their norms, written into the next stack), on top of
``mock_measure`` (and through it every other emulation).

Written from the contract in ``include/tenpy_amd.h``; set as attributes of the ``MockLib`` instance, because names that instance does
not have are forwarded to the real shared library, which would be handed host pointers (``_device.lib_provides`` looks for exactly
these attributes).  ``calls`` counts the calls of the two entry points."""
import numpy as np

import mock_measure
from mock_device import REG, _npdt
from tenpy_amd import _lib

calls = {'tpa_sample_select_batch': 0, 'tpa_sample_gather_batch': 0}


def tpa_sample_select_batch(code, segs_p, n_segs, groups_p, n_groups, dim, n_rows_total, x_p, u_p, out_p, stream):
    calls['tpa_sample_select_batch'] += 1
    if code not in (0, 1) or not 1 <= dim <= _lib.SAMPLE_MAX_DIM or n_segs < 0 or n_groups < 0:
        return _lib.E_BADARG
    if n_rows_total <= 0:
        return 0
    if not (segs_p and groups_p and x_p and u_p and out_p):
        return _lib.E_BADARG
    segs = REG.view(segs_p, np.int64)[:8 * n_segs].reshape(n_segs, 8)
    groups = REG.view(groups_p, np.int64)[:4 * n_groups].reshape(n_groups, 4)
    x, u = REG.view(x_p, _npdt(code)), REG.view(u_p, np.float64)
    out = REG.view(out_p, np.float64)[:4 * n_rows_total].reshape(n_rows_total, 4)
    group_of = np.full(n_rows_total, -1)
    for g in range(n_groups - 1, -1, -1):       # (the first group that holds a row wins)
        r0, nr = int(groups[g, 2]), int(groups[g, 3])
        lo, hi = max(r0, 0), min(r0 + nr, n_rows_total)
        if hi > lo:
            group_of[lo:hi] = g
    for r in range(n_rows_total):
        p = np.zeros(dim)
        g = group_of[r]
        if g >= 0:
            i = r - int(groups[g, 2])
            for s in range(int(groups[g, 0]), int(groups[g, 0] + groups[g, 1])):
                if not 0 <= s < n_segs:
                    continue
                x_off, x_ld, d, post, sigma0 = segs[s, :5].tolist()
                if post <= 0:
                    continue
                for c in range(d):
                    if 0 <= sigma0 + c < dim:
                        v = x[x_off + i * x_ld + c * post: x_off + i * x_ld + (c + 1) * post]
                        p[sigma0 + c] = np.sum(v.real**2 + v.imag**2)
        total = 0.
        for s in range(dim):
            total += p[s]
        if not (total > 0. and np.isfinite(total)):
            out[r] = (-1., 0., total, 0.)
            continue
        run, count, last = 0., 0, 0
        for s in range(dim):
            run += p[s]
            count += bool(run / total <= u[r])
            if p[s] > 0:
                last = s
        pick = min(count, last)
        out[r] = (float(pick), np.sqrt(p[pick]), total, 0.)
    return 0


def tpa_sample_gather_batch(code, rows_p, n_rows, src_p, out_p, dst_p, stream):
    calls['tpa_sample_gather_batch'] += 1
    if code not in (0, 1):
        return _lib.E_BADARG
    if n_rows <= 0:
        return 0
    if not (rows_p and src_p and out_p and dst_p) or src_p == dst_p:
        return _lib.E_BADARG
    dt = _npdt(code)
    rows = REG.view(rows_p, np.int64)[:4 * n_rows].reshape(n_rows, 4)
    src, dst, out = REG.view(src_p, dt), REG.view(dst_p, dt), REG.view(out_p, np.float64)
    for src_off, n, dst_off, out_row in rows.tolist():
        if n <= 0:
            continue
        w = out[4 * out_row + 1]
        v = src[src_off:src_off + n]
        with np.errstate(all='ignore'):
            if code == 1:       # component by component: a true division of the real and of the imaginary part
                dst[dst_off:dst_off + n] = v.real / w + 1j * (v.imag / w)
            else:
                dst[dst_off:dst_off + n] = v / w
    return 0


def install(monkeypatch):
    """``mock_measure.install`` plus the emulations of this file; returns the ``MockLib`` instance."""
    mock = mock_measure.install(monkeypatch)
    mock.tpa_sample_select_batch = tpa_sample_select_batch
    mock.tpa_sample_gather_batch = tpa_sample_gather_batch
    return mock
