"""TEST INFRASTRUCTURE ONLY: numpy emulation of the device entry points that came with the time-evolution path
(``tpa_krylov_combine_z``), on top of ``mock_device``.

``mock_device.MockLib`` forwards names it does not emulate to the real shared library, which would then be handed host pointers;
the emulations of newer entry points therefore live here and are set as attributes of the ``MockLib`` instance that
``mock_device.install`` returns.  Like ``mock_device`` it follows the documented contract of ``include/tenpy_amd.h``."""
import numpy as np

import mock_device
from mock_device import REG, _host, _npdt


def tpa_krylov_combine_z(code, n, krylov_p, N, coeff_p, scale, out_p, red_p, scr_p, norm_p, stream):
    coeff = _host(coeff_p, (N, 2), np.float64)
    c = coeff[:, 0] + 1j * coeff[:, 1]
    V = REG.view(krylov_p, _npdt(code))
    out = REG.view(out_p, np.complex128)[:n]
    acc = np.zeros(n, dtype=np.complex128)
    for k in range(N):
        acc += c[k] * V[k * n:(k + 1) * n]
    nrm2 = float(np.real(np.vdot(acc, acc)))
    out[:] = scale * acc
    red = REG.view(red_p, np.float64)
    red[0], red[1] = nrm2, 0.
    _host(norm_p, (1,), np.float64)[0] = np.sqrt(nrm2)
    return 0


def install(monkeypatch):
    """``mock_device.install`` plus the emulations of this file; returns the ``MockLib`` instance."""
    mock = mock_device.install(monkeypatch)
    mock.tpa_krylov_combine_z = tpa_krylov_combine_z
    return mock
