"""``tpa_krylov_combine_z`` through the C-ABI against numpy: ``out = scale * sum_k c_k v_k`` with complex ``c_k``, real and complex
Krylov basis, output always complex128, ``|sum_k c_k v_k|`` (before the scale) returned to the host.

Tolerance (derived, not tuned): every output element is an N-term complex dot product accumulated with fused multiply-adds; each
complex product / sum contributes a few roundings, so ``|err_i| <= 4 N eps * sum_k |c_k| |v_k[i]|`` against an accumulation in
``longdouble``; the final multiplication by ``scale`` adds one more rounding of the result (covered by the factor 4 for N >= 1
together with ``+ eps |ref_i|``).  The norm inherits the element errors, ``| |x + e| - |x| | <= |e|`` with ``e`` the vector of the
bounds above, plus the summation of n non-negative squares in blocks (per thread, per wavefront, per workgroup, over workgroups; the
longest chain has n / (256 * 2048) + 8 + 4 + 8 < 40 additions for n <= 2^22) and one square root: ``+ 44 eps |x|``."""
import ctypes

import numpy as np
import pytest

from tdvp_fixtures import zbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

EPS = np.finfo(np.float64).eps
CASES = [(N, n) for N in (1, 2, 7, 20, 64) for n in (1, 3, 4097, 2**21 + 5) if not (n > 2**21 and N > 20)]


def test_symbol_and_signature():
    lib = _lib.load()
    assert 'tpa_krylov_combine_z' in _lib.exported_symbols()
    f = lib.tpa_krylov_combine_z
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_double,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]


def _combine(basis, c, scale, n, N):
    L = dev.lib()
    V = dev.to_device(basis.reshape(-1))
    out = dev.empty(n, np.complex128)
    red, scr = dev.reduction_buffers()
    coeff = np.ascontiguousarray(np.stack([c.real, c.imag], axis=1))
    nrm = np.full(1, np.nan)
    dev.check(L.tpa_krylov_combine_z(dev.code(basis.dtype), n, V.data_ptr(), N, coeff.ctypes.data, float(scale), out.data_ptr(),
                                     red.data_ptr(), scr.data_ptr(), nrm.ctypes.data, dev.stream()), "krylov_combine_z")
    assert out.dtype == dev.tdtype(np.complex128)
    return dev.to_host(out), float(nrm[0])


@pytest.mark.parametrize("cplx", [False, True], ids=['real_basis', 'complex_basis'])
@pytest.mark.parametrize("N,n", CASES)
def test_combine_z(zbackend, cplx, N, n):
    rng = np.random.default_rng(1000 * N + n % 1000 + int(cplx))
    basis = rng.standard_normal((N, n))
    if cplx:
        basis = basis + 1j * rng.standard_normal((N, n))
    c = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    scale = 0.37
    got, nrm = _combine(basis, c, scale, n, N)
    assert got.dtype == np.complex128 and got.shape == (n,)
    # reference in extended precision, real and imaginary parts separately (numpy has no complex longdouble arithmetic worth trusting)
    ld = np.longdouble
    br, bi = basis.real.astype(ld), (basis.imag.astype(ld) if cplx else np.zeros((N, n), ld))
    cr, ci = c.real.astype(ld)[:, None], c.imag.astype(ld)[:, None]
    ref_re = np.sum(cr * br - ci * bi, axis=0)
    ref_im = np.sum(cr * bi + ci * br, axis=0)
    bound = 4 * N * EPS * (np.abs(c)[:, None] * np.abs(basis)).sum(axis=0)
    ref = (ref_re + 1j * ref_im.astype(np.float64)).astype(np.complex128)
    err = np.abs(got - scale * ref)
    lim = scale * bound + EPS * np.abs(scale * ref)
    print("N=%d n=%d cplx=%d: max err / bound = %.3g" % (N, n, cplx, float(np.max(err / lim))))
    assert np.all(err <= lim)
    nrm_ref = float(np.sqrt(np.sum(ref_re**2 + ref_im**2)))
    print("   norm %.17g ref %.17g" % (nrm, nrm_ref))
    assert abs(nrm - nrm_ref) <= np.linalg.norm(bound) + 44 * EPS * nrm_ref


@pytest.mark.parametrize("cplx", [False, True], ids=['real_basis', 'complex_basis'])
def test_unaligned_base(zbackend, cplx):
    """A Krylov basis that does not start on a 16-byte boundary (a view one double into an arena) takes the scalar form."""
    N, n = 5, 1001
    rng = np.random.default_rng(3)
    basis = rng.standard_normal((N, n))
    if cplx:
        basis = basis + 1j * rng.standard_normal((N, n))
    c = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    L = dev.lib()
    buf = dev.to_device(np.concatenate([[0.], np.ascontiguousarray(basis).reshape(-1).view(np.float64)]))
    out = dev.empty(n, np.complex128)
    red, scr = dev.reduction_buffers()
    coeff = np.ascontiguousarray(np.stack([c.real, c.imag], axis=1))
    nrm = np.zeros(1)
    dev.check(L.tpa_krylov_combine_z(int(cplx), n, buf.data_ptr() + 8, N, coeff.ctypes.data, 1., out.data_ptr(), red.data_ptr(),
                                     scr.data_ptr(), nrm.ctypes.data, dev.stream()), "krylov_combine_z")
    ref = (c[:, None] * basis).sum(axis=0)
    bound = 4 * N * EPS * (np.abs(c)[:, None] * np.abs(basis)).sum(axis=0)
    assert np.all(np.abs(dev.to_host(out) - ref) <= 2 * bound)      # (the float64 reference carries the same bound itself)
    assert abs(nrm[0] - np.linalg.norm(ref)) <= 2 * np.linalg.norm(bound) + 44 * EPS * nrm[0]


def test_bad_arguments():
    """Argument checks run before any device work."""
    lib = _lib.load()
    x = np.zeros(4)
    assert lib.tpa_krylov_combine_z(0, 4, x.ctypes.data, 65, x.ctypes.data, 1., x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                    x.ctypes.data, None) == _lib.E_BADARG
    assert lib.tpa_krylov_combine_z(2, 4, x.ctypes.data, 1, x.ctypes.data, 1., x.ctypes.data, x.ctypes.data, x.ctypes.data,
                                    x.ctypes.data, None) == _lib.E_BADARG
