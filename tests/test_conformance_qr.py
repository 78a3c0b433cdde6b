"""Conformance of the Householder / compact-WY kernel family (csrc/tpa_qrp.inc and its two drivers) against the K5 / K6 sections of
include/tenpy_amd.h: ``tpa_qr_batch`` on every dispatch path, and the pivoted panel variants of ``tpa_svd_batch``.  Every case runs
on the numpy emulation (LAPACK) and, marked ``gpu``, on the HIP kernels; the test id names the dispatch path of the device.

What one QR call is held to (tests/conformance_qr_cases.py::check_qr): outputs go into NaN-filled arenas with canaries in every gap;
backward error per column and orthogonality within the bounds below; R below the diagonal exactly +0.0 and a real diagonal; R of the
well-conditioned blocks equal to an unblocked long double Householder QR in LAPACK's sign convention; the A arena and every canary
bit-identical; a second identical call bit-identical.

BOUNDS.  Form: c f eps sqrt(k) for the backward error and the R factor, c f eps sqrt(m) for orthogonality (k = min(m, n), eps = 2^-53,
f = 4 for complex data, the column norms of A as the scale); the SVD measures use sigma_1 and sqrt(max(m, n)).  c is calibrated on
the REFERENCE implementation, never on the kernels: the committed cases run through the emulation (LAPACK geqrf / orgqr, gesvd), c =
8 x (the largest ratio error / (f eps sqrt(.)) LAPACK reaches), rounded up to a power of two.  The margin of 8 covers another
summation order on the matrix cores and blocked against unblocked reflector application.  Measured with LAPACK (OpenBLAS, x86-64),
largest over all committed cases (the mock halves of the tests print them as CALIBRATION lines and assert the margin):

    measure                                   LAPACK ratio   x 8      c
    QR backward error                         6.00           48.0     64
    QR orthogonality                          3.78           30.2     32
    QR R factor against long double           2.24           17.9     32
    SVD |S - sigma| / sigma_1                 0.241          1.93     2
    SVD residual of U S VH                    1.11           8.90     16
    SVD orthonormality of U, VH               2.05           16.4     32
"""
import os

import numpy as np
import pytest

import conformance_qr_cases as cq
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev


def _report(what, inst, ratios):
    print("CONFORMANCE %s %s %s" % (what, inst, " ".join("%s=%.4f" % kv for kv in sorted(ratios.items()))))


# ---- the cases themselves (no device) -----------------------------------------------------------------------------------------

def test_every_batch_holds_every_kind_and_a_block_that_pins_r():
    for name in list(cq.QR_CASES) + list(cq.NEGATIVE_OFFSET_CASES):
        c = cq.qr_case(name)
        for kind in (cq.KINDS_COMPLEX if c.cplx else cq.KINDS_REAL):       # not the label alone: a block on which the kind acts
            mine = [b for b in c.blocks if b.kind == kind and cq.acts(kind, b.m, b.n)]
            assert mine, "%s: no block on which '%s' acts" % (name, kind)
            j = {'zero_column': lambda b: b.n // 2, 'equal_columns': lambda b: (b.n - 1) // 2}.get(kind)
            if j:       # the special column is reduced: among the first k, with rows below its diagonal element
                assert any(j(b) < b.k and j(b) + 1 < b.m for b in mine), (name, kind)
            if kind == 'zero_column':
                assert all(not b.a[:, b.n // 2].any() for b in mine)
            if kind == 'triangular':
                assert any(b.k >= 2 and not np.tril(b.a, -1).any() and not np.diagonal(b.a).imag.any() for b in mine), name
            if kind in ('negative_real_lead', 'imaginary_lead'):          # the sign convention at Re x0 < 0 / Re x0 == +0.0: R is compared
                b = next((b for b in mine if b.compare_r), None)
                assert b is not None and b.m >= 2 * b.n, (name, kind)
                lead = b.a[0, 0]
                assert (lead.real < 0 and lead.imag == 0) if kind == 'negative_real_lead' else \
                    (lead.real == 0 and not np.signbit(lead.real) and lead.imag != 0), (name, kind)
        assert any(b.kind == 'gaussian' and b.compare_r for b in c.blocks), name      # some block pins the sign convention
        if c.blocks[0].m >= 2 * c.blocks[0].n:                                        # ... the path-defining one where it is tall
            assert c.blocks[0].kind == 'gaussian' and c.blocks[0].compare_r, name
        assert np.isnan(c.Q0[c.q_mask].view(np.float64)).all() and np.isfinite(c.Q0[~c.q_mask].view(np.float64)).all()
        assert np.isnan(c.R0[c.r_mask].view(np.float64)).all() and np.isfinite(c.R0[~c.r_mask].view(np.float64)).all()
        for mask in (c.q_mask, c.r_mask):      # a canary in front of, between and behind the blocks
            assert not mask[0] and not mask[-1] and len(np.flatnonzero(mask[1:] & ~mask[:-1])) == len(c.blocks)


def test_long_double_householder_is_a_qr_in_lapack_convention():
    rng = np.random.default_rng(5)
    for cplx in (False, True):
        a = cq.make_block(rng, 23, 11, cplx, 'gaussian')
        r_ld = cq.qr_householder_ld(a)
        q, r = np.linalg.qr(a)
        assert np.max(np.abs(r_ld - r)) < 1e-13 * np.max(np.abs(r)), "LAPACK itself follows the convention of the reference"
        assert np.all(np.diagonal(r_ld).imag == 0)
        t = cq.make_block(rng, 9, 12, cplx, 'triangular')
        assert np.array_equal(cq.qr_householder_ld(t), t.astype(r_ld.dtype))       # H = I throughout: A is returned as it is


# ---- tpa_qr_batch on every dispatch path --------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(cq.QR_CASES) + list(cq.NEGATIVE_OFFSET_CASES))
def test_qr_batch(backend, path):
    c = cq.qr_case(path)
    out = cq.run_qr(c)
    if path in cq.NEGATIVE_OFFSET_CASES:
        assert (out['a_off'] < 0).any() and (out['a_off'] > 0).any() and len(c.A) == 2
    ratios = cq.check_qr(c, out)
    _report("tpa_qr_batch[%s]" % backend, path, ratios)
    if backend == 'mock':
        _lapack_calibration("qr", path, ratios, _C)
    cq.check_repeatable(c, out, cq.run_qr(c))


_C = dict(backward=cq.C_BACKWARD, orthogonality=cq.C_ORTH, rfactor=cq.C_RFACTOR, S=cq.C_SVD_S, residual=cq.C_SVD_RESIDUAL)


def _lapack_calibration(what, name, ratios, c):
    """The emulation is LAPACK: c was chosen a factor 8 .. 16 above the largest ratio it reaches over the cases, so every case stays
    a factor 8 below its bound.  (Asserted with a factor 4: another build of LAPACK sums in another order.)  The printed lines
    are what the table in the docstring was made from."""
    for key, v in sorted(ratios.items()):
        print("CALIBRATION %s %s %s: LAPACK ratio %.3f, c = %d" % (what, name, key, v * c[key], c[key]))
    assert all(v <= 1 / 4 for v in ratios.values()), (name, ratios)


# ---- argument behaviour -------------------------------------------------------------------------------------------------------

def _call(cplx, jobs, a, q0, r0):
    jobs = np.array(jobs, np.int64).reshape(-1, 8)
    Ad, Qd, Rd = dev.to_device(a), dev.to_device(q0), dev.to_device(r0)
    rc = dev.lib().tpa_qr_batch(int(cplx), jobs.ctypes.data, len(jobs), Ad.data_ptr(), Qd.data_ptr(), Rd.data_ptr(), dev.stream())
    return rc, dev.to_host(Qd), dev.to_host(Rd)


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_qr_arguments(backend, cplx):
    dt = np.complex128 if cplx else np.float64
    a = np.arange(1., 13.).astype(dt)
    nan = np.full(12, cq._nan(dt), dt)
    rc, q, r = _call(cplx, [], a, nan, nan)
    assert rc == 0 and np.isnan(q.view(np.float64)).all() and np.isnan(r.view(np.float64)).all()          # n_jobs = 0
    for m, n in ((0, 3), (3, 0)):
        rc, q, r = _call(cplx, [[0, 3, 4, 0, 0, 0, 0, 0], [0, m, n, 0, 0, 0, 0, 0]], a, nan, nan)
        assert rc == _lib.E_BADARG
        assert np.isnan(q.view(np.float64)).all() and np.isnan(r.view(np.float64)).all(), "outputs written before the argument check"


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_qr_one_workgroup_row_limit(backend, cplx):
    """The reflector of the one-workgroup kernel lives in LDS (150 KB): 19200 rows of f64 / 9600 of c128 are factorised, one more is
    TPA_E_BADARG with the outputs untouched."""
    dt = np.complex128 if cplx else np.float64
    m = cq.ONEWG_LDS_BYTES // np.dtype(dt).itemsize
    assert m == (9600 if cplx else 19200)
    x = cq.make_block(np.random.default_rng(8), m + 1, 1, cplx, 'gaussian').reshape(-1)
    q0 = np.full(m + 3, cq._nan(dt), dt)
    q0[m:] = [7., 8., 9.]
    r0 = np.array([cq._nan(dt), 5.], dt)
    rc, q, r = _call(cplx, [[0, m, 1, 0, 0, 0, 0, 0]], x, q0, r0)
    assert rc == 0
    assert np.array_equal(cq.bits(q[m:]), cq.bits(q0[m:])) and np.array_equal(cq.bits(r[1:]), cq.bits(r0[1:]))
    nrm = np.sqrt(np.sum(np.abs(x[:m].astype(cq.CLD if cplx else cq.LD)) ** 2))
    assert r[0].imag == 0 and abs(abs(r[0]) - nrm) <= cq.C_RFACTOR * cq._f(cplx) * cq.EPS * nrm
    assert float(np.max(cq.qr_backward(x[:m, None], q[:m, None], r[:1, None]))) <= cq.C_BACKWARD * cq._f(cplx) * cq.EPS
    assert float(cq.qr_orthogonality(q[:m, None])) <= cq.C_ORTH * cq._f(cplx) * cq.EPS * np.sqrt(m)
    rc, q, r = _call(cplx, [[0, m + 1, 1, 0, 0, 0, 0, 0]], x, q0, r0)
    assert rc == _lib.E_BADARG
    assert np.array_equal(cq.bits(q), cq.bits(q0)) and np.array_equal(cq.bits(r), cq.bits(r0))


# ---- the pivoted panel variants of the rank-revealing QR, through tpa_svd_batch -------------------------------------------------

@pytest.mark.parametrize("variant", list(cq.SVD_CASES))
def test_svd_pivoted_panel_variant(backend, variant):
    c = cq.svd_case(variant)
    L = dev.lib()
    if backend == 'gpu':       # (svd_run_qrp reads the variable on every call: 0 would turn the <64,8> ids into <256,8> runs)
        assert os.environ.get('TPA_SVD_SMALL_PANEL', '1') == '1', "the test ids name the panel variants of the default switches"
    out = cq.run_svd(c)
    if backend == 'gpu':
        assert cq.svd_used_pivoted_qr(L), "the call must take the pivoted-QR path"
    ratios = cq.check_svd(c, out)
    _report("tpa_svd_batch[%s]" % backend, variant, ratios)
    if backend == 'mock':
        _lapack_calibration("svd", variant, ratios, dict(_C, orthogonality=cq.C_SVD_ORTH))
