"""Conformance of ``tpa_project_out`` (dst = src - sum_j <b_j|src> b_j over m packed vectors) with the extended-precision statement of
the header, on the numpy emulation (``mock``) and on the HIP kernels (``gpu``), real and complex, in the style of
``test_conformance_vec.py``.

Launch geometry (documented next to the kernels in csrc/tpa_vec.hip and repeated by ``geometry`` below).  The 16-byte form runs when
basis, src and dst are 16-byte aligned and, for real data, n and (for m > 1) the stride are even; an ITEM is then 16 bytes (one complex
or two real elements), otherwise one element.  256 threads, 4 items per thread: g = min(1024, ceil(items / 1024)) workgroups, grid
stride.  So the edges are: one thread, one wavefront (64), one workgroup (256), one workgroup's share (1024 items), the cap of the grid
(1024 * 1024 items = 2^20 elements, 2^21 real elements in the 16-byte form) and 2^22 + 3 (more than one grid-stride pass).  The
coefficients are taken for J = 8 vectors per read of src: m = 1, 7, 8, 9 and 64 (= TPA_PROJECT_MAX).

Bounds (derived; EPS = 2^-52 = 2 u).
Coefficients: a term of c_j passes P p additions of its thread's loop (p = ceil(items / (256 g)); P = 2 products per item for complex
data and for the 16-byte real form, else 1), 6 + 4 of the tree over the workgroup, ceil(g / 256) of the thread's share of the partials in
pass 2 and 6 + 4 of that workgroup's tree: L = P p + ceil(g / 256) + 20, |err| <= (L + 2) EPS sum_i |b_j[i] src[i]| per component, as in
test_conformance_vec.py.
Vector: dst_i is a chain of m (real) or 2 m (complex) fused multiply-adds, so a term is rounded at most that often, and the device
uses its own c_j: per component  sum_j lim(c_j) |b_j[i]| + R (m + 1) EPS (|src_i| + sum_j |c_j| |b_j[i]|), R = 1 real, 2 complex.
Norm: first-order propagation, sum_i (2 |d_i| e_i + e_i^2) for the elementwise bounds e, plus (L + 2) EPS sum |d_i|^2 for its reduction
(the same L: the pass that writes dst has the grid of the coefficient pass)."""
import numpy as np
import pytest

import kernel_reference as kref
from ortho_fixtures import obackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

EPS = 2.0**-52
LD = np.longdouble
J = 8
CAP = 1024 * 1024           # items at which the grid is capped
GUARD = 4                   # doubles in front of and behind every payload (even: the payload keeps its alignment)
SENTINEL = -7.25e300


def geometry(cplx, n, m, stride, misaligned):
    """(items, products per item, g, L) of the module docstring."""
    vec = not misaligned and (cplx or (n % 2 == 0 and (m <= 1 or stride % 2 == 0)))
    items = n // 2 if (vec and not cplx) else n
    P = 2 if (cplx or vec) else 1
    g = min(1024, max(1, -(-items // 1024)))
    p = -(-items // (256 * g))
    return items, P, g, P * p + -(-g // 256) + 20


def test_geometry():
    assert geometry(False, 1025, 1, 1025, False)[1:] == (1, 2, 3 + 1 + 20)            # odd n: 8-byte form, 2 workgroups
    assert geometry(False, 2048, 9, 2048, False)[:3] == (1024, 2, 1)                  # 16-byte form: one workgroup's share
    assert geometry(False, 2048, 9, 2049, False)[:3] == (2048, 1, 2)                  # odd stride: 8-byte form
    assert geometry(True, CAP + 1, 1, CAP + 1, False)[1:] == (2, 1024, 2 * 5 + 4 + 20)
    assert geometry(False, 2**22 + 3, 1, 2**22 + 3, False)[1:] == (1, 1024, 17 + 4 + 20)


def _vec(rng, n, cplx):
    v = rng.standard_normal(n)
    return v + 1j * rng.standard_normal(n) if cplx else v


def _flat(x):
    return np.ascontiguousarray(x).view(np.float64).reshape(-1)


class _Buf:
    """A payload of doubles between guards on the device, optionally 8 bytes off a 16-byte boundary."""

    def __init__(self, payload, off8):
        self.lead = GUARD + (1 if off8 else 0)
        self.host = np.concatenate([np.full(self.lead, SENTINEL), payload, np.full(GUARD, SENTINEL)])
        self.dev = dev.to_device(self.host)
        self.n = len(payload)

    @property
    def ptr(self):
        return self.dev.data_ptr() + 8 * self.lead

    def reset(self):
        self.dev.copy_(dev.to_device(self.host))

    def get(self):
        got = dev.to_host(self.dev)
        assert np.array_equal(kref.bits(got[:self.lead]), kref.bits(self.host[:self.lead])), "written in front of the payload"
        assert np.array_equal(kref.bits(got[self.lead + self.n:]), kref.bits(self.host[self.lead + self.n:])), "written behind the payload"
        return got[self.lead:self.lead + self.n].copy()


def reference(B, src):
    """Extended precision: coefficients (re, im, magnitude sums) and dst = src - sum_j c_j b_j with the magnitudes of its terms."""
    sr, si = kref.split(src)
    dr, di = sr.copy(), si.copy()
    mr, mi = np.abs(sr), np.abs(si)
    coeff = []
    for b in B:
        cr, ci, mcr, mci = kref.dot(b, src, True)
        br, bi = kref.split(b)
        coeff.append((cr, ci, mcr, mci))
        dr -= cr * br - ci * bi
        di -= cr * bi + ci * br
        mr += np.abs(cr * br) + np.abs(ci * bi)
        mi += np.abs(cr * bi) + np.abs(ci * br)
    return coeff, dr, di, mr, mi


def run_and_check(cplx, n, m, gap=0, inplace=False, with_nrm=True, mis=None, tag=''):
    """One call (twice: bit-identical), everything the header promises checked; -> worst err / bound."""
    L = dev.lib()
    W = 2 if cplx else 1
    stride = n + gap
    rng = np.random.default_rng([sum(map(ord, 'project' + tag)), int(cplx), n, m, gap])
    B = [_vec(rng, n, cplx) for _ in range(m)]
    src = _vec(rng, n, cplx)
    basis_host = np.full(max((m - 1) * stride + n, 1) * W if m else W, np.nan)        # NaN in the gaps: never to be read
    for j, b in enumerate(B):
        basis_host[j * stride * W:(j * stride + n) * W] = _flat(b)
    bb = _Buf(basis_host, mis == 'basis')
    sb = _Buf(_flat(src), mis == 'src')
    db = sb if inplace else _Buf(np.full(n * W, SENTINEL), mis == 'dst')
    cb = _Buf(np.full(2 * m, SENTINEL), False)
    nb = _Buf(np.full(2, SENTINEL), False)
    work = dev.scratch('project_test_work', _lib.PROJECT_WORK, np.float64)
    res = []
    for _ in range(2):
        for b in (sb, db, cb, nb):
            b.reset()
        dev.check(L.tpa_project_out(int(cplx), n, bb.ptr if m else None, m, stride, sb.ptr, db.ptr, cb.ptr if m else None,
                                    nb.ptr if with_nrm else None, work.data_ptr(), dev.stream()), "project_out")
        res.append((db.get(), cb.get(), nb.get()))
        assert np.array_equal(kref.bits(bb.get()), kref.bits(basis_host)), "the basis was written"
        if not inplace:
            assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src))), "src was written"
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(kref.bits(a), kref.bits(b)), "tpa_project_out is not deterministic"
    got_d, got_c, got_n = res[0]
    got_d = got_d.view(np.complex128) if cplx else got_d
    misaligned = mis is not None
    _, P, g, Lc = geometry(cplx, n, m, stride, misaligned)
    coeff, dr, di, mr, mi = reference(B, src)
    ratios = []
    lim_c = []
    for j, (cr, ci, mcr, mci) in enumerate(coeff):
        lr, li = (Lc + 2) * EPS * mcr, (Lc + 2) * EPS * mci
        lim_c.append((lr, li))
        er, ei = abs(LD(got_c[2 * j]) - cr), abs(LD(got_c[2 * j + 1]) - ci)
        assert er <= lr and ei <= li, "coefficient %d: err / bound = %.3g, %.3g" % (j, er / max(lr, LD(1e-300)), ei / max(li, LD(1e-300)))
        if not cplx:
            assert got_c[2 * j + 1] == 0
        ratios += [float(er / lr) if lr > 0 else 0., float(ei / li) if li > 0 else 0.]
    R = 2 if cplx else 1
    e_re, e_im = R * (m + 1) * EPS * mr, R * (m + 1) * EPS * mi
    for (lr, li), b in zip(lim_c, B):
        br, bi = kref.split(b)
        e_re = e_re + lr * np.abs(br) + li * np.abs(bi)
        e_im = e_im + lr * np.abs(bi) + li * np.abs(br)
    gr, gi = kref.split(got_d)
    err_r, err_i = np.abs(gr - dr), np.abs(gi - di)
    assert np.all(err_r <= e_re) and np.all(err_i <= e_im), "dst: worst err / bound = %.3g" % float(
        max(np.max(err_r / np.maximum(e_re, LD(1e-300))), np.max(err_i / np.maximum(e_im, LD(1e-300)))))
    ratios.append(float(np.max(err_r / np.maximum(e_re, LD(1e-300)))))
    if cplx:
        ratios.append(float(np.max(err_i / np.maximum(e_im, LD(1e-300)))))
    if with_nrm:
        nrm = np.sum(dr * dr + di * di)
        lim = np.sum(2 * np.abs(dr) * e_re + e_re**2) + np.sum(2 * np.abs(di) * e_im + e_im**2) + (Lc + 2) * EPS * nrm
        en = abs(LD(got_n[0]) - nrm)
        assert en <= lim, "norm: err / bound = %.3g" % float(en / lim)
        assert got_n[1] == 0
        ratios.append(float(en / lim) if lim > 0 else 0.)
    else:
        assert np.array_equal(kref.bits(got_n), kref.bits(np.full(2, SENTINEL)))
    r = max(ratios) if ratios else 0.
    print("CONFORMANCE tpa_project_out(%s) %s n=%d m=%d stride=n+%d %s%s%s g=%d L=%d max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', n, m, gap, 'inplace' if inplace else 'outofplace', ' nrm2' if with_nrm else '',
             ' mis=' + mis if mis else '', g, Lc, r))
    return r


SMALL = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2046, 2047, 2048, 2049, 2050]


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_lengths(obackend, cplx, n):
    """The small edges: m = J + 1 (two chunks of the coefficient pass), alternating in place / out of place and with / without norm."""
    run_and_check(cplx, n, J + 1, inplace=bool(n % 2), with_nrm=bool(n % 3), tag='len')


@pytest.mark.parametrize("m", [1, J - 1, J, J + 1, 64])
@pytest.mark.parametrize("gap", [0, 1], ids=['dense', 'gap'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_m_and_stride(obackend, cplx, gap, m):
    """Every m at the edges of the chunking, stride = n and n + 1 (real data: odd stride, the 8-byte form), n even and odd."""
    for n in (258, 1025):
        run_and_check(cplx, n, m, gap=gap, inplace=(m % 2 == 0), with_nrm=True, tag='m')


@pytest.mark.parametrize("mis", ['basis', 'src', 'dst'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(obackend, cplx, mis):
    """A base pointer 8 bytes off a 16-byte boundary (real data: an odd offset into an arena): the 8-byte form -- also at exactly one
    workgroup's share of it (n = 1024 items; aligned, that even n takes the 16-byte form with 512 items)."""
    for n in (256, 1024, 2050):
        run_and_check(cplx, n, J + 1, inplace=(mis == 'src'), with_nrm=True, mis=mis, tag='mis')


@pytest.mark.parametrize("inplace", [False, True], ids=['outofplace', 'inplace'])
@pytest.mark.parametrize("with_nrm", [False, True], ids=['plain', 'nrm2'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_variants(obackend, cplx, with_nrm, inplace):
    run_and_check(cplx, 2048, J, inplace=inplace, with_nrm=with_nrm, tag='var')
    run_and_check(cplx, 777, 3, gap=1, inplace=inplace, with_nrm=with_nrm, tag='var')


@pytest.mark.parametrize("case", [('real', CAP - 1, 1, None), ('real', CAP, 1, 'src'), ('real', CAP + 1, 1, None),
                                  ('real', 2 * CAP - 2, 1, None), ('real', 2 * CAP, 1, None), ('real', 2 * CAP + 2, 1, None),
                                  ('complex', CAP - 1, 1, None), ('complex', CAP, 1, None), ('complex', CAP + 1, 1, None),
                                  ('real', 2**22 + 3, 1, None), ('complex', 2**22 + 3, 1, None)],
                         ids=lambda c: "%s-%d-m%d%s" % (c[0], c[1], c[2], '-mis' if c[3] else ''))
def test_grid_cap(obackend, case):
    """The cap of the grid (2^20 items: 8-byte form real -- odd n, or an even n behind a misaligned base --, 16-byte form real at 2^21
    elements, complex) and its neighbours, and lengths beyond it, where the grid-stride loop wraps."""
    kind, n, m, mis = case
    run_and_check(kind == 'complex', n, m, inplace=True, with_nrm=True, mis=mis, tag='cap')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_m_zero(obackend, cplx):
    """m = 0: dst = src bit for bit (a copy; in place nothing), the norm when asked, coeff untouched."""
    L = dev.lib()
    W = 2 if cplx else 1
    for n in (1, 257, 2048):
        for inplace in (False, True):
            for with_nrm in (False, True):
                src = _vec(np.random.default_rng(n), n, cplx)
                sb = _Buf(_flat(src), False)
                db = sb if inplace else _Buf(np.full(n * W, SENTINEL), False)
                cb, nb = _Buf(np.full(2, SENTINEL), False), _Buf(np.full(2, SENTINEL), False)
                work = dev.scratch('project_test_work', _lib.PROJECT_WORK, np.float64)
                assert L.tpa_project_out(int(cplx), n, None, 0, n, sb.ptr, db.ptr, cb.ptr, nb.ptr if with_nrm else None, work.data_ptr(),
                                         dev.stream()) == 0
                assert np.array_equal(kref.bits(db.get()), kref.bits(_flat(src)))
                assert np.array_equal(kref.bits(cb.get()), kref.bits(np.full(2, SENTINEL)))
                got = nb.get()
                if with_nrm:
                    ref = kref.nrm2sq(src)
                    Lc = geometry(cplx, n, 0, n, False)[3]
                    assert abs(LD(got[0]) - ref) <= (Lc + 2) * EPS * ref and got[1] == 0
                else:
                    assert np.array_equal(kref.bits(got), kref.bits(np.full(2, SENTINEL)))


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_n_zero_and_bad_arguments(obackend, cplx):
    """n <= 0: no vector element is touched, coeff[0:2m] and nrm2[0:2] are posted as zeros.  Argument errors: TPA_E_BADARG, and
    nothing is written."""
    L = dev.lib()
    code, W, n, m = int(cplx), 2 if cplx else 1, 64, 3
    rng = np.random.default_rng(9)
    basis = np.concatenate([_flat(_vec(rng, n, cplx)) for _ in range(m)])
    src = _flat(_vec(rng, n, cplx))
    bb, sb, db = _Buf(basis, False), _Buf(src, False), _Buf(np.full(n * W, SENTINEL), False)
    cb, nb = _Buf(np.full(2 * m, SENTINEL), False), _Buf(np.full(2, SENTINEL), False)
    work = dev.scratch('project_test_work', _lib.PROJECT_WORK, np.float64)
    st, wp = dev.stream(), work.data_ptr()
    untouched = np.full(n * W, SENTINEL)
    for n0 in (0, -1):
        cb.reset()
        nb.reset()
        assert L.tpa_project_out(code, n0, bb.ptr, m, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp, st) == 0
        assert cb.get().tolist() == [0.] * (2 * m) and nb.get().tolist() == [0., 0.]
        assert np.array_equal(kref.bits(db.get()), kref.bits(untouched)) and np.array_equal(kref.bits(sb.get()), kref.bits(src))
    cb.reset()
    nb.reset()
    bad = [
        (2, n, bb.ptr, m, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp),                           # dtype
        (code, n, bb.ptr, -1, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp),                       # m < 0
        (code, n, bb.ptr, _lib.PROJECT_MAX + 1, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp),     # m > TPA_PROJECT_MAX
        (code, n, bb.ptr, m, n - 1, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp),                    # stride < n
        (code, n, None, m, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, wp),                          # no basis
        (code, n, bb.ptr, m, n, sb.ptr, db.ptr, None, nb.ptr, wp),                          # no coeff
        (code, n, bb.ptr, m, n, None, db.ptr, cb.ptr, nb.ptr, wp),                          # no src
        (code, n, bb.ptr, m, n, sb.ptr, None, cb.ptr, nb.ptr, wp),                          # no dst
        (code, n, bb.ptr, m, n, sb.ptr, db.ptr, cb.ptr, nb.ptr, None),                      # no work area
        (code, n, bb.ptr, m, n, sb.ptr, bb.ptr + 8 * W * n, cb.ptr, nb.ptr, wp),            # dst overlaps the basis
    ]
    for args in bad:
        assert L.tpa_project_out(*args, st) == _lib.E_BADARG, args
    assert np.array_equal(kref.bits(db.get()), kref.bits(untouched)) and np.array_equal(kref.bits(bb.get()), kref.bits(basis))
    assert np.array_equal(kref.bits(cb.get()), kref.bits(np.full(2 * m, SENTINEL)))
    assert np.array_equal(kref.bits(nb.get()), kref.bits(np.full(2, SENTINEL)))
