"""Conformance of the vector entry points (``tpa_dot``, ``tpa_nrm2sq``, ``tpa_axpy``, ``tpa_scal``, ``tpa_lanczos_update``,
``tpa_lanczos_step``, ``tpa_krylov_combine``) with the extended-precision statement of the header (tests/kernel_reference.py), on the
numpy emulation (``mock``) and on the HIP kernels (``gpu``), real and complex, at lengths around every edge of the launch geometry:
one thread, one wavefront (64), one workgroup (256), one workgroup's share of a reduction (256 * 8 = 2048), the length used so far
(100003: 49 workgroups), the cap of the grid at MAXBLK = 1024 workgroups (1024 * 256 * 8 and its neighbours) and 2^22 + 3 (more than
one grid-stride pass with the capped grid -- the regime of the chi = 2048 two-site wave function).

Tolerances (derived; u = 2^-53 is the unit roundoff, EPS = 2^-52 = 2 u; no absolute constants).

Elementwise results.  A term of the magnitude sum ``mag`` (kernel_reference.py) passes through at most r roundings on its way into
the result, so the error is at most gamma_r mag, gamma_r = r u / (1 - r u): r = 1 (fused) or 2 (product, then sum) for real axpy /
scal and for the complex scal (product, difference), r <= 4 for the complex axpy and for the Lanczos updates (product, difference of
products, first and second subtraction).  The tests allow ``R EPS (1 + R EPS) mag`` >= gamma_{2 R} mag with R = 1 resp. 2: "one or two
roundings of the magnitude sum" in units of EPS = 2 u.

Reductions.  The header documents a two-pass tree: pass 1 leaves one partial per workgroup, pass 2 adds the partials in one workgroup.
With P elements per thread the grid is g = min(1024, ceil(n / (256 P))) workgroups (P = 8; tpa_krylov_combine: P = 4), so the longest
chain of additions that a term sees is
      p = ceil(n / (256 g))   its thread's grid-stride loop        (complex dot products and |z|^2: 2 p, two products per element)
    + 6 + 4                   butterfly over the 64 lanes of a wavefront, the 4 wavefronts of the workgroup
    + ceil(g / 256)           the thread's share of the partials in pass 2
    + 6 + 4                   the same tree over the one workgroup of pass 2,
L = (1 or 2) p + ceil(g / 256) + 20, and a sum whose longest chain has L additions obeys |err| <= gamma_L sum |terms| (Higham, section
4.2).  The tests allow ``(L + 2) EPS sum |x_i y_i|``: gamma_{L+1} (one more for the rounding of a product that is not fused) with a
factor two in hand.  (``tpa_nrm2sq`` of complex data is the real reduction over 2 n doubles.)

Composite results (norm after an update, the Lanczos step) propagate these bounds to first order; the formulas stand next to the
assertions.

n = 0 (read from csrc/tpa_vec.hip, pinned by test_n_zero, written into the header): tpa_axpy / tpa_scal do nothing; tpa_dot / tpa_nrm2sq /
tpa_lanczos_update write (0, 0); tpa_lanczos_step writes alpha = 0, bsq = 0 and leaves w alone; tpa_krylov_combine is TPA_E_BADARG."""
import numpy as np
import pytest

import kernel_reference as kref
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

EPS = 2.0**-52
LD = np.longdouble
CAP = 1024 * 256 * 8
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 100003, CAP - 1, CAP, CAP + 1, 2**22 + 3]


def chain_length(n, per_thread=8, products=1):
    """L of the module docstring for a reduction over n items (n >= 1)."""
    g = min(1024, max(1, -(-n // (256 * per_thread))))
    p = -(-n // (256 * g))
    return products * p + -(-g // 256) + 20


def test_chain_length_geometry():
    assert chain_length(100003) == 8 + 1 + 20          # 49 workgroups, 8 elements per thread
    assert chain_length(CAP) == 8 + 4 + 20 and chain_length(CAP + 1) == 9 + 4 + 20
    assert chain_length(2**22 + 3, products=2) == 2 * 17 + 4 + 20


def _vec(rng, n, cplx):
    v = rng.standard_normal(n)
    return v + 1j * rng.standard_normal(n) if cplx else v


def _rng(tag, cplx, n):
    return np.random.default_rng([sum(map(ord, tag)), int(cplx), n])


def _report(entry, cplx, n, ratio):
    print("CONFORMANCE %s %s n=%d max_err_over_bound=%.4f" % (entry, 'complex' if cplx else 'real', n, ratio))


def _ratio(err, lim):
    err, lim = np.atleast_1d(np.asarray(err, LD)), np.atleast_1d(np.asarray(lim, LD))
    assert np.all(err <= lim), "worst err / bound = %.3g" % float(np.max(err / np.maximum(lim, np.finfo(LD).tiny)))
    nz = lim > 0
    return float(np.max(err[nz] / lim[nz])) if nz.any() else 0.0


def _err(got, re, im):
    gr, gi = kref.split(got)
    return np.abs(gr - re), np.abs(gi - im)


def _red_out():
    out, scr = dev.reduction_buffers()
    return out, scr


# ---- runners: upload, call, download ------------------------------------------------------------------------------------------

def run_dot(x, y, do_conj, L=None):
    L = L if L is not None else dev.lib()
    cplx = np.iscomplexobj(x)
    xd, yd = dev.to_device(x), dev.to_device(y)
    out, scr = _red_out()
    res = []
    for _ in range(2):
        dev.check(L.tpa_fill_zero(out.data_ptr(), 16, dev.stream()), "fill_zero")
        dev.check(L.tpa_dot(int(cplx), len(x), xd.data_ptr(), yd.data_ptr(), do_conj, out.data_ptr(), scr.data_ptr(), dev.stream()), "dot")
        res.append(dev.to_host(out)[:2].copy())
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_dot is not deterministic"
    return res[0]


def check_dot(x, y, do_conj, got):
    """-> max err / bound; |err| <= (L + 2) EPS sum |x_i y_i| per component."""
    cplx = np.iscomplexobj(x)
    re, im, mr, mi = kref.dot(x, y, do_conj and cplx)
    L = chain_length(len(x), products=2 if cplx else 1)
    r = _ratio([abs(LD(got[0]) - re), abs(LD(got[1]) - im)], [(L + 2) * EPS * mr, (L + 2) * EPS * mi])
    if not cplx:
        assert got[1] == 0
    return r


# ---- tests ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize("do_conj", [0, 1])
def test_dot(backend, do_conj, cplx, n):
    rng = _rng('dot', cplx, n)
    x, y = _vec(rng, n, cplx), _vec(rng, n, cplx)
    _report("tpa_dot(do_conj=%d)" % do_conj, cplx, n, check_dot(x, y, do_conj, run_dot(x, y, do_conj)))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_nrm2sq(backend, cplx, n):
    L = dev.lib()
    x = _vec(_rng('nrm', cplx, n), n, cplx)
    xd = dev.to_device(x)
    out, scr = _red_out()
    res = []
    for _ in range(2):
        dev.check(L.tpa_nrm2sq(int(cplx), n, xd.data_ptr(), out.data_ptr(), scr.data_ptr(), dev.stream()), "nrm2sq")
        res.append(dev.to_host(out)[:2].copy())
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_nrm2sq is not deterministic"
    ref = kref.nrm2sq(x)
    Lc = chain_length(2 * n if cplx else n)          # complex: the flat real pass over 2 n doubles
    assert res[0][1] == 0
    _report("tpa_nrm2sq", cplx, n, _ratio(abs(LD(res[0][0]) - ref), (Lc + 2) * EPS * ref))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_axpy_scal(backend, cplx, n):
    L = dev.lib()
    rng = _rng('axpy', cplx, n)
    x, y = _vec(rng, n, cplx), _vec(rng, n, cplx)
    alpha = complex(0.37, -1.21) if cplx else -1.21
    R = 2 if cplx else 1          # complex axpy: up to 4 roundings of a term; real: product and sum
    xd, yd = dev.to_device(x), dev.to_device(y)
    dev.check(L.tpa_axpy(int(cplx), n, float(np.real(alpha)), float(np.imag(alpha)), xd.data_ptr(), yd.data_ptr(), dev.stream()), "axpy")
    re, im, mr, mi = kref.axpy(alpha, x, y)
    er, ei = _err(dev.to_host(yd), re, im)
    _report("tpa_axpy", cplx, n, max(_ratio(er, R * EPS * (1 + R * EPS) * mr), _ratio(ei, R * EPS * (1 + R * EPS) * mi)))
    assert np.array_equal(kref.bits(dev.to_host(xd)), kref.bits(x))
    dev.check(L.tpa_scal(int(cplx), n, float(np.real(alpha)), float(np.imag(alpha)), xd.data_ptr(), dev.stream()), "scal")
    re, im, mr, mi = kref.scal(alpha, x)
    er, ei = _err(dev.to_host(xd), re, im)
    _report("tpa_scal", cplx, n, max(_ratio(er, EPS * (1 + EPS) * mr), _ratio(ei, EPS * (1 + EPS) * mi)))      # product, difference: gamma_2


def _norm_bound(re, im, d_re, d_im, n_items, products):
    """| sum |w + d|^2 - sum |w|^2 | <= sum (2 |w_i| d_i + d_i^2) for elementwise errors d, plus the reduction of the squares."""
    prop = np.sum(2 * np.abs(re) * d_re + d_re**2) + np.sum(2 * np.abs(im) * d_im + d_im**2)
    return prop + (chain_length(n_items, products=products) + 2) * EPS * np.sum(re * re + im * im)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize("with_v0", [False, True], ids=['no_v0', 'v0'])
def test_lanczos_update(backend, with_v0, cplx, n):
    L = dev.lib()
    rng = _rng('lzu', cplx, n)
    w, v1, v0 = _vec(rng, n, cplx), _vec(rng, n, cplx), (_vec(rng, n, cplx) if with_v0 else None)
    alpha, beta = (complex(0.83, 0.4), complex(-0.6, 0.2)) if cplx else (0.83, -0.6)
    wd, v1d = dev.to_device(w), dev.to_device(v1)
    v0d = dev.to_device(v0) if with_v0 else None
    out, scr = _red_out()
    res = []
    for _ in range(2):
        wd.copy_(dev.to_device(w))
        dev.check(L.tpa_lanczos_update(int(cplx), n, wd.data_ptr(), float(np.real(alpha)), float(np.imag(alpha)), v1d.data_ptr(),
                                       float(np.real(beta)), float(np.imag(beta)), v0d.data_ptr() if with_v0 else None, out.data_ptr(),
                                       scr.data_ptr(), dev.stream()), "lanczos_update")
        res.append((dev.to_host(wd).copy(), dev.to_host(out)[:2].copy()))
    assert np.array_equal(kref.bits(res[0][0]), kref.bits(res[1][0])) and np.array_equal(kref.bits(res[0][1]), kref.bits(res[1][1]))
    ref = kref.lanczos_update(w, alpha, v1, beta, v0)
    d_re, d_im = 2 * EPS * (1 + 2 * EPS) * ref['mag_re'], 2 * EPS * (1 + 2 * EPS) * ref['mag_im']          # <= 4 roundings of a term: gamma_4
    er, ei = _err(res[0][0], ref['re'], ref['im'])
    r = max(_ratio(er, d_re), _ratio(ei, d_im))
    r = max(r, _ratio(abs(LD(res[0][1][0]) - ref['nrm2sq']), _norm_bound(ref['re'], ref['im'], d_re, d_im, n, 2 if cplx else 1)))
    _report("tpa_lanczos_update(%s)" % ('v0' if with_v0 else 'no_v0'), cplx, n, r)


def run_lanczos_step(L, cplx, n, wd, v1d, v0d, bsq_prev_ptr, ab, ab_index, scr):
    dev.check(L.tpa_lanczos_step(int(cplx), n, wd.data_ptr(), v1d.data_ptr(), v0d.data_ptr() if v0d is not None else None, bsq_prev_ptr,
                                 ab.data_ptr() + 8 * ab_index, scr.data_ptr(), dev.stream()), "lanczos_step")


def check_lanczos_step(cplx, w, v1, v0, bsq_prev, got_w, got_ab):
    """alpha: the reduction bound d_alpha.  u = w - alpha v1 - beta v0 on the device uses the device's alpha and beta = sqrt(bsq_prev)
    (correctly rounded): d_u = d_alpha |v1| + 2 EPS (|w| + |alpha v1| + |beta v0|) per component (<= 3 roundings of a term plus the
    rounding of beta: 4 u).  bsq: _norm_bound.  w_out = u / sqrt(bsq): d_u / beta + |w_out| (d_bsq / (2 bsq) + 2 EPS) (square root,
    reciprocal, product).  First order in EPS."""
    n = len(w)
    ref = kref.lanczos_step(w, v1, v0, bsq_prev)
    prod = 2 if cplx else 1
    d_alpha = (chain_length(n, products=prod) + 2) * EPS * ref['alpha_mag']
    ratios = [_ratio(abs(LD(got_ab[0]) - ref['alpha']), d_alpha)]
    wr, wi = kref.split(w)
    pr, pi = kref.split(v1)
    qr, qi = kref.split(v0) if v0 is not None else (0 * wr, 0 * wi)
    a, b = abs(ref['alpha']), ref['beta_prev']
    d_re = d_alpha * np.abs(pr) + 2 * EPS * (np.abs(wr) + a * np.abs(pr) + b * np.abs(qr))
    d_im = d_alpha * np.abs(pi) + 2 * EPS * (np.abs(wi) + a * np.abs(pi) + b * np.abs(qi))
    d_bsq = _norm_bound(ref['u_re'], ref['u_im'], d_re, d_im, n, prod)
    ratios.append(_ratio(abs(LD(got_ab[1]) - ref['bsq']), d_bsq))
    f = 1 / np.sqrt(ref['bsq'])
    rel = d_bsq / (2 * ref['bsq']) + 2 * EPS
    er, ei = _err(got_w, ref['out_re'], ref['out_im'])
    ratios.append(_ratio(er, d_re * f + np.abs(ref['out_re']) * rel))
    ratios.append(_ratio(ei, d_im * f + np.abs(ref['out_im']) * rel))
    return max(ratios)


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize("kind", ['no_v0', 'v0', 'cancellation'])
def test_lanczos_step(backend, kind, cplx, n):
    """One step: alpha, bsq and the normalised w, without and with v0 / bsq_prev; 'cancellation': <w|v1> is 1e-9 of sum |w_i v1_i|."""
    L = dev.lib()
    rng = _rng('lzs' + kind, cplx, n)
    w, v1 = _vec(rng, n, cplx), _vec(rng, n, cplx)
    v0 = _vec(rng, n, cplx) if kind != 'no_v0' else None
    if kind == 'cancellation' and n > 1:
        w = w - (np.vdot(v1, w) / np.vdot(v1, v1)) * v1 + 1e-9 * v1
    bsq_prev = 0.7310585786300049
    wd, v1d = dev.to_device(w), dev.to_device(v1)
    v0d = dev.to_device(v0) if v0 is not None else None
    out, scr = _red_out()
    res = []
    for _ in range(2):
        ab = dev.to_device(np.array([np.nan, np.nan, bsq_prev, np.nan]))
        wd.copy_(dev.to_device(w))
        run_lanczos_step(L, cplx, n, wd, v1d, v0d, ab.data_ptr() + 16 if v0 is not None else None, ab, 0, scr)
        res.append((dev.to_host(wd).copy(), dev.to_host(ab).copy()))
    assert np.array_equal(kref.bits(res[0][0]), kref.bits(res[1][0])) and np.array_equal(kref.bits(res[0][1]), kref.bits(res[1][1]))
    got_w, got_ab = res[0]
    assert got_ab[2] == bsq_prev and np.isnan(got_ab[3])
    _report("tpa_lanczos_step(%s)" % kind, cplx, n, check_lanczos_step(cplx, w, v1, v0, bsq_prev, got_w, got_ab))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_lanczos_step_chained(backend, cplx, n):
    """Two steps as the native Lanczos loop chains them: step 2 gets ``&ab_out[1]`` of step 1 as ``bsq_prev``, step 1's normalised w as
    v1 and step 1's v1 as v0.  The reference of step 2 starts from what the device left after step 1."""
    L = dev.lib()
    rng = _rng('lzc', cplx, n)
    w1, v1, w2 = _vec(rng, n, cplx), _vec(rng, n, cplx), _vec(rng, n, cplx)
    w1d, v1d, w2d = dev.to_device(w1), dev.to_device(v1), dev.to_device(w2)
    out, scr = _red_out()
    ab = dev.to_device(np.full(4, np.nan))
    run_lanczos_step(L, cplx, n, w1d, v1d, None, None, ab, 0, scr)
    run_lanczos_step(L, cplx, n, w2d, w1d, v1d, ab.data_ptr() + 8, ab, 2, scr)
    ab_h, w1_h, w2_h = dev.to_host(ab), dev.to_host(w1d), dev.to_host(w2d)
    r1 = check_lanczos_step(cplx, w1, v1, None, None, w1_h, ab_h[0:2])
    r2 = check_lanczos_step(cplx, w2, w1_h, v1, ab_h[1], w2_h, ab_h[2:4])
    _report("tpa_lanczos_step(chained)", cplx, n, max(r1, r2))


@pytest.mark.parametrize("n,N", [(n, 4) for n in LENGTHS] + [(257, 1), (257, 64)])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_krylov_combine(backend, cplx, n, N):
    """out_i = sum_k c_k V_k[i] as a chain of N fused multiply-adds (the emulation: N products and N sums): (N + 2) EPS mag_i.  The norm
    |out| inherits the elementwise bounds e, | |x + e| - |x| | <= |e|_2, plus the reduction of the squares over the flat doubles
    (P = 4 per thread) and the square root: ((L + 2) / 2 + 1) EPS |out|."""
    L = dev.lib()
    rng = _rng('kry', cplx, n + N)
    V = np.stack([_vec(rng, n, cplx) for _ in range(N)])
    coeff = np.ascontiguousarray(rng.standard_normal(N))
    Vd = dev.to_device(V.reshape(-1))
    od = dev.to_device(np.full(n, np.nan, dtype=V.dtype))
    out, scr = _red_out()
    res = []
    for _ in range(2):
        nrm = np.full(1, np.nan)
        dev.check(L.tpa_krylov_combine(int(cplx), n, Vd.data_ptr(), N, coeff.ctypes.data, od.data_ptr(), out.data_ptr(), scr.data_ptr(),
                                       nrm.ctypes.data, dev.stream()), "krylov_combine")
        res.append((dev.to_host(od).copy(), nrm.copy()))
    assert np.array_equal(kref.bits(res[0][0]), kref.bits(res[1][0])) and np.array_equal(kref.bits(res[0][1]), kref.bits(res[1][1]))
    ref = kref.krylov_combine(V, coeff)
    d_re, d_im = (N + 2) * EPS * ref['mag_re'], (N + 2) * EPS * ref['mag_im']
    er, ei = _err(res[0][0], ref['re'], ref['im'])
    r = max(_ratio(er, d_re), _ratio(ei, d_im))
    Lc = chain_length(2 * n if cplx else n, per_thread=4)
    lim = np.sqrt(np.sum(d_re**2) + np.sum(d_im**2)) + ((Lc + 2) / 2 + 1) * EPS * ref['norm']
    r = max(r, _ratio(abs(LD(res[0][1][0]) - ref['norm']), lim))
    _report("tpa_krylov_combine(N=%d)" % N, cplx, n, r)


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_n_zero(backend, cplx):
    """n = 0: nothing is read or written through the vector pointers; the reductions still post their (zero) results."""
    L = dev.lib()
    code = int(cplx)
    x = _vec(np.random.default_rng(1), 4, cplx)
    xd, yd = dev.to_device(x), dev.to_device(x)
    out, scr = _red_out()
    st = dev.stream()

    def poison():
        out.copy_(dev.to_device(np.full(4, np.nan)))

    def unchanged():
        assert np.array_equal(kref.bits(dev.to_host(xd)), kref.bits(x)) and np.array_equal(kref.bits(dev.to_host(yd)), kref.bits(x))
    assert L.tpa_axpy(code, 0, 2., 0., xd.data_ptr(), yd.data_ptr(), st) == 0
    assert L.tpa_scal(code, 0, 2., 0., xd.data_ptr(), st) == 0
    unchanged()
    for do_conj in (0, 1):
        poison()
        assert L.tpa_dot(code, 0, xd.data_ptr(), yd.data_ptr(), do_conj, out.data_ptr(), scr.data_ptr(), st) == 0
        assert dev.to_host(out)[:2].tolist() == [0., 0.]
    poison()
    assert L.tpa_nrm2sq(code, 0, xd.data_ptr(), out.data_ptr(), scr.data_ptr(), st) == 0
    assert dev.to_host(out)[:2].tolist() == [0., 0.]
    poison()
    assert L.tpa_lanczos_update(code, 0, yd.data_ptr(), 2., 0., xd.data_ptr(), 3., 0., xd.data_ptr(), out.data_ptr(), scr.data_ptr(), st) == 0
    assert dev.to_host(out)[:2].tolist() == [0., 0.]
    ab = dev.to_device(np.array([np.nan, np.nan, 0.5, np.nan]))
    assert L.tpa_lanczos_step(code, 0, yd.data_ptr(), xd.data_ptr(), xd.data_ptr(), ab.data_ptr() + 16, ab.data_ptr(), scr.data_ptr(), st) == 0
    got = dev.to_host(ab)
    assert got[:3].tolist() == [0., 0., 0.5] and np.isnan(got[3])
    unchanged()
    coeff, nrm = np.ones(2), np.full(1, np.nan)
    assert L.tpa_krylov_combine(code, 0, xd.data_ptr(), 2, coeff.ctypes.data, yd.data_ptr(), out.data_ptr(), scr.data_ptr(),
                                nrm.ctypes.data, st) == _lib.E_BADARG
    assert np.isnan(nrm[0])
    unchanged()
