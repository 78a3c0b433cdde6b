"""Plain extended-precision statements of the device entry points of ``include/tenpy_amd.h``: one function per entry point, written
from the table layouts of the header alone (nothing here knows about tiles, workgroups or the numpy emulation of ``mock_device.py``).

Conventions: tables and arenas are HOST numpy arrays exactly as they are uploaded.  Arithmetic is ``np.longdouble``; complex data is
carried as two longdouble arrays (re, im).  Besides the result every function returns the componentwise MAGNITUDE SUM its rounding
error scales with (the sum of the absolute values of all the terms that are added into that component, e.g. ``sum |a| |b| (+ |C0|)``
for a GEMM), so that a test can state a bound of the form ``c * EPS * magnitude`` without an absolute constant.  Pure data movement
returns the expected array itself (compared bit for bit).  ``mask`` marks the elements of a destination arena that some job
addresses: everything else has to stay bit-unchanged."""
import numpy as np

LD = np.longdouble
MAXD = 6       # TPA_COPY_MAXDIM


def split(x):
    """(re, im) of an array as longdouble (im = 0 for real data)."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        return x.real.astype(LD), x.imag.astype(LD)
    return x.astype(LD), np.zeros(x.shape, LD)


def bits(x):
    """The bit patterns of a float64 / complex128 array (for bitwise comparisons; NaN compares equal to the same NaN)."""
    return np.ascontiguousarray(x).reshape(-1).view(np.uint64)


# ---- K1 ---------------------------------------------------------------------------------------------------------------------

def gemm_chain(cplx, tasks, links, A, B, C0):
    """C_t = [C_t +] sum_l A_l B_l per task.  Returns dict(re, im, mag, ktot, mask, acc) over the flat C arena: ``mag`` = sum |a| |b|
    (+ |C0| when accumulating; moduli for complex data), ``ktot`` = sum of the k of the task's links."""
    Ar, Ai = split(A)
    Br, Bi = split(B)
    Cr, Ci = split(C0)
    aA, aB, aC = np.abs(A).astype(LD), np.abs(B).astype(LD), np.abs(C0).astype(LD)
    re, im = Cr.copy(), Ci.copy()
    mag = np.zeros(len(C0), LD)
    ktot = np.zeros(len(C0), np.int64)
    mask, accm = np.zeros(len(C0), bool), np.zeros(len(C0), bool)
    for c_off, m, n, ldc, lb, lc, acc, _ in np.asarray(tasks).reshape(-1, 8).tolist():
        sr, si, sm = np.zeros((m, n), LD), np.zeros((m, n), LD), np.zeros((m, n), LD)
        K = 0
        for a_off, b_off, k, a_rs, a_ks, b_ks, b_ns, flags in np.asarray(links).reshape(-1, 8)[lb:lb + lc].tolist():
            if k <= 0:
                continue
            ia = a_off + np.arange(m)[:, None] * a_rs + np.arange(k)[None, :] * a_ks
            ib = b_off + np.arange(k)[:, None] * b_ks + np.arange(n)[None, :] * b_ns
            ar, br = Ar[ia], Br[ib]
            sr += ar @ br
            if cplx:
                ai = -Ai[ia] if flags & 1 else Ai[ia]
                bi = -Bi[ib] if flags & 2 else Bi[ib]
                sr -= ai @ bi
                si += ar @ bi + ai @ br
            sm += aA[ia] @ aB[ib]
            K += k
        ic = (c_off + np.arange(m)[:, None] * ldc + np.arange(n)[None, :]).reshape(-1)
        assert not mask[ic].any(), "two tasks address the same element of C"
        if acc:
            sr += Cr[ic].reshape(m, n)
            si += Ci[ic].reshape(m, n)
            sm += aC[ic].reshape(m, n)
        re[ic], im[ic], mag[ic], ktot[ic], mask[ic], accm[ic] = sr.reshape(-1), si.reshape(-1), sm.reshape(-1), K, True, bool(acc)
    return dict(re=re, im=im, mag=mag, ktot=ktot, mask=mask, acc=accm)


# ---- K2 - K4 ----------------------------------------------------------------------------------------------------------------

def dot(x, y, do_conj):
    """sum conj?(x_i) y_i -> (re, im, mag_re, mag_im)."""
    xr, xi = split(x)
    yr, yi = split(y)
    if do_conj:
        xi = -xi
    return (np.sum(xr * yr - xi * yi), np.sum(xr * yi + xi * yr),
            np.sum(np.abs(xr * yr) + np.abs(xi * yi)), np.sum(np.abs(xr * yi) + np.abs(xi * yr)))


def nrm2sq(x):
    """sum |x_i|^2 (its own magnitude sum)."""
    xr, xi = split(x)
    return np.sum(xr * xr + xi * xi)


def _cmul(ar, ai, xr, xi):
    """(a x) and the magnitude sums of its two components."""
    return ar * xr - ai * xi, ar * xi + ai * xr, np.abs(ar * xr) + np.abs(ai * xi), np.abs(ar * xi) + np.abs(ai * xr)


def axpy(alpha, x, y):
    """y + alpha x -> (re, im, mag_re, mag_im)."""
    xr, xi = split(x)
    yr, yi = split(y)
    pr, pi, mr, mi = _cmul(LD(np.real(alpha)), LD(np.imag(alpha)), xr, xi)
    return yr + pr, yi + pi, np.abs(yr) + mr, np.abs(yi) + mi


def scal(alpha, x):
    """alpha x -> (re, im, mag_re, mag_im)."""
    xr, xi = split(x)
    return _cmul(LD(np.real(alpha)), LD(np.imag(alpha)), xr, xi)


def lanczos_update(w, alpha, v1, beta, v0):
    """w - alpha v1 [- beta v0] -> dict(re, im, mag_re, mag_im, nrm2sq)."""
    r, i, mr, mi = axpy(-alpha, v1, w)
    if v0 is not None:
        pr, pi, qr, qi = _cmul(LD(np.real(beta)), LD(np.imag(beta)), *split(v0))
        r, i, mr, mi = r - pr, i - pi, mr + qr, mi + qi
    return dict(re=r, im=i, mag_re=mr, mag_im=mi, nrm2sq=np.sum(r * r + i * i))


def lanczos_step(w, v1, v0, bsq_prev):
    """alpha = Re <w|v1>; u = w - alpha v1 [- sqrt(bsq_prev) v0]; bsq = |u|^2; w_out = u / sqrt(bsq).
    -> dict(alpha, alpha_mag, beta_prev, u_re, u_im, bsq, out_re, out_im)."""
    wr, wi = split(w)
    pr, pi = split(v1)
    alpha = np.sum(wr * pr + wi * pi)
    alpha_mag = np.sum(np.abs(wr * pr) + np.abs(wi * pi))
    ur, ui = wr - alpha * pr, wi - alpha * pi
    beta = LD(0)
    if v0 is not None:
        beta = np.sqrt(LD(bsq_prev))
        qr, qi = split(v0)
        ur, ui = ur - beta * qr, ui - beta * qi
    bsq = np.sum(ur * ur + ui * ui)
    f = 1 / np.sqrt(bsq) if bsq > 0 else LD(1)
    return dict(alpha=alpha, alpha_mag=alpha_mag, beta_prev=beta, u_re=ur, u_im=ui, bsq=bsq, out_re=ur * f, out_im=ui * f)


def krylov_combine(V, coeff):
    """sum_k coeff[k] V[k] (V: N x n, real coefficients) -> dict(re, im, mag_re, mag_im, norm)."""
    Vr, Vi = split(V)
    c = np.asarray(coeff).astype(LD)[:, None]
    r, i = np.sum(c * Vr, axis=0), np.sum(c * Vi, axis=0)
    return dict(re=r, im=i, mag_re=np.sum(np.abs(c * Vr), axis=0), mag_im=np.sum(np.abs(c * Vi), axis=0),
                norm=np.sqrt(np.sum(r * r + i * i)))


# ---- data movement ----------------------------------------------------------------------------------------------------------

def _job_offsets(shape, strides, off):
    idx = np.indices(shape).reshape(len(shape), -1)
    return off + (idx * np.asarray(strides, np.int64)[:, None]).sum(axis=0)


def copy_batch(cplx, jobs, src, dst0):
    """-> (expected dst, mask).  jobs: int64[n][4 + 3 MAXD]; the last dim is the fastest loop index (no influence on the result)."""
    out, mask = dst0.copy(), np.zeros(len(dst0), bool)
    for j in np.asarray(jobs).reshape(-1, 4 + 3 * MAXD):
        nd = int(j[2])
        shape = [int(s) for s in j[4:4 + nd]]
        if nd == 0 or min(shape) <= 0:
            if nd == 0:      # the empty product: ONE element
                shape = []
            else:
                continue
        do = _job_offsets(shape, j[4 + MAXD:4 + MAXD + nd], j[0]) if nd else np.array([j[0]])
        so = _job_offsets(shape, j[4 + 2 * MAXD:4 + 2 * MAXD + nd], j[1]) if nd else np.array([j[1]])
        v = src[so]
        if cplx and (j[3] & 1):
            v = np.conj(v)
        assert not mask[do].any() and len(np.unique(do)) == len(do), "a destination element is written twice"
        out[do], mask[do] = v, True
    return out, mask


def lincomb_batch(cplx, jobs, terms, src, dst0):
    """-> dict(re, im, mag_re, mag_im, nterms, mask) over the flat dst arena."""
    sr, si = split(src)
    re, im = split(dst0)
    n = len(dst0)
    mr, mi, nt, mask = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, np.int64), np.zeros(n, bool)
    terms = np.asarray(terms).reshape(-1, 4)
    alphas = terms[:, 2:4].copy().view(np.float64)
    for d_off, rows, cols, d_ld, tb, tc, _, _ in np.asarray(jobs).reshape(-1, 8).tolist():
        if rows <= 0 or cols <= 0:
            continue
        do = (d_off + np.arange(rows)[:, None] * d_ld + np.arange(cols)[None, :]).reshape(-1)
        assert not mask[do].any()
        ar_, ai_, amr, ami = (np.zeros(rows * cols, LD) for _ in range(4))
        for t in range(tb, tb + tc):
            so = (int(terms[t, 0]) + np.arange(rows)[:, None] * int(terms[t, 1]) + np.arange(cols)[None, :]).reshape(-1)
            pr, pi, qr, qi = _cmul(LD(alphas[t, 0]), LD(alphas[t, 1]) if cplx else LD(0), sr[so], si[so])
            ar_, ai_, amr, ami = ar_ + pr, ai_ + pi, amr + qr, ami + qi
        re[do], im[do], mr[do], mi[do], nt[do], mask[do] = ar_, ai_, amr, ami, tc, True
    return dict(re=re, im=im, mag_re=mr, mag_im=mi, nterms=nt, mask=mask)


def scale_axis_batch(jobs, x0, s):
    """x[i, j, l] * s[s_off + j] -> dict(re, im, mag_re, mag_im, mask[, fp64]) over the flat arena (in place on the device).  A REAL s
    takes one fp64 product per component: ``fp64`` is that product (no second rounding through the longdouble value)."""
    xr, xi = split(x0)
    sr, si = split(s)
    re, im = xr.copy(), xi.copy()
    n = len(x0)
    mr, mi, mask = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, bool)
    fp64 = None if np.iscomplexobj(s) else np.array(x0, copy=True)
    for x_off, pre, ln, post, s_off, _ in np.asarray(jobs).reshape(-1, 6).tolist():
        if pre * ln * post <= 0:
            continue
        e = np.arange(pre * ln * post)
        j = s_off + (e // post) % ln
        assert not mask[x_off + e].any()
        re[x_off + e], im[x_off + e], mr[x_off + e], mi[x_off + e] = _cmul(sr[j], si[j], xr[x_off + e], xi[x_off + e])
        mask[x_off + e] = True
        if fp64 is not None:
            comp = fp64.view(np.float64).reshape(n, -1)          # (n, 1) real / (n, 2) complex components, in place
            comp[x_off + e] = comp[x_off + e] * np.asarray(s, np.float64)[j][:, None]
    return dict(re=re, im=im, mag_re=mr, mag_im=mi, mask=mask, fp64=fp64)


def gather_axis_batch(jobs, idx, src, dst0):
    """dst[i, j, l] = src[i, idx[idx_off + j], l] -> (expected dst, mask)."""
    out, mask = dst0.copy(), np.zeros(len(dst0), bool)
    for d_off, s_off, pre, ls, ld, post, i_off, _ in np.asarray(jobs).reshape(-1, 8).tolist():
        if pre * ld * post <= 0:
            continue
        i, j, l = np.indices((pre, ld, post)).reshape(3, -1)
        do = d_off + (i * ld + j) * post + l
        assert not mask[do].any()
        out[do], mask[do] = src[s_off + (i * ls + idx[i_off + j]) * post + l], True
    return out, mask


def axis_sqnorm_batch(jobs, rows, x, out0):
    """out[o_off + j] = sum_{i,l} |x[i, j, l]|^2 for the rows {job, j} with job >= 0 -> (values, mask, terms per lane)."""
    xr, xi = split(x)
    val, mask = out0.astype(LD), np.zeros(len(out0), bool)
    jobs = np.asarray(jobs).reshape(-1, 6)
    cnt = np.zeros(len(out0), np.int64)
    for jb, j in np.asarray(rows).reshape(-1, 2).tolist():
        if jb < 0:
            continue
        x_off, pre, ln, post, o_off, _ = jobs[jb].tolist()
        i, l = np.indices((pre, post)).reshape(2, -1)
        e = x_off + (i * ln + j) * post + l
        val[o_off + j], mask[o_off + j], cnt[o_off + j] = np.sum(xr[e]**2 + xi[e]**2), True, pre * post
    return val, mask, cnt


def tri_lower_batch(jobs, g0):
    """Strict lower triangle kept, zeros above, diagonal (Re G_ii - 1) / 2 (imaginary part 0).
    -> (expected arena with the fp64 value of the diagonal, mask, diagonal mask, extended-precision diagonal)."""
    out, mask, dmask = g0.copy(), np.zeros(len(g0), bool), np.zeros(len(g0), bool)
    diag = np.zeros(len(g0), LD)
    for g_off, n in np.asarray(jobs).reshape(-1, 2).tolist():
        if n <= 0:
            continue
        i, j = np.indices((n, n)).reshape(2, -1)
        e = g_off + i * n + j
        assert not mask[e].any()
        out[e[i < j]] = 0
        d = e[i == j]
        diag[d] = (g0[d].real.astype(LD) - 1) / 2
        out[d] = 0.5 * (g0[d].real - 1.0)
        mask[e], dmask[d] = True, True
    return out, mask, dmask, diag


def convert(from_cplx, to_cplx, src, conj):
    """astype / conjugation of a flat arena (c128 -> f64 keeps the real part; ``conj`` acts on c128 -> c128 only)."""
    if from_cplx and not to_cplx:
        return np.ascontiguousarray(src.real)
    if not from_cplx and to_cplx:
        return src.astype(np.complex128)
    return np.conj(src) if (from_cplx and conj) else src.copy()


def fill_zero(raw0, n_bytes):
    """The first n_bytes of a byte arena are zero, the rest is unchanged."""
    out = raw0.copy()
    out[:max(int(n_bytes), 0)] = 0
    return out
