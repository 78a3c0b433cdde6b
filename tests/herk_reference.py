"""Plain extended-precision statement of ``tpa_herk_chain`` (include/tenpy_amd.h, K1h), written from the table layouts of the header
alone: nothing here knows about tiles, triangles, workgroups or the numpy emulation of ``mock_mixer.py``.  Conventions as in
``kernel_reference.py``: host numpy tables and arenas as they are uploaded, ``np.longdouble`` arithmetic, complex data as (re, im).

A Hermitian task is stated as what it is mathematically -- the full m x m block of sum s a conj(a) -- and, with ``accumulate``, as
"the elements on and below the diagonal take C0, the elements above are their conjugates, the diagonal is real"."""
import numpy as np

from kernel_reference import LD, split

LINK_W, TASK_W = 12, 10


def herk_chain(cplx, tasks, links, A, B, wvec, C0):
    """-> dict(re, im, mag, ktot, mask, acc, herm, mirrors) over the flat C arena.  ``mag`` = sum |s| |a| |b| (+ |C0| when accumulating),
    ``ktot`` = sum of the k of the task's links; ``herm``: list of (c_off, m, ldc) of the Hermitian tasks; ``mirrors``: list of
    (c_off, m, n, ldc, mirror_off, mirror_ldc) of the general tasks with a mirror."""
    Ar, Ai = split(A)
    Br, Bi = split(B)
    Cr, Ci = split(C0)
    aA, aB, aC = np.abs(A).astype(LD), np.abs(B).astype(LD), np.abs(C0).astype(LD)
    W = None if wvec is None else np.asarray(wvec).astype(LD)
    re, im = Cr.copy(), Ci.copy()
    mag = np.zeros(len(C0), LD)
    ktot = np.zeros(len(C0), np.int64)
    mask, accm = np.zeros(len(C0), bool), np.zeros(len(C0), bool)
    herm_list, mirror_list = [], []
    links = np.asarray(links).reshape(-1, LINK_W)
    for c_off, m, n, ldc, lb, lc, acc, herm, m_off, m_ld in np.asarray(tasks).reshape(-1, TASK_W).tolist():
        sr, si, sm = np.zeros((m, n), LD), np.zeros((m, n), LD), np.zeros((m, n), LD)
        K = 0
        for a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off, w_len, w_inner, _, _ in links[lb:lb + lc].tolist():
            if k <= 0:
                continue
            ia = a_off + np.arange(m)[:, None] * a_rs + np.arange(k)[None, :] * a_ks
            ib = b_off + np.arange(n)[:, None] * b_rs + np.arange(k)[None, :] * b_ks
            s = np.ones(k, LD) if w_off < 0 else W[w_off + (np.arange(k) // w_inner) % w_len]
            ar, br = Ar[ia] * s, Br[ib].T
            sr += ar @ br
            if cplx:
                ai, bi = Ai[ia] * s, -Bi[ib].T          # conj(B)
                sr -= ai @ bi
                si += ar @ bi + ai @ br
            sm += (aA[ia] * np.abs(s)) @ aB[ib].T
            K += k
        ic = c_off + np.arange(m)[:, None] * ldc + np.arange(n)[None, :]
        if acc:
            low = np.tril(np.ones((m, n), bool)) if herm else np.ones((m, n), bool)
            cr, ci, ca = Cr[ic], Ci[ic], aC[ic]
            if herm:        # the elements on and below the diagonal are read; above: their conjugates; the diagonal is real
                cr = np.where(low, cr, cr.T)
                ci = np.where(low, ci, -ci.T)
                ca = np.where(low, ca, ca.T)
                ci[np.arange(m), np.arange(m)] = 0
            sr, si, sm = sr + cr, si + ci, sm + ca
        if herm:
            assert m == n
            si[np.arange(m), np.arange(m)] = 0
            herm_list.append((c_off, m, ldc))
        targets = [(ic.reshape(-1), sr.reshape(-1), si.reshape(-1), sm.reshape(-1))]
        if not herm and m_off >= 0:
            im_ = m_off + np.arange(n)[:, None] * m_ld + np.arange(m)[None, :]
            targets.append((im_.reshape(-1), sr.T.reshape(-1), -si.T.reshape(-1), sm.T.reshape(-1)))
            mirror_list.append((c_off, m, n, ldc, m_off, m_ld))
        for idx, r_, i_, m_ in targets:
            assert not mask[idx].any(), "two tasks address the same element of C"
            re[idx], im[idx], mag[idx], ktot[idx], mask[idx], accm[idx] = r_, i_, m_, K, True, bool(acc)
    return dict(re=re, im=im, mag=mag, ktot=ktot, mask=mask, acc=accm, herm=herm_list, mirrors=mirror_list)
