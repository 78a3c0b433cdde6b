"""Sensitivity of the conformance suite: the numpy emulation is wrapped with ONE deliberate defect at a time and the checkers of
tests/test_conformance_gemm.py, test_conformance_vec.py, test_conformance_copy.py, test_conformance_qr.py and test_conformance_eigh.py
have to reject every one
of them (and accept the unbroken emulation on the same cases).  Needs no GPU: this is the evidence that a subtly wrong kernel would not pass."""
import itertools

import numpy as np
import pytest

import conformance_gemm_cases as cg
import conformance_eigh_cases as ce
import conformance_qr_cases as cq
import mock_device
import test_conformance_copy as tc
import test_conformance_vec as tv
from tenpy_amd.linalg import _device as dev

GEMM_CASE_STEP = 3         # every third case of the pairwise design of one real and one complex instantiation


class Mutant:
    """The emulation with some entry points replaced."""

    def __init__(self, base, **entry_points):
        self.base = base
        self.__dict__.update(entry_points)

    def __getattr__(self, name):
        return getattr(self.base, name)


def _table(ptr, dtype, width):
    return mock_device.REG.view(ptr, dtype).reshape(-1, width).copy()


# ---- defects of tpa_gemm_chain: (code, cfg, tasks, links, tiles, n_tiles, A, B, C, stream) ----------------------------------

def _gemm_with_tables(edit):
    """A defect that is a change of the tables the kernel sees."""
    def make(base, case):
        def gemm(code, cfg, tasks_p, links_p, tiles_p, n_tiles, A_p, B_p, C_p, stream):
            tasks, links = _table(tasks_p, np.int64, 8), _table(links_p, np.int64, 8)
            edit(tasks, links)
            td, ld = dev.to_device(tasks), dev.to_device(links)
            return base.tpa_gemm_chain(code, cfg, td.data_ptr(), ld.data_ptr(), tiles_p, n_tiles, A_p, B_p, C_p, stream)
        return Mutant(base, tpa_gemm_chain=gemm)
    return make


def _gemm_with_output(edit):
    """A defect that shows in C after a correct product: edit(case, tasks, C before, C after [writable view])."""
    def make(base, case):
        def gemm(code, cfg, tasks_p, links_p, tiles_p, n_tiles, A_p, B_p, C_p, stream):
            dt = np.complex128 if code else np.float64
            C = mock_device.REG.view(C_p, dt)
            before = C.copy()
            rc = base.tpa_gemm_chain(code, cfg, tasks_p, links_p, tiles_p, n_tiles, A_p, B_p, C_p, stream)
            edit(case, _table(tasks_p, np.int64, 8), before, C)
            return rc
        return Mutant(base, tpa_gemm_chain=gemm)
    return make


def _conj_b_ignored(tasks, links):
    links[:, 7] &= ~2


def _last_k_dropped(tasks, links):
    links[:, 2] -= (links[:, 2] % 16 != 0) & (links[:, 2] > 0)


def _accumulate_ignored(tasks, links):
    tasks[:, 6] = 0


def _empty_middle_link_ends_chain(tasks, links):
    for t in tasks:
        ks = links[t[4]:t[4] + t[5], 2]
        nonempty = np.flatnonzero(ks > 0)
        if len(nonempty):
            stop = [i for i in np.flatnonzero(ks == 0) if i > nonempty[0]]
            if stop:
                t[5] = stop[0]


def _row_63_not_written(case, tasks, before, C):
    for c_off, m, n, ldc in tasks[:, :4]:
        if m >= 64:
            C[c_off + 63 * ldc:c_off + 63 * ldc + n] = before[c_off + 63 * ldc:c_off + 63 * ldc + n]


def _one_element_off_by_16_bounds(case, tasks, before, C):
    lim = np.where(cg.reference(case)['mask'], cg.bound(case), 0)
    i = int(np.argmax(lim))
    C[i] += 16 * float(lim[i])


def _write_into_ldc_padding(case, tasks, before, C):
    c_off, m, n, ldc = tasks[0, :4]
    C[c_off + (m - 1) * ldc + n] = 0.0


GEMM_DEFECTS = {
    'conj_b_ignored': _gemm_with_tables(_conj_b_ignored),
    'last_k_of_partial_k_tiles_dropped': _gemm_with_tables(_last_k_dropped),
    'last_row_of_a_64_row_tile_not_written': _gemm_with_output(_row_63_not_written),
    'accumulate_ignored': _gemm_with_tables(_accumulate_ignored),
    'empty_middle_link_ends_the_chain': _gemm_with_tables(_empty_middle_link_ends_chain),
    'one_element_off_by_16_bounds': _gemm_with_output(_one_element_off_by_16_bounds),
    'one_write_into_the_ldc_padding': _gemm_with_output(_write_into_ldc_padding),
}

_gemm_cases = {}


def gemm_cases():
    if not _gemm_cases:
        for inst in ('chain_64x64x1x2_real_cfg1', 'chain_64x32x2x1_complex_cfg1'):
            _gemm_cases[inst] = list(itertools.islice(cg.small_cases(inst), 0, None, GEMM_CASE_STEP))
    return [c for cases in _gemm_cases.values() for c in cases]


def _rejected(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _gemm_rejections(make, base):
    return sum(_rejected(lambda c: cg.check_case(c, cg.run_case(c, L=make(base, c))), c) for c in gemm_cases())


# ---- defects of the vector and copy entry points ----------------------------------------------------------------------------

def _dot_drops_last(base):
    return Mutant(base, tpa_dot=lambda code, n, x, y, cj, out, scr, st: base.tpa_dot(code, n - 1, x, y, cj, out, scr, st))


def _copy_conj_ignored(base):
    def call(code, jobs_p, n_jobs, max_elems, src_p, dst_p, stream):
        jobs = _table(jobs_p, np.int64, 4 + 3 * tc.MAXD)
        jobs[:, 3] = 0
        jd = dev.to_device(jobs)
        return base.tpa_copy_batch(code, jd.data_ptr(), n_jobs, max_elems, src_p, dst_p, stream)
    return Mutant(base, tpa_copy_batch=call)


def _gather_idx_off_ignored(base):
    """(Flat addressing like the kernel's: an index that belongs to another job may point beyond this job's source block.)"""
    def call(code, jobs_p, n_jobs, max_elems, idx_p, src_p, dst_p, stream):
        dt = np.complex128 if code else np.float64
        idx, src, dst = mock_device.REG.view(idx_p, np.int64), mock_device.REG.view(src_p, dt), mock_device.REG.view(dst_p, dt)
        for d_off, s_off, pre, ls, ld, post, i_off, _ in _table(jobs_p, np.int64, 8)[:n_jobs]:
            i, j, l = np.indices((pre, ld, post)).reshape(3, -1)
            dst[d_off + (i * ld + j) * post + l] = src[np.minimum(s_off + (i * ls + idx[0 + j]) * post + l, len(src) - 1)]
        return 0
    return Mutant(base, tpa_gather_axis_batch=call)


def _tri_diagonal_not_halved(base):
    def call(code, jobs_p, n_jobs, max_elems, g_p, stream):
        rc = base.tpa_tri_lower_batch(code, jobs_p, n_jobs, max_elems, g_p, stream)
        g = mock_device.REG.view(g_p, np.complex128 if code else np.float64)
        for g_off, n in _table(jobs_p, np.int64, 2)[:n_jobs]:
            g[g_off + np.arange(n) * (n + 1)] *= 2          # (G_ii - 1) instead of (G_ii - 1) / 2
        return rc
    return Mutant(base, tpa_tri_lower_batch=call)


def _vec_copy_probes():
    """name -> (make mutant, [probe(L) that raises AssertionError when the checker rejects the library L])"""
    rng = np.random.default_rng(12)
    probes = {}
    dots = [(tv._vec(rng, n, cplx), tv._vec(rng, n, cplx), cj) for n in (2, 65, 2049) for cplx in (False, True) for cj in (0, 1)]
    probes['tpa_dot_drops_its_last_element'] = (_dot_drops_last, [
        (lambda L, a=a: tv.check_dot(a[0], a[1], a[2], tv.run_dot(a[0], a[1], a[2], L=L))) for a in dots])
    copies = [tc.copy_case(np.random.default_rng([13, b]), True, batch) for b, batch in enumerate(('one_element', 'forty_jobs'))]
    copies[0].jobs[:, 3] = 1
    probes['copy_conjugation_flag_ignored'] = (_copy_conj_ignored, [
        (lambda L, c=c: tc.check_copy(c, tc.run_copy(c, L=L))) for c in copies])
    gathers = [tc.gather_case(np.random.default_rng([14, int(cplx)]), cplx, 'forty_jobs') for cplx in (False, True)]
    probes['gather_idx_off_ignored'] = (_gather_idx_off_ignored, [
        (lambda L, c=c: tc.check_gather(c, tc.run_gather(c, L=L))) for c in gathers])
    tris = [tc.tri_case(np.random.default_rng([15, int(cplx)]), cplx, [1, 5, 64]) for cplx in (False, True)]
    probes['tri_lower_diagonal_not_halved'] = (_tri_diagonal_not_halved, [
        (lambda L, c=c: tc.check_tri(c, tc.run_tri(c, L=L))) for c in tris])
    return probes


# ---- defects of tpa_qr_batch (code, jobs, n_jobs, A, Q, R, stream) and of tpa_svd_batch --------------------------------------

def _qr_blocks(code, jobs_p, n_jobs, a_p, q_p, r_p):
    """Writable views (A_b, Q_b, R_b, element behind Q_b) per job of a call of the emulation."""
    dt = np.complex128 if code else np.float64
    Q, R = mock_device.REG.view(q_p, dt), mock_device.REG.view(r_p, dt)
    out = []
    for a_off, m, n, q_off, r_off in mock_device._host(jobs_p, (n_jobs, 8))[:, :5].tolist():
        k = min(m, n)
        A = mock_device.REG.view(a_p + a_off * np.dtype(dt).itemsize, dt)
        A.flags.writeable = True
        out.append((A[:m * n].reshape(m, n), Q[q_off:q_off + m * k].reshape(m, k), R[r_off:r_off + k * n].reshape(k, n),
                    Q[q_off + m * k:q_off + m * k + 1]))
    return out


def _qr_with_output(edit, last_block=True):
    """A defect that shows in the arenas after a correct factorisation: edit(A_b, Q_b, R_b, behind Q_b) per block."""
    def make(base):
        def qr(code, jobs_p, n_jobs, a_p, q_p, r_p, stream):
            rc = base.tpa_qr_batch(code, jobs_p, n_jobs - (0 if last_block else 1), a_p, q_p, r_p, stream)
            for blk in _qr_blocks(code, jobs_p, n_jobs, a_p, q_p, r_p)[:None if last_block else -1]:
                edit(*blk)
            return rc
        return Mutant(base, tpa_qr_batch=qr)
    return make


def _r_lower_unwritten(a, q, r, behind):
    r[np.tril_indices(r.shape[0], -1, r.shape[1])] = cq._nan(r.dtype)      # (what the caller's uninitialised memory held)


def _write_behind_q(a, q, r, behind):
    behind[:] = 0


def _a_overwritten(a, q, r, behind):
    a[:r.shape[0]] = r


def _q_conjugated(a, q, r, behind):
    q[:] = q.conj()


def _sign_flipped(a, q, r, behind):
    q[:, 0], r[0] = -q[:, 0], -r[0]


def _r_column_perturbed(a, q, r, behind):
    j = r.shape[1] - 1
    r[0, j] += 1e-12 * np.linalg.norm(a[:, j])


def _q_column_perturbed(a, q, r, behind):
    q[0, 0] += 1e-13


def _qr_unsigned_offsets(base):
    """a_off taken as unsigned: a block in front of a_base is read from somewhere else (modelled: from unrelated memory)."""
    def qr(code, jobs_p, n_jobs, a_p, q_p, r_p, stream):
        jobs = mock_device._host(jobs_p, (n_jobs, 8)).copy()
        isz = 16 if code else 8
        keep = []
        for j in jobs:
            if j[0] < 0:
                keep.append(dev.to_device(np.random.default_rng(3).standard_normal(2 * j[1] * j[2] + 2)))
                j[0] = (keep[-1].data_ptr() + isz - 1 - a_p) // isz
        return base.tpa_qr_batch(code, jobs.ctypes.data, n_jobs, a_p, q_p, r_p, stream)
    return Mutant(base, tpa_qr_batch=qr)


def _svd_with_output(edit):
    def make(base):
        def svd(code, jobs_p, n_jobs, a_p, u_p, s_p, vh_p, *rest):
            rc = base.tpa_svd_batch(code, jobs_p, n_jobs, a_p, u_p, s_p, vh_p, *rest)
            _, m, n, _, s_off = mock_device._host(jobs_p, (n_jobs, 8))[0, :5].tolist()
            edit(mock_device.REG.view(s_p, np.float64)[s_off:s_off + min(m, n)])
            return rc
        return Mutant(base, tpa_svd_batch=svd)
    return make


def _s_zero_with_vectors(s):
    s[cq.SVD_RANK:] = 0          # the values beyond the rank are declared zero, their vectors stay


def _s_pair_swapped(s):
    s[[3, 4]] = s[[4, 3]]


QR_DEFECTS = {
    'qr_lower_triangle_of_r_unwritten': _qr_with_output(_r_lower_unwritten),
    'qr_one_element_written_behind_q': _qr_with_output(_write_behind_q),
    'qr_a_overwritten_with_r': _qr_with_output(_a_overwritten),
    'qr_a_off_taken_as_unsigned': _qr_unsigned_offsets,
    'qr_q_conjugated': _qr_with_output(_q_conjugated),
    'qr_sign_of_a_row_of_r_and_column_of_q_flipped': _qr_with_output(_sign_flipped),
    'qr_trailing_column_misses_a_reflector': _qr_with_output(_r_column_perturbed),
    'qr_column_of_q_perturbed': _qr_with_output(_q_column_perturbed),
    'qr_last_block_skipped': _qr_with_output(lambda *blk: None, last_block=False),
}
SVD_DEFECTS = {
    'svd_vector_left_where_s_is_zero': _svd_with_output(_s_zero_with_vectors),
    'svd_pair_of_s_swapped': _svd_with_output(_s_pair_swapped),
}
QR_PROBE_CASES = ('wy_k32_real', 'wy_k32_complex', 'negative_a_off_wy_real', 'negative_a_off_onewg_complex')
SVD_PROBE_CASES = ('qrp_64x8_real_500x48', 'qrp_256x4_complex_48x1000')


def _qr_probe_list():
    return [(lambda L, c=cq.qr_case(n): cq.check_qr(c, cq.run_qr(c, L=L))) for n in QR_PROBE_CASES]


def _svd_probe_list():
    return [(lambda L, c=cq.svd_case(n): cq.check_svd(c, cq.run_svd(c, L=L))) for n in SVD_PROBE_CASES]


def _qr_probes():
    probes = {name: (make, _qr_probe_list()) for name, make in QR_DEFECTS.items()}
    probes.update({name: (make, _svd_probe_list()) for name, make in SVD_DEFECTS.items()})
    return probes


# ---- defects of tpa_eigh_batch (code, jobs, n_jobs, A, W, V, work, work_bytes, max_sweeps, tol, sweeps, stream) and of
#      tpa_eigh_from_svd (code, jobs, n_jobs, U, S, VH, lam, err, stream) ---------------------------------------------------------

def _eigh_blocks(code, jobs_p, n_jobs, a_p, w_p, v_p):
    """Writable views (A_b, W_b, V_b, element behind V_b) per job of a call of the emulation."""
    dt = np.complex128 if code else np.float64
    A, W, V = mock_device.REG.view(a_p, dt), mock_device.REG.view(w_p, np.float64), mock_device.REG.view(v_p, dt)
    A.flags.writeable = True
    return [(A[a_off:a_off + n * n].reshape(n, n), W[w_off:w_off + n], V[v_off:v_off + n * n].reshape(n, n), V[v_off + n * n:v_off + n * n + 1])
            for a_off, n, w_off, v_off in mock_device._host(jobs_p, (n_jobs, 8))[:, :4].tolist()]


def _eigh_with_output(edit, last_block=True):
    """A defect that shows in the arenas after a correct decomposition: edit(A_b, W_b, V_b, behind V_b) per block."""
    def make(base):
        def eigh(code, jobs_p, n_jobs, a_p, w_p, v_p, *rest):
            rc = base.tpa_eigh_batch(code, jobs_p, n_jobs - (0 if last_block else 1), a_p, w_p, v_p, *rest)
            for blk in _eigh_blocks(code, jobs_p, n_jobs, a_p, w_p, v_p)[:None if last_block else -1]:
                edit(*blk)
            return rc
        return Mutant(base, tpa_eigh_batch=eigh)
    return make


def _upper_triangle_read(a, w, v, behind):
    try:
        w[:], v[:] = np.linalg.eigh(a, 'U')
    except np.linalg.LinAlgError:          # (LAPACK on NaN)
        w[:], v[:] = np.nan, np.nan


def _descending(a, w, v, behind):
    w[:], v[:] = w[::-1].copy(), v[:, ::-1].copy()


def _vectors_as_rows(a, w, v, behind):
    v[:] = v.T.copy()


def _vectors_conjugated(a, w, v, behind):
    v[:] = v.conj()


def _vectors_swapped(a, w, v, behind):
    if len(w) >= 2:
        v[:, [0, 1]] = v[:, [1, 0]]


def _eigenvalue_perturbed(a, w, v, behind):
    w[len(w) // 2] += 1e-12 * np.linalg.norm(ce.lower_hermitian(a))


def _vector_perturbed(a, w, v, behind):
    v[0, 0] += 1e-12


def _write_behind_v(a, w, v, behind):
    behind[:] = 0


def _eigh_a_overwritten(a, w, v, behind):
    a[0, 0] = w[0]


def _eigh_w_off_ignored(base):
    def eigh(code, jobs_p, n_jobs, *rest):
        jobs = mock_device._host(jobs_p, (n_jobs, 8)).copy()
        jobs[:, 2] = np.cumsum(jobs[:, 1]) - jobs[:, 1]
        return base.tpa_eigh_batch(code, jobs.ctypes.data, n_jobs, *rest)
    return Mutant(base, tpa_eigh_batch=eigh)


def _from_svd_with_output(edit):
    """edit(u_b, s_b, v_b (columns v_i), lam_b, err (the words of all jobs), job index, err before the call)."""
    def make(base):
        def from_svd(code, jobs_p, n_jobs, u_p, s_p, vh_p, lam_p, err_p, stream):
            dt = np.complex128 if code else np.float64
            R = mock_device.REG
            U, VH, S, lam, err = R.view(u_p, dt), R.view(vh_p, dt), R.view(s_p, np.float64), R.view(lam_p, np.float64), R.view(err_p, np.float64)
            before = err[:n_jobs].copy()
            rc = base.tpa_eigh_from_svd(code, jobs_p, n_jobs, u_p, s_p, vh_p, lam_p, err_p, stream)
            for j, (uo, n, so, vo, lo) in enumerate(mock_device._host(jobs_p, (n_jobs, 8))[:, :5].tolist()):
                edit(U[uo:uo + n * n].reshape(n, n), S[so:so + n], VH[vo:vo + n * n].reshape(n, n).conj().T, lam[lo:lo + n], err, j, before)
            return rc
        return Mutant(base, tpa_eigh_from_svd=from_svd)
    return make


def _sign_always_plus(u, s, v, lam, err, j, before):
    lam[:] = s


def _err_of_first_64(u, s, v, lam, err, j, before):
    with np.errstate(invalid='ignore'):
        e = (s * np.linalg.norm(v - u * np.sign(lam + (lam == 0))[None, :], axis=0))[:64]
    err[j] = np.max(np.where(np.isnan(e), 1e300, e))


def _err_not_cleared(u, s, v, lam, err, j, before):
    if before[j:j + 1].view(np.uint64)[0] > err[j:j + 1].view(np.uint64)[0]:      # (the maximum is taken on the bit patterns)
        err[j] = before[j]


def _from_svd_vh_not_conjugated(base):
    def from_svd(code, jobs_p, n_jobs, u_p, s_p, vh_p, *rest):
        keep = dev.to_device(mock_device.REG.view(vh_p, np.complex128 if code else np.float64).conj())
        return base.tpa_eigh_from_svd(code, jobs_p, n_jobs, u_p, s_p, keep.data_ptr(), *rest)
    return Mutant(base, tpa_eigh_from_svd=from_svd)


EIGH_DEFECTS = {
    'eigh_upper_triangle_read': _eigh_with_output(_upper_triangle_read),
    'eigh_eigenvalues_descending': _eigh_with_output(_descending),
    'eigh_vectors_as_rows': _eigh_with_output(_vectors_as_rows),
    'eigh_vectors_conjugated': _eigh_with_output(_vectors_conjugated),
    'eigh_two_vectors_swapped_without_their_values': _eigh_with_output(_vectors_swapped),
    'eigh_one_eigenvalue_off_by_1e-12': _eigh_with_output(_eigenvalue_perturbed),
    'eigh_one_vector_perturbed_by_1e-12': _eigh_with_output(_vector_perturbed),
    'eigh_w_off_ignored': _eigh_w_off_ignored,
    'eigh_one_element_written_behind_v': _eigh_with_output(_write_behind_v),
    'eigh_a_overwritten': _eigh_with_output(_eigh_a_overwritten),
    'eigh_last_block_skipped': _eigh_with_output(lambda *blk: None, last_block=False),
}
FROM_SVD_DEFECTS = {
    'from_svd_sign_always_plus': _from_svd_with_output(_sign_always_plus),
    'from_svd_err_over_the_first_64_vectors_only': _from_svd_with_output(_err_of_first_64),
    'from_svd_err_dev_not_cleared': _from_svd_with_output(_err_not_cleared),
    'from_svd_vh_not_conjugated': _from_svd_vh_not_conjugated,
}
EIGH_PROBE_CASES = ('small_b32', 'small_c')


def _eigh_probe_list():
    return [(lambda L, c=ce.eigh_case(n): ce.check_eigh(c, ce.run_eigh(c, L=L))) for n in EIGH_PROBE_CASES]


def _from_svd_probe_list():
    kinds = [(k, False) for k in ce.FROM_SVD_KINDS_REAL] + [(k, True) for k in ce.FROM_SVD_KINDS_COMPLEX]
    return [(lambda L, c=ce.from_svd_case(k, cplx): ce.check_from_svd(c, ce.run_from_svd(c, L=L))) for k, cplx in kinds]


def _eigh_probes():
    probes = {name: (make, _eigh_probe_list()) for name, make in EIGH_DEFECTS.items()}
    probes.update({name: (make, _from_svd_probe_list()) for name, make in FROM_SVD_DEFECTS.items()})
    return probes


DEFECTS = list(GEMM_DEFECTS) + ['tpa_dot_drops_its_last_element', 'copy_conjugation_flag_ignored', 'gather_idx_off_ignored',
                                'tri_lower_diagonal_not_halved'] + list(QR_DEFECTS) + list(SVD_DEFECTS) + list(EIGH_DEFECTS) + list(FROM_SVD_DEFECTS)


def test_defect_list_is_complete():
    assert len(DEFECTS) == 37 and set(DEFECTS) == (set(GEMM_DEFECTS) | set(_vec_copy_probes()) | set(QR_DEFECTS) | set(SVD_DEFECTS)
                                                   | set(EIGH_DEFECTS) | set(FROM_SVD_DEFECTS))
    assert len(EIGH_DEFECTS) == 11 and len(FROM_SVD_DEFECTS) == 4 and set(_eigh_probes()) == set(EIGH_DEFECTS) | set(FROM_SVD_DEFECTS)
    assert len(QR_DEFECTS) == 9 and len(SVD_DEFECTS) == 2 and set(_qr_probes()) == set(QR_DEFECTS) | set(SVD_DEFECTS)


def test_unbroken_emulation_is_accepted(monkeypatch):
    base = mock_device.install(monkeypatch)
    assert _gemm_rejections(lambda b, c: b, base) == 0
    for make, probes in _vec_copy_probes().values():
        for probe in probes:
            probe(base)
    for probe in _qr_probe_list() + _svd_probe_list() + _eigh_probe_list() + _from_svd_probe_list():
        probe(base)


@pytest.mark.parametrize("defect", DEFECTS)
def test_conformance_detects_mutations(monkeypatch, defect):
    base = mock_device.install(monkeypatch)
    if defect in GEMM_DEFECTS:
        n = _gemm_rejections(GEMM_DEFECTS[defect], base)
        print("MUTATION %s: rejected by %d of %d GEMM cases" % (defect, n, len(gemm_cases())))
    else:
        make, probes = (_qr_probes() if defect in QR_DEFECTS or defect in SVD_DEFECTS else
                        _eigh_probes() if defect in EIGH_DEFECTS or defect in FROM_SVD_DEFECTS else _vec_copy_probes())[defect]
        n = sum(_rejected(probe, make(base)) for probe in probes)
        print("MUTATION %s: rejected by %d of %d probes" % (defect, n, len(probes)))
    assert n >= 1, "the conformance checker accepts an emulation with the defect '%s'" % defect
