"""Conformance of ``tpa_mpo_expand_batch`` (row o of a job = sum_t alpha_t * one row of a source slab, written ``dst_row_off_o`` elements
behind ``dst_off + i dst_ld``; the source of a row is ``src`` or ``src2``) with the extended-precision statement of the header, on the
numpy emulation (``mock``) and on the HIP kernel (``gpu``), real and complex, in the style of ``test_conformance_mpo_entry.py``.

Launch geometry (documented next to the kernel in csrc/tpa_copy.hip): that of ``tpa_mpo_entry_apply_batch``.  A thread owns one column
(i, item of j) of a job and walks the rows of the job; an ITEM is 16 bytes (one complex element, or two real elements of one row) when
src_base, src2_base and dst_base are 16-byte aligned and, for real data, post, dst_off, dst_ld and every dst_row_off, src_off and
src_ld of the job are even -- else one element (decided per job).  256 threads per workgroup, grid (min(512, ceil(max_job_cols /
(EPI 256))), n_jobs), grid-stride over the columns.  So the edges are: post even and odd, each of the six quantities as the only odd
one, each base 8 bytes off a 16-byte boundary, n_rows = 1 and 25, rows in a scattered order with gaps between them, rows of both
sources in one job, a row without terms, two jobs whose rows interleave in one block, pre = 0, and a job with more items than
512 * 256 threads.

Bound (derived; u = 2^-53), as for the sibling: a component of dst is one chain of n fused multiply-adds, so
|err| <= gamma_n sum_t |alpha_t| |x_t| with gamma_n = n u / (1 - n u) and n = term_count (real), 4 term_count (complex: the emulation
rounds the products and sums of a complex multiplication separately).  term_count = 0: exact zeros."""
import numpy as np
import pytest

import kernel_reference as kref
from expand_fixtures import xbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble
CAP = 512 * 256             # threads of the capped grid of one job


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one launch.  ``add_src(pre, m_in, post, sel=)`` -> index of a slab of source ``sel`` (slabs ``gap`` elements
    apart); ``region(n)`` -> offset of ``n`` free elements of dst; ``add_job(off, pre, post, dst_ld, rows)`` with
    rows = [(dst_row_off, sel, [(slab, c, alpha), ...]), ...]: the row is the sum of alpha * middle row c of slab (all of source sel)."""

    def __init__(self, cplx, seed, gap=3):
        self.cplx, self.gap = cplx, gap
        self.rng = np.random.default_rng(seed)
        self.slabs, self.src_len = [], [gap, gap]
        self.jobs, self.rows, self.terms, self.want = [], [], [], []
        self.dst_len = gap

    def add_src(self, pre, m_in, post, pad=0, sel=0, lead=0):
        """A slab (pre, m_in, post) of source ``sel`` whose rows i are ``m_in * post + pad`` elements apart, ``lead`` elements further on."""
        off = self.src_len[sel] + lead
        ld = m_in * post + pad
        data = _rand(self.rng, max(pre, 1) * ld, self.cplx)
        self.slabs.append((off, ld, pre, m_in, post, data, sel))
        self.src_len[sel] = off + len(data) + self.gap
        return len(self.slabs) - 1

    def region(self, n, lead=0):
        off = self.dst_len + lead
        self.dst_len = off + n + self.gap
        return off

    def add_job(self, off, pre, post, dst_ld, rows):
        row_begin = len(self.rows)
        for row_off, sel, terms in rows:
            self.rows.append([len(self.terms), len(terms), row_off, sel])
            for slab, c, alpha in terms:
                s_off, s_ld, s_pre, m_in, s_post, _, s_sel = self.slabs[slab]
                assert s_post == post and c < m_in and s_pre >= pre and s_sel == sel
                a = complex(alpha)
                self.terms.append([s_off + c * post, s_ld] + np.array([a.real, a.imag]).view(np.int64).tolist())
        self.jobs.append([off, pre, len(rows), post, row_begin, dst_ld, 0, 0])
        self.want.append((off, pre, post, dst_ld, rows))

    @staticmethod
    def dst_index(off, pre, post, dst_ld, rows):
        """Element index of (i, o, j) of a job."""
        row_off = np.array([r[0] for r in rows], dtype=np.int64).reshape(-1)
        return off + np.arange(pre)[:, None, None] * dst_ld + row_off[None, :, None] + np.arange(post)[None, None, :]

    def src_host(self, sel):
        dt = np.complex128 if self.cplx else np.float64
        src = np.full(self.src_len[sel], np.nan, dtype=dt)
        for off, ld, pre, m_in, post, data, s in self.slabs:
            if s == sel:
                src[off:off + len(data)] = data
        return src

    def reference(self, srcs):
        """Per job: (re, im, magnitude sums, chain lengths per row) in extended precision."""
        out = []
        for off, pre, post, _, rows in self.want:
            shape = (pre, len(rows), post)
            re, im, mr, mi = (np.zeros(shape, LD) for _ in range(4))
            nt = np.zeros(len(rows), dtype=np.int64)
            ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
            for o, (_, sel, terms) in enumerate(rows):
                nt[o] = len(terms)
                for slab, c, alpha in terms:
                    s_off, s_ld = self.slabs[slab][:2]
                    xr, xi = kref.split(srcs[sel][s_off + c * post + ii * s_ld + jj])
                    ar, ai = LD(complex(alpha).real), LD(complex(alpha).imag)
                    re[:, o] += ar * xr - ai * xi
                    im[:, o] += ar * xi + ai * xr
                    mr[:, o] += np.abs(ar * xr) + np.abs(ai * xi)
                    mi[:, o] += np.abs(ar * xi) + np.abs(ai * xr)
            out.append((re, im, mr, mi, nt))
        return out


def run_and_check(case, mis=None, tag='', null_src2=False):
    """One launch (twice: bit-identical) into a destination pre-filled with NaN at the listed elements and sentinels everywhere else;
    everything the header promises checked; -> worst err / bound."""
    L = dev.lib()
    cplx = case.cplx
    W = 2 if cplx else 1
    dt = np.complex128 if cplx else np.float64
    srcs = [case.src_host(0), case.src_host(1)]
    sb = [_Buf(_flat(srcs[0]), mis == 'src'), _Buf(_flat(srcs[1]), mis == 'src2')]
    fill = np.full(case.dst_len * W, SENTINEL)
    listed = np.zeros(case.dst_len, dtype=bool)
    for job in case.want:
        idx = Case.dst_index(*job).reshape(-1)
        assert not listed[idx].any() and len(np.unique(idx)) == len(idx), "the tables of the test list an element twice"
        listed[idx] = True
        for w in range(W):
            fill[W * idx + w] = np.nan
    db = _Buf(fill, mis == 'dst')
    jobs = np.array(case.jobs, dtype=np.int64).reshape(-1, 8)
    rows = np.array(case.rows if case.rows else [[0, 0, 0, 0]], dtype=np.int64).reshape(-1, 4)
    terms = np.array(case.terms if case.terms else [[0, 0, 0, 0]], dtype=np.int64).reshape(-1, 4)
    jd, rd, td = dev.to_device(jobs), dev.to_device(rows), dev.to_device(terms)
    max_cols = int(np.max(jobs[:, 1] * jobs[:, 3]))
    if null_src2:
        assert not np.any(rows[:, 3])
    res = []
    for _ in range(2):
        db.reset()
        dev.check(L.tpa_mpo_expand_batch(int(cplx), jd.data_ptr(), len(jobs), rd.data_ptr(), td.data_ptr(), max_cols, sb[0].ptr,
                                         None if null_src2 else sb[1].ptr, db.ptr, dev.stream()), "mpo_expand")
        res.append(db.get())
        for s in (0, 1):
            assert np.array_equal(kref.bits(sb[s].get()), kref.bits(_flat(srcs[s]))), "a source was written"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_mpo_expand_batch is not deterministic"
    got = res[0].view(dt) if cplx else res[0]
    worst = 0.
    for job, (re, im, mr, mi, nt) in zip(case.want, case.reference(srcs)):
        off, pre = job[0], job[1]
        block = got[Case.dst_index(*job)]
        assert not np.isnan(block).any(), "job at %d: an element was not written" % off
        gr, gi = kref.split(block)
        g = np.array([gamma((4 if cplx else 1) * k) for k in nt], dtype=LD)[None, :, None]
        lim_r, lim_i = g * mr, g * mi
        err_r, err_i = np.abs(gr - re), np.abs(gi - im)
        for o in np.nonzero(nt == 0)[0]:
            assert np.array_equal(kref.bits(_flat(np.ascontiguousarray(block[:, o]))), kref.bits(np.zeros(pre * job[2] * W))), "row without terms"
        ratio = float(max(np.max(err_r / np.maximum(lim_r, LD(1e-300)), initial=0.), np.max(err_i / np.maximum(lim_i, LD(1e-300)), initial=0.)))
        assert np.all(err_r <= lim_r) and np.all(err_i <= lim_i), "job at %d: worst err / bound = %.3g" % (off, ratio)
        worst = max(worst, ratio)
    untouched = np.repeat(~listed, W)
    assert np.array_equal(kref.bits(res[0][untouched]), kref.bits(np.full(int(untouched.sum()), SENTINEL))), "an element that is not listed was written"
    print("CONFORMANCE tpa_mpo_expand_batch(%s) %s jobs=%d rows=%d terms=%d max_cols=%d gap=%d%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(jobs), len(case.rows), len(case.terms), max_cols, case.gap,
             ' mis=' + mis if mis else '', worst))
    assert worst <= 1
    return worst


def _alpha(case):
    a = _rand(case.rng, 1, case.cplx)[0]
    return complex(a) if case.cplx else float(a)


def _terms(case, slabs, o, max_terms):
    nt = 1 + (o * 7 + 3) % max_terms
    return [(slabs[(o + t) % len(slabs)], (3 * o + 5 * t) % case.slabs[slabs[(o + t) % len(slabs)]][3], _alpha(case)) for t in range(nt)]


def _scattered(n_rows):
    """Positions 0 .. n_rows - 1 in an order that goes up and down."""
    pos = [(7 * o + 3) % n_rows for o in range(n_rows)] if n_rows % 7 else list(range(n_rows))[::-1]
    assert sorted(pos) == list(range(n_rows))
    return pos


def _scatter_job(case, pre, post, n_rows, pitch, rows_of, ld_extra=0, lead=0):
    """A job whose row o lies at ``_scattered(n_rows)[o] * pitch`` (pitch > post: a gap behind every row that must stay untouched) of a
    region with dst_ld = n_rows * pitch + ld_extra; ``rows_of(o)`` -> (sel, terms)."""
    assert pitch > post
    ld = n_rows * pitch + ld_extra
    off = case.region(max(pre, 1) * ld, lead=lead)
    pos = _scattered(n_rows)
    case.add_job(off, pre, post, ld, [(pos[o] * pitch,) + tuple(rows_of(o)) for o in range(n_rows)])


@pytest.mark.parametrize("n_rows", [1, 25])
@pytest.mark.parametrize("post", [64, 65, 1, 6])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(xbackend, cplx, post, n_rows):
    """post even and odd, n_rows = 1 and 25, pre = 1 and 3, rows in a scattered order with gaps between them, everything at even
    offsets (even post: the 16-byte form of real data) and at odd ones (its 8-byte form); up to 6 terms per row (the loads of four
    terms at a time and the remainder).  No row selects src2: it is passed as NULL."""
    for pre in (1, 3):
        for gap in (2, 3):
            case = Case(cplx, [1, int(cplx), post, n_rows, pre, gap], gap=gap)
            slabs = [case.add_src(pre, 7, post), case.add_src(pre, 4, post)]
            _scatter_job(case, pre, post, n_rows, post + gap, lambda o: (0, _terms(case, slabs, o, 6)), ld_extra=gap)
            run_and_check(case, tag='shape', null_src2=True)


@pytest.mark.parametrize("mis", ['src', 'src2', 'dst'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(xbackend, cplx, mis):
    """src_base / src2_base / dst_base one real element off a 16-byte boundary, with an even and an odd post; rows of both sources."""
    for post in (64, 65):
        case = Case(cplx, [2, int(cplx), post], gap=2)
        s0 = [case.add_src(3, 5, post), case.add_src(3, 2, post)]
        s1 = [case.add_src(3, 3, post, sel=1)]
        _scatter_job(case, 3, post, 4, post + 2, lambda o: (o % 2, _terms(case, s1 if o % 2 else s0, o, 3)))
        run_and_check(case, mis=mis, tag='mis')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_sources_empty_rows_and_interleaved_jobs(xbackend, cplx):
    """In one launch: a job mixing rows of src_sel 0 and 1 (the row of theta: one term with alpha = 1), a row with term_count = 0
    inside a job (zeros over the NaN fill), terms of one row with different src_ld, two jobs whose rows interleave in one block (the
    column slices of two wR' blocks), a job with pre = 0 and a job without any term."""
    for post, gap, pad in ((64, 2, 2), (64, 2, 1), (33, 3, 1)):     # (real data: 16-byte form; odd src_ld; odd post and offsets)
        case = Case(cplx, [3, int(cplx), post, pad], gap=gap)
        a, b, c = case.add_src(3, 5, post), case.add_src(3, 3, post, pad=pad), case.add_src(3, 2, post, pad=4)
        th = case.add_src(3, 2, post, sel=1)

        def mixed(o):
            if o == 1:
                return 1, [(th, 1, 1.)]
            if o == 2:
                return 0, []
            if o == 3:
                return 0, [(a, 1, _alpha(case)), (b, 2, _alpha(case)), (c, 0, _alpha(case)), (b, 0, _alpha(case)), (a, 4, _alpha(case))]
            return 0, _terms(case, [a, b, c], o, 4)
        _scatter_job(case, 3, post, 5, post + gap, mixed)
        # one block of 3 x (6 rows of 2 post + gap): job A writes the first post columns of every row, job B the second post
        pitch = 2 * post + gap
        ld = 6 * pitch
        off = case.region(3 * ld)
        pos = _scattered(6)
        case.add_job(off, 3, post, ld, [(pos[o] * pitch, 0, _terms(case, [a, b, c], o, 5)) for o in range(6)])
        case.add_job(off + post, 3, post, ld, [(pos[5 - o] * pitch, o % 2, _terms(case, [th] if o % 2 else [c, a], o, 2)) for o in range(6)])
        case.add_job(case.region(post), 0, post, post, [(0, 0, [(a, 0, 1.)])])
        _scatter_job(case, 2, post, 2, post + gap, lambda o: (0, []))
        run_and_check(case, tag='rows')


ODD = ['dst_row_off', 'dst_off', 'dst_ld', 'src_off', 'src_ld']


@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_a_single_odd_quantity(xbackend, cplx, odd):
    """A job whose ONLY odd quantity is one dst_row_off, dst_off, dst_ld, one slab's src_off or src_ld: everything else is even, so
    for real data that quantity alone sends the job to the 8-byte form."""
    case = Case(cplx, [6, int(cplx), ODD.index(odd)], gap=2)
    post, pre, n_rows, pitch = 64, 3, 5, 68
    a = case.add_src(pre, 4, post, pad=1 if odd == 'src_ld' else 0, lead=1 if odd == 'src_off' else 0)
    ld = n_rows * pitch + (1 if odd == 'dst_ld' else 0)
    off = case.region(pre * ld, lead=1 if odd == 'dst_off' else 0)
    pos = _scattered(n_rows)
    rows = [(pos[o] * pitch + (1 if odd == 'dst_row_off' and o == 2 else 0), 0, _terms(case, [a], o, 3)) for o in range(n_rows)]
    case.add_job(off, pre, post, ld, rows)
    (dst_off, _, _, post_j, _, dst_ld, _, _), = case.jobs
    odd_ones = [n for n, v in (('post', post_j), ('dst_off', dst_off), ('dst_ld', dst_ld)) if v % 2] + \
        [n for n, vs in (('dst_row_off', {r[2] for r in case.rows}), ('src_off', {t[0] for t in case.terms}),
                         ('src_ld', {t[1] for t in case.terms})) if any(v % 2 for v in vs)]
    assert odd_ones == [odd]
    run_and_check(case, tag='odd_' + odd)


def test_job_beyond_the_grid(xbackend):
    """One real job with pre = post = 520: 520 * 260 items of 16 bytes, more than the 512 * 256 threads of the capped grid, so the
    grid-stride loop runs.  Two rows, the second in front of the first."""
    assert 520 * 260 > CAP
    case = Case(False, [4], gap=2)
    a = case.add_src(520, 2, 520)
    ld = 2 * 522
    off = case.region(520 * ld)
    case.add_job(off, 520, 520, ld, [(522, 0, [(a, 1, 0.75), (a, 0, -1.5)]), (0, 0, [(a, 0, 0.5)])])
    run_and_check(case, tag='big')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(xbackend, cplx):
    """n_jobs = 0 and -1: 0; n_jobs = 65536 and dtype = 2: TPA_E_BADARG; nothing is written in any of them."""
    L = dev.lib()
    W = 2 if cplx else 1
    case = Case(cplx, [5], gap=2)
    a = case.add_src(3, 2, 64)
    case.add_job(case.region(3 * 128), 3, 64, 128, [(64, 0, [(a, 0, 1.)]), (0, 0, [(a, 1, 2.)])])
    sb = _Buf(_flat(case.src_host(0)))
    db = _Buf(np.full(case.dst_len * W, SENTINEL))
    jd, rd, td = (dev.to_device(np.array(t, dtype=np.int64)) for t in (case.jobs, case.rows, case.terms))
    args = lambda n_jobs: (int(cplx), jd.data_ptr(), n_jobs, rd.data_ptr(), td.data_ptr(), 3 * 64, sb.ptr, None, db.ptr, dev.stream())
    assert L.tpa_mpo_expand_batch(*args(0)) == 0
    assert L.tpa_mpo_expand_batch(*args(-1)) == 0
    assert L.tpa_mpo_expand_batch(*args(65536)) == _lib.E_BADARG
    assert L.tpa_mpo_expand_batch(2, *args(1)[1:]) == _lib.E_BADARG          # dtype
    assert np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))
    assert L.tpa_mpo_expand_batch(*args(1)) == 0                             # (the same arguments do run)
    assert not np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))


def test_symbol_is_exported():
    assert 'tpa_mpo_expand_batch' in _lib.exported_symbols()
