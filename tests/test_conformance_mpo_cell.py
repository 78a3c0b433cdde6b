"""Conformance of ``tpa_mpo_cell_apply_batch`` (the rows of a job = coeff (n_rows x n_src) times the job's distinct source rows, row o
written ``dst_row_off_o`` elements behind ``dst_off + i dst_ld``) with the extended-precision statement of the header, on the numpy
emulation (``mock``) and on the HIP kernel (``gpu``), real and complex, with the apparatus of ``test_conformance_mpo_expand.py``.

Launch geometry (documented next to the kernel in csrc/tpa_copy.hip): a thread owns one column (i, item of j) of a job, loads every
source item once and keeps R = 8, 16 or 32 accumulators (the smallest R >= max_rows); an ITEM is 16 bytes (one complex element, or two
real elements of one row) when src_base and dst_base are 16-byte aligned and, for real data, post, dst_off, dst_ld and every
dst_row_off, src_off and src_ld of the job are even -- else one element (decided per job).  256 threads per workgroup, grid
(min(512, ceil(max_job_cols / (EPI 256))), n_jobs), grid-stride over the columns; the loads of four sources are issued at a time.  So
the edges are: n_rows at, below and above the compiled sizes (1, 7, 8, 9, 16, 17, 32), n_src = 0, 1, 5 and 33, a coefficient matrix
with zero entries and a whole zero row, post even and odd, each of the six parity quantities as the only odd one, each base 8 bytes off
a 16-byte boundary, rows in a scattered order with gaps, two jobs whose rows interleave in one block, pre = 0, a job with more items
than 512 * 256 threads, two jobs sharing one source list (the split of a 40-row cell), and max_rows below a job's n_rows (the upper
rows are not written).

Bound (derived; u = 2^-53), as for the sibling: a component of dst is one chain of n fused multiply-adds, so
|err| <= gamma_n sum_k |c_k| |x_k| with gamma_n = n u / (1 - n u) and n = n_src (real), 4 n_src (complex: the emulation rounds the
products and sums of a complex multiplication separately).  n_src = 0: exact zeros.

Equality with ``tpa_mpo_expand_batch``: the same chain with the zero coefficients left out; fma(0, x, acc) = acc on finite data, so the
two results compare ``==`` (a signed zero may differ)."""
import numpy as np
import pytest

import kernel_reference as kref
from mpo_cell_fixtures import cbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble
CAP = 512 * 256             # threads of the capped grid of one job
MAXROWS = 32


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one launch.  ``add_src(pre, m_in, post)`` -> index of a source slab (slabs ``gap`` elements apart);
    ``region(n)`` -> offset of ``n`` free elements of dst; ``add_job(off, pre, post, dst_ld, row_offs, srcs, C)`` with
    srcs = [(slab, c), ...] (middle row c of slab) or the number of an earlier job whose source list is shared, and C the
    (n_rows, n_src) coefficient matrix."""

    def __init__(self, cplx, seed, gap=3):
        self.cplx, self.gap = cplx, gap
        self.rng = np.random.default_rng(seed)
        self.slabs, self.src_len = [], gap
        self.jobs, self.rows, self.srcs, self.coeff, self.want = [], [], [], [], []
        self.dst_len = gap

    def add_src(self, pre, m_in, post, pad=0, lead=0):
        """A slab (pre, m_in, post) whose rows i are ``m_in * post + pad`` elements apart, ``lead`` elements further on."""
        off = self.src_len + lead
        ld = m_in * post + pad
        data = _rand(self.rng, max(pre, 1) * ld, self.cplx)
        self.slabs.append((off, ld, pre, m_in, post, data))
        self.src_len = off + len(data) + self.gap
        return len(self.slabs) - 1

    def region(self, n, lead=0):
        off = self.dst_len + lead
        self.dst_len = off + n + self.gap
        return off

    def matrix(self, n_rows, n_src, zero_row=True):
        """Random coefficients, about a third of them exact zeros, row 1 all zeros (where there is one)."""
        C = _rand(self.rng, n_rows * n_src, self.cplx).reshape(n_rows, n_src)
        C[self.rng.random((n_rows, n_src)) < 0.3] = 0
        if zero_row and n_rows > 1:
            C[1] = 0
        return C

    def add_job(self, off, pre, post, dst_ld, row_offs, srcs, C):
        n_rows = len(row_offs)
        if isinstance(srcs, int):       # the source list of an earlier job
            src_begin, n_src, src_tab = self.jobs[srcs][6], self.jobs[srcs][7], self.want[srcs][5]
        else:
            src_begin, n_src, src_tab = len(self.srcs), len(srcs), []
            for slab, c in srcs:
                s_off, s_ld, s_pre, m_in, s_post, _ = self.slabs[slab]
                assert s_post == post and c < m_in and s_pre >= pre
                src_tab.append((s_off + c * post, s_ld))
            self.srcs += [list(s) for s in src_tab]
        C = np.asarray(C).reshape(n_rows, n_src)
        self.jobs.append([off, pre, n_rows, post, dst_ld, len(self.rows), src_begin, n_src, len(self.coeff), 0])
        self.rows += [[r, 0] for r in row_offs]
        self.coeff += C.T.reshape(-1).tolist()                    # coeff_off + k * n_rows + o
        self.want.append((off, pre, post, dst_ld, list(row_offs), src_tab, C))

    @staticmethod
    def dst_index(off, pre, post, dst_ld, row_offs):
        """Element index of (i, o, j) of a job."""
        row_off = np.array(row_offs, dtype=np.int64).reshape(-1)
        return off + np.arange(pre)[:, None, None] * dst_ld + row_off[None, :, None] + np.arange(post)[None, None, :]

    def src_host(self):
        src = np.full(self.src_len, np.nan, dtype=np.complex128 if self.cplx else np.float64)
        for off, ld, pre, m_in, post, data in self.slabs:
            src[off:off + len(data)] = data
        return src

    def tables(self):
        dt = np.complex128 if self.cplx else np.float64
        jobs = np.array(self.jobs, dtype=np.int64).reshape(-1, 10)
        rows = np.array(self.rows if self.rows else [[0, 0]], dtype=np.int64).reshape(-1, 2)
        srcs = np.array(self.srcs if self.srcs else [[0, 0]], dtype=np.int64).reshape(-1, 2)
        coeff = np.array(self.coeff if self.coeff else [0], dtype=dt)
        return jobs, rows, srcs, coeff

    def reference(self, src):
        """Per job: (re, im, magnitude sums) in extended precision."""
        out = []
        for off, pre, post, _, row_offs, src_tab, C in self.want:
            shape = (pre, len(row_offs), post)
            re, im, mr, mi = (np.zeros(shape, LD) for _ in range(4))
            ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
            for k, (s_off, s_ld) in enumerate(src_tab):
                xr, xi = kref.split(src[s_off + ii * s_ld + jj])
                for o in range(len(row_offs)):
                    ar, ai = LD(complex(C[o, k]).real), LD(complex(C[o, k]).imag)
                    re[:, o] += ar * xr - ai * xi
                    im[:, o] += ar * xi + ai * xr
                    mr[:, o] += np.abs(ar * xr) + np.abs(ai * xi)
                    mi[:, o] += np.abs(ar * xi) + np.abs(ai * xr)
            out.append((re, im, mr, mi))
        return out


def launch(case, max_rows, sb, db):
    jobs, rows, srcs, coeff = case.tables()
    keep = [dev.to_device(t) for t in (jobs, rows, srcs, _flat(coeff))]
    max_cols = int(np.max(jobs[:, 1] * jobs[:, 3]))
    dev.check(dev.lib().tpa_mpo_cell_apply_batch(int(case.cplx), keep[0].data_ptr(), len(jobs), keep[1].data_ptr(), keep[2].data_ptr(),
                                                 keep[3].data_ptr(), max_rows, max_cols, sb.ptr, db.ptr, dev.stream()), "mpo_cell")
    return keep


def run_and_check(case, mis=None, tag='', max_rows=None):
    """One launch (twice: bit-identical) into a destination pre-filled with NaN at the listed elements and sentinels everywhere else;
    everything the header promises checked; -> (worst err / bound, the destination)."""
    cplx = case.cplx
    W = 2 if cplx else 1
    dt = np.complex128 if cplx else np.float64
    src = case.src_host()
    sb = _Buf(_flat(src), mis == 'src')
    n_max = max(len(w[4]) for w in case.want)
    if max_rows is None:
        max_rows = n_max
    fill = np.full(case.dst_len * W, SENTINEL)
    listed = np.zeros(case.dst_len, dtype=bool)
    for off, pre, post, dst_ld, row_offs, _, _ in case.want:
        idx = Case.dst_index(off, pre, post, dst_ld, row_offs[:max_rows]).reshape(-1)     # rows o >= max_rows are not written
        assert not listed[idx].any() and len(np.unique(idx)) == len(idx), "the tables of the test list an element twice"
        listed[idx] = True
        for w in range(W):
            fill[W * idx + w] = np.nan
    db = _Buf(fill, mis == 'dst')
    res = []
    for _ in range(2):
        db.reset()
        keep = launch(case, max_rows, sb, db)
        res.append(db.get())
        del keep
        assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src))), "the source was written"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_mpo_cell_apply_batch is not deterministic"
    got = res[0].view(dt) if cplx else res[0]
    worst = 0.
    for (off, pre, post, dst_ld, row_offs, src_tab, C), (re, im, mr, mi) in zip(case.want, case.reference(src)):
        nw = min(len(row_offs), max_rows)
        block = got[Case.dst_index(off, pre, post, dst_ld, row_offs[:nw])]
        assert not np.isnan(block).any(), "job at %d: an element was not written" % off
        gr, gi = kref.split(block)
        g = gamma((4 if cplx else 1) * len(src_tab))
        lim_r, lim_i = g * mr[:, :nw], g * mi[:, :nw]
        err_r, err_i = np.abs(gr - re[:, :nw]), np.abs(gi - im[:, :nw])
        if not src_tab:
            assert np.array_equal(kref.bits(_flat(np.ascontiguousarray(block))), kref.bits(np.zeros(block.size * W))), "job without sources"
        ratio = float(max(np.max(err_r / np.maximum(lim_r, LD(1e-300)), initial=0.), np.max(err_i / np.maximum(lim_i, LD(1e-300)), initial=0.)))
        assert np.all(err_r <= lim_r) and np.all(err_i <= lim_i), "job at %d: worst err / bound = %.3g" % (off, ratio)
        worst = max(worst, ratio)
    untouched = np.repeat(~listed, W)
    assert np.array_equal(kref.bits(res[0][untouched]), kref.bits(np.full(int(untouched.sum()), SENTINEL))), "an element that is not listed was written"
    print("CONFORMANCE tpa_mpo_cell_apply_batch(%s) %s jobs=%d rows=%d srcs=%d max_rows=%d gap=%d%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(case.jobs), len(case.rows), len(case.srcs), max_rows, case.gap,
             ' mis=' + mis if mis else '', worst))
    assert worst <= 1
    return worst, got


def _scattered(n_rows):
    """Positions 0 .. n_rows - 1 in an order that goes up and down."""
    pos = [(7 * o + 3) % n_rows for o in range(n_rows)] if n_rows % 7 else list(range(n_rows))[::-1]
    assert sorted(pos) == list(range(n_rows))
    return pos


def _src_list(case, slabs, n_src):
    """n_src distinct (slab, middle row) pairs, going round the slabs."""
    all_rows = [(s, c) for c in range(max(case.slabs[s][3] for s in slabs)) for s in slabs if c < case.slabs[s][3]]
    assert n_src <= len(all_rows)
    return all_rows[:n_src]


def _scatter_job(case, pre, post, n_rows, pitch, srcs, C=None, ld_extra=0, lead=0):
    """A job whose row o lies at ``_scattered(n_rows)[o] * pitch`` (pitch > post: a gap behind every row that must stay untouched) of a
    region with dst_ld = n_rows * pitch + ld_extra."""
    assert pitch > post
    ld = n_rows * pitch + ld_extra
    off = case.region(max(pre, 1) * ld, lead=lead)
    n_src = case.jobs[srcs][7] if isinstance(srcs, int) else len(srcs)
    case.add_job(off, pre, post, ld, [p * pitch for p in _scattered(n_rows)], srcs, case.matrix(n_rows, n_src) if C is None else C)


@pytest.mark.parametrize("n_rows", [1, 7, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(cbackend, cplx, n_rows):
    """n_rows at and around the compiled accumulator counts, n_src = 0, 1, 5, 33 (none, the remainder loop alone, one group of four and
    the remainder, eight groups and the remainder), post even and odd, pre = 1 and 3, rows in a scattered order with gaps, everything at
    even offsets (even post: the 16-byte form of real data) and at odd ones (its 8-byte form); zero coefficients and a zero row."""
    for post, pre, gap in ((64, 3, 2), (65, 1, 3), (6, 3, 2), (1, 3, 3)):
        for n_src in (0, 1, 5, 33):
            case = Case(cplx, [1, int(cplx), post, n_rows, n_src], gap=gap)
            slabs = [case.add_src(pre, 20, post), case.add_src(pre, 14, post)]
            _scatter_job(case, pre, post, n_rows, post + gap, _src_list(case, slabs, n_src), ld_extra=gap)
            run_and_check(case, tag='shape')


@pytest.mark.parametrize("mis", ['src', 'dst'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(cbackend, cplx, mis):
    """src_base / dst_base one real element off a 16-byte boundary, with an even and an odd post."""
    for post in (64, 65):
        case = Case(cplx, [2, int(cplx), post], gap=2)
        slabs = [case.add_src(3, 5, post), case.add_src(3, 2, post)]
        _scatter_job(case, 3, post, 9, post + 2, _src_list(case, slabs, 6))
        run_and_check(case, mis=mis, tag='mis')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_interleaved_shared_and_empty_jobs(cbackend, cplx):
    """In one launch: two jobs whose rows interleave in one block (the column slices of two wR' blocks), sources of one job with
    different src_ld, a cell of 40 rows split into jobs of 32 and 8 rows over ONE source list, a job with pre = 0 and a job with
    n_src = 0 (zeros over the NaN fill)."""
    for post, gap, pad in ((64, 2, 2), (64, 2, 1), (33, 3, 1)):     # (real data: 16-byte form; odd src_ld; odd post and offsets)
        case = Case(cplx, [3, int(cplx), post, pad], gap=gap)
        a, b, c = case.add_src(3, 5, post), case.add_src(3, 3, post, pad=pad), case.add_src(3, 4, post, pad=4)
        # one block of 3 x (6 rows of 2 post + gap): job A writes the first post columns of every row, job B the second post
        pitch = 2 * post + gap
        ld = 6 * pitch
        off = case.region(3 * ld)
        pos = _scattered(6)
        case.add_job(off, 3, post, ld, [pos[o] * pitch for o in range(6)], _src_list(case, [a, b, c], 7), case.matrix(6, 7))
        case.add_job(off + post, 3, post, ld, [pos[5 - o] * pitch for o in range(6)], _src_list(case, [c, a], 3), case.matrix(6, 3))
        # 40 rows over the same 11 sources: rows 0..31 and 32..39 as two jobs, the second one naming the source list of the first
        pitch = post + gap
        ld = 40 * pitch
        off = case.region(3 * ld)
        pos = _scattered(40)
        C = case.matrix(40, 11)
        case.add_job(off, 3, post, ld, [pos[o] * pitch for o in range(32)], _src_list(case, [a, b, c], 11), C[:32])
        case.add_job(off, 3, post, ld, [pos[o] * pitch for o in range(32, 40)], len(case.jobs) - 1, C[32:])
        assert case.jobs[-1][6] == case.jobs[-2][6] and case.jobs[-1][8] != case.jobs[-2][8]
        case.add_job(case.region(post), 0, post, post, [0], [(a, 0)], [[1.]])
        _scatter_job(case, 2, post, 2, post + gap, [])
        run_and_check(case, tag='jobs')


ODD = ['post', 'dst_row_off', 'dst_off', 'dst_ld', 'src_off', 'src_ld']


@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_a_single_odd_quantity(cbackend, cplx, odd):
    """A job whose ONLY odd quantity is post, one dst_row_off, dst_off, dst_ld, one source's src_off or src_ld: everything else is
    even, so for real data that quantity alone sends the job to the 8-byte form."""
    case = Case(cplx, [6, int(cplx), ODD.index(odd)], gap=2)
    post, pre, n_rows, pitch = (65 if odd == 'post' else 64), 3, 5, 68
    # (odd post: middle rows 0 and 2 of a slab whose leading dimension 4 * 65 is even keep every src_off and src_ld even)
    a = case.add_src(pre, 4, post, pad=1 if odd == 'src_ld' else 0, lead=1 if odd == 'src_off' else 0)
    ld = n_rows * pitch + (1 if odd == 'dst_ld' else 0)
    off = case.region(pre * ld, lead=1 if odd == 'dst_off' else 0)
    pos = _scattered(n_rows)
    row_offs = [pos[o] * pitch + (1 if odd == 'dst_row_off' and o == 2 else 0) for o in range(n_rows)]
    case.add_job(off, pre, post, ld, row_offs, [(a, 0), (a, 2)], case.matrix(n_rows, 2))
    (dst_off, _, _, post_j, dst_ld, _, _, _, _, _), = case.jobs
    odd_ones = [n for n, v in (('post', post_j), ('dst_off', dst_off), ('dst_ld', dst_ld)) if v % 2] + \
        [n for n, vs in (('dst_row_off', {r[0] for r in case.rows}), ('src_off', {s[0] for s in case.srcs}),
                         ('src_ld', {s[1] for s in case.srcs})) if any(v % 2 for v in vs)]
    assert odd_ones == [odd]
    run_and_check(case, tag='odd_' + odd)


def test_job_beyond_the_grid(cbackend):
    """One real job with pre = post = 520: 520 * 260 items of 16 bytes, more than the 512 * 256 threads of the capped grid, so the
    grid-stride loop runs.  Two rows, the second in front of the first."""
    assert 520 * 260 > CAP
    case = Case(False, [4], gap=2)
    a = case.add_src(520, 2, 520)
    ld = 2 * 522
    off = case.region(520 * ld)
    case.add_job(off, 520, 520, ld, [522, 0], [(a, 1), (a, 0)], [[0.75, -1.5], [0., 0.5]])
    run_and_check(case, tag='big')


@pytest.mark.parametrize("max_rows", [8, 9, 16])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_max_rows_below_n_rows(cbackend, cplx, max_rows):
    """A job of 19 rows under max_rows = 8, 9 and 16 (8 and 16 accumulators): rows o < max_rows are written with their values, the
    upper rows keep their sentinels; a second job that respects the limit is written completely."""
    case = Case(cplx, [7, int(cplx), max_rows], gap=2)
    slabs = [case.add_src(3, 5, 64)]
    _scatter_job(case, 3, 64, 19, 66, _src_list(case, slabs, 5))
    _scatter_job(case, 3, 64, 6, 66, _src_list(case, slabs, 3))
    run_and_check(case, tag='max_rows', max_rows=max_rows)


@pytest.mark.parametrize("post", [64, 33])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_equals_expand_on_the_nonzeros(cbackend, cplx, post):
    """The same cells through ``tpa_mpo_expand_batch``, every row listing its nonzero coefficients in the order of the sources: the two
    results compare equal (==)."""
    W = 2 if cplx else 1
    case = Case(cplx, [8, int(cplx), post], gap=2)
    slabs = [case.add_src(3, 6, post), case.add_src(3, 5, post, pad=2)]
    _scatter_job(case, 3, post, 17, post + 2, _src_list(case, slabs, 9))
    _scatter_job(case, 2, post, 5, post + 2, _src_list(case, slabs, 4))
    _, got = run_and_check(case, tag='vs_expand')
    jobs, rows, terms = [], [], []
    for off, pre, post_j, dst_ld, row_offs, src_tab, C in case.want:
        jobs.append([off, pre, len(row_offs), post_j, len(rows), dst_ld, 0, 0])
        for o, r in enumerate(row_offs):
            nz = [k for k in range(len(src_tab)) if C[o, k] != 0]
            rows.append([len(terms), len(nz), r, 0])
            for k in nz:
                a = complex(C[o, k])
                terms.append(list(src_tab[k]) + np.array([a.real, a.imag]).view(np.int64).tolist())
    jobs, rows, terms = (np.array(t, dtype=np.int64) for t in (jobs, rows, terms))
    sb = _Buf(_flat(case.src_host()))
    db = _Buf(np.full(case.dst_len * W, SENTINEL))
    jd, rd, td = dev.to_device(jobs), dev.to_device(rows), dev.to_device(terms)
    dev.check(dev.lib().tpa_mpo_expand_batch(int(cplx), jd.data_ptr(), len(jobs), rd.data_ptr(), td.data_ptr(),
                                             int(np.max(jobs[:, 1] * jobs[:, 3])), sb.ptr, None, db.ptr, dev.stream()), "mpo_expand")
    exp = db.get()
    exp = exp.view(np.complex128) if cplx else exp
    assert np.all(np.isfinite(_flat(got)) | (_flat(got) == SENTINEL))
    assert np.array_equal(got, exp), "the cell route and the entry route differ"


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(cbackend, cplx):
    """n_jobs = 0 and -1: 0; n_jobs = 65536, dtype = 2, max_rows = 0 and 33: TPA_E_BADARG; nothing is written in any of them."""
    L = dev.lib()
    W = 2 if cplx else 1
    case = Case(cplx, [5], gap=2)
    a = case.add_src(3, 2, 64)
    case.add_job(case.region(3 * 128), 3, 64, 128, [64, 0], [(a, 0), (a, 1)], [[1., 0.], [0., 2.]])
    sb = _Buf(_flat(case.src_host()))
    db = _Buf(np.full(case.dst_len * W, SENTINEL))
    jobs, rows, srcs, coeff = case.tables()
    jd, rd, sd, cd = (dev.to_device(t) for t in (jobs, rows, srcs, _flat(coeff)))
    args = lambda n_jobs, max_rows=2, code=int(cplx): (code, jd.data_ptr(), n_jobs, rd.data_ptr(), sd.data_ptr(), cd.data_ptr(), max_rows,
                                                       3 * 64, sb.ptr, db.ptr, dev.stream())
    assert L.tpa_mpo_cell_apply_batch(*args(0)) == 0
    assert L.tpa_mpo_cell_apply_batch(*args(-1)) == 0
    assert L.tpa_mpo_cell_apply_batch(*args(65536)) == _lib.E_BADARG
    assert L.tpa_mpo_cell_apply_batch(*args(1, code=2)) == _lib.E_BADARG                # dtype
    assert L.tpa_mpo_cell_apply_batch(*args(1, max_rows=0)) == _lib.E_BADARG
    assert L.tpa_mpo_cell_apply_batch(*args(1, max_rows=MAXROWS + 1)) == _lib.E_BADARG
    assert L.tpa_mpo_cell_apply_batch(*args(0, max_rows=0)) == _lib.E_BADARG            # (max_rows is checked before n_jobs)
    assert np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))
    assert L.tpa_mpo_cell_apply_batch(*args(1, max_rows=MAXROWS)) == 0                  # (the same tables do run)
    assert not np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))
