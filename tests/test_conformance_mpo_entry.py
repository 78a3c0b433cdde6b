"""Conformance of ``tpa_mpo_entry_apply_batch`` (dst slab (pre, n_rows, post): row o = sum_t alpha_t * one middle row of a src slab)
with the extended-precision statement of the header, on the numpy emulation (``mock``) and on the HIP kernel (``gpu``), real and
complex, in the style of ``test_conformance_mpo_apply.py``.

Launch geometry (documented next to the kernel in csrc/tpa_copy.hip).  A thread owns one column (i, item of j) of a job and walks the
rows of the job; an ITEM is 16 bytes (one complex element, or two real elements of one row) when src_base and dst_base are 16-byte
aligned and, for real data, post, dst_off, dst_ld and every src_off and src_ld of the job are even -- else one element (decided per
job).  256 threads per workgroup, grid (min(512, ceil(max_job_cols / (EPI 256))), n_jobs) with EPI = 2 for real data on aligned bases,
grid-stride over the columns.  So the edges are: post even and odd, odd dst_off / src_off / src_ld, a base 8 bytes off a 16-byte
boundary, n_rows = 1 and 25, a row without terms inside a job, dst_ld > n_rows post with two jobs sharing a block, terms of one row
with different src_ld, a job with pre = 0, and a job with more items than 512 * 256 threads.

Bound (derived; u = 2^-53).  A component of dst is one chain of n fused multiply-adds, n = term_count (real) or 2 term_count (complex;
the emulation rounds the products and sums of a complex multiplication separately: at most term_count + 2 roundings per term), so
|err| <= gamma_n sum_t |alpha_t| |x_t| with gamma_n = n u / (1 - n u) and n = term_count (real), 4 term_count (complex).
term_count = 0: exact zeros."""
import numpy as np
import pytest

import kernel_reference as kref
from mpo_entry_fixtures import ebackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble
CAP = 512 * 256             # threads of the capped grid of one job


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one launch.  ``add_src(pre, m_in, post)`` -> index of a source slab (slabs ``gap`` elements apart);
    ``add_block(pre, post, rows, ...)`` with rows = [[(slab, c, alpha), ...], ...]: row o is the sum of alpha * middle row c of slab."""

    def __init__(self, cplx, seed, gap=3):
        self.cplx, self.gap = cplx, gap
        self.rng = np.random.default_rng(seed)
        self.slabs, self.src_len = [], gap
        self.jobs, self.rows, self.terms, self.want = [], [], [], []
        self.dst_len = gap

    def add_src(self, pre, m_in, post, pad=0):
        """A slab (pre, m_in, post) whose rows i are ``m_in * post + pad`` elements apart."""
        off = self.src_len
        ld = m_in * post + pad
        data = _rand(self.rng, max(pre, 1) * ld, self.cplx)
        self.slabs.append((off, ld, pre, m_in, post, data))
        self.src_len += len(data) + self.gap
        return len(self.slabs) - 1

    def add_block(self, pre, post, rows, split=None, ld_pad=0):
        """One destination block; ``split`` = row ranges [(r0, r1), ...] served by one job each (dst_ld = the whole block);
        ``ld_pad`` elements between the slabs i of the block that no job may write (dst_ld = n_rows post + ld_pad)."""
        n_rows = len(rows)
        ld = n_rows * post + ld_pad
        off = self.dst_len
        row_begin = len(self.rows)
        for terms in rows:
            self.rows.append([len(self.terms), len(terms)])
            for slab, c, alpha in terms:
                s_off, s_ld, s_pre, m_in, s_post, _ = self.slabs[slab]
                assert s_post == post and c < m_in and s_pre >= pre
                a = complex(alpha)
                self.terms.append([s_off + c * post, s_ld] + np.array([a.real, a.imag]).view(np.int64).tolist())
        if split is None:
            self.jobs.append([off, pre, n_rows, post, row_begin, ld if ld_pad else 0, 0, 0])
        else:
            for r0, r1 in split:
                self.jobs.append([off + r0 * post, pre, r1 - r0, post, row_begin + r0, ld, 0, 0])
        self.want.append((off, pre, post, rows, ld))
        self.dst_len += (max(pre - 1, 0) * ld + n_rows * post if pre else 0) + self.gap

    @staticmethod
    def dst_index(off, pre, post, rows, ld):
        """Element index of (i, o, j) of a destination block."""
        return off + np.arange(pre)[:, None, None] * ld + np.arange(len(rows))[None, :, None] * post + np.arange(post)[None, None, :]

    def src_host(self):
        dt = np.complex128 if self.cplx else np.float64
        src = np.full(self.src_len, np.nan, dtype=dt)
        for off, ld, pre, m_in, post, data in self.slabs:
            src[off:off + len(data)] = data
        return src

    def reference(self, src):
        """Per block: (re, im, magnitude sums, chain lengths per row) in extended precision."""
        out = []
        for off, pre, post, rows, _ in self.want:
            shape = (pre, len(rows), post)
            re, im, mr, mi = (np.zeros(shape, LD) for _ in range(4))
            nt = np.zeros(len(rows), dtype=np.int64)
            ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
            for o, terms in enumerate(rows):
                nt[o] = len(terms)
                for slab, c, alpha in terms:
                    s_off, s_ld = self.slabs[slab][:2]
                    xr, xi = kref.split(src[s_off + c * post + ii * s_ld + jj])
                    ar, ai = LD(complex(alpha).real), LD(complex(alpha).imag)
                    re[:, o] += ar * xr - ai * xi
                    im[:, o] += ar * xi + ai * xr
                    mr[:, o] += np.abs(ar * xr) + np.abs(ai * xi)
                    mi[:, o] += np.abs(ar * xi) + np.abs(ai * xr)
            out.append((re, im, mr, mi, nt))
        return out


def run_and_check(case, mis=None, tag=''):
    """One launch (twice: bit-identical) into a destination pre-filled with NaN between sentinels; everything the header promises
    checked; -> worst err / bound."""
    L = dev.lib()
    cplx = case.cplx
    W = 2 if cplx else 1
    dt = np.complex128 if cplx else np.float64
    src_host = case.src_host()
    sb = _Buf(_flat(src_host), mis == 'src')
    fill = np.full(case.dst_len * W, SENTINEL)
    for blk in case.want:
        idx = Case.dst_index(*blk).reshape(-1)
        for w in range(W):
            fill[W * idx + w] = np.nan
    db = _Buf(fill, mis == 'dst')
    jobs = np.array(case.jobs, dtype=np.int64).reshape(-1, 8)
    rows = np.array(case.rows if case.rows else [[0, 0]], dtype=np.int64).reshape(-1, 2)
    terms = np.array(case.terms if case.terms else [[0, 0, 0, 0]], dtype=np.int64).reshape(-1, 4)
    jd, rd, td = dev.to_device(jobs), dev.to_device(rows), dev.to_device(terms)
    max_cols = int(np.max(jobs[:, 1] * jobs[:, 3]))
    res = []
    for _ in range(2):
        db.reset()
        dev.check(L.tpa_mpo_entry_apply_batch(int(cplx), jd.data_ptr(), len(jobs), rd.data_ptr(), td.data_ptr(), max_cols, sb.ptr, db.ptr,
                                              dev.stream()), "mpo_entry_apply")
        res.append(db.get())
        assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src_host))), "src was written"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_mpo_entry_apply_batch is not deterministic"
    got = res[0].view(dt) if cplx else res[0]
    written = np.zeros(case.dst_len, dtype=bool)
    worst = 0.
    for (off, pre, post, rws, ld), (re, im, mr, mi, nt) in zip(case.want, case.reference(src_host)):
        idx = Case.dst_index(off, pre, post, rws, ld)
        assert not written[idx].any()
        written[idx] = True
        block = got[idx]
        assert not np.isnan(block).any(), "block at %d: an element was not written" % off
        gr, gi = kref.split(block)
        g = np.array([gamma((4 if cplx else 1) * k) for k in nt], dtype=LD)[None, :, None]
        lim_r, lim_i = g * mr, g * mi
        err_r, err_i = np.abs(gr - re), np.abs(gi - im)
        for o in np.nonzero(nt == 0)[0]:
            assert np.array_equal(kref.bits(_flat(np.ascontiguousarray(block[:, o]))), kref.bits(np.zeros(pre * post * W))), "row without terms"
        ratio = float(max(np.max(err_r / np.maximum(lim_r, LD(1e-300)), initial=0.), np.max(err_i / np.maximum(lim_i, LD(1e-300)), initial=0.)))
        assert np.all(err_r <= lim_r) and np.all(err_i <= lim_i), "block at %d: worst err / bound = %.3g" % (off, ratio)
        worst = max(worst, ratio)
    untouched = np.repeat(~written, W)
    assert np.array_equal(kref.bits(res[0][untouched]), kref.bits(np.full(int(untouched.sum()), SENTINEL))), "a gap between the slabs was written"
    print("CONFORMANCE tpa_mpo_entry_apply_batch(%s) %s jobs=%d rows=%d terms=%d max_cols=%d gap=%d%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(jobs), len(case.rows), len(case.terms), max_cols, case.gap,
             ' mis=' + mis if mis else '', worst))
    assert worst <= 1
    return worst


def _alpha(case):
    a = _rand(case.rng, 1, case.cplx)[0]
    return complex(a) if case.cplx else float(a)


def _random_rows(case, slabs, n_rows, max_terms):
    rows = []
    for o in range(n_rows):
        nt = 1 + (o * 7 + 3) % max_terms
        rows.append([(slabs[(o + t) % len(slabs)], (3 * o + 5 * t) % case.slabs[slabs[(o + t) % len(slabs)]][3], _alpha(case))
                     for t in range(nt)])
    return rows


@pytest.mark.parametrize("n_rows", [1, 25])
@pytest.mark.parametrize("post", [64, 65, 1, 6])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(ebackend, cplx, post, n_rows):
    """post even and odd, n_rows = 1 and 25 (beyond the 16 accumulators of the older kernel), pre = 1 and 3, one block per launch at
    an even gap (even post: the 16-byte form of real data) and at an odd one (odd dst_off and src_off: its 8-byte form); up to 6
    terms per row (the loads of four terms at a time and the remainder)."""
    for pre in (1, 3):
        for gap in (2, 3):
            case = Case(cplx, [1, int(cplx), post, n_rows, pre, gap], gap=gap)
            slabs = [case.add_src(pre, 7, post), case.add_src(pre, 4, post)]
            case.add_block(pre, post, _random_rows(case, slabs, n_rows, 6))
            run_and_check(case, tag='shape')


@pytest.mark.parametrize("mis", ['src', 'dst'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(ebackend, cplx, mis):
    """src_base / dst_base one real element off a 16-byte boundary, with an even and an odd post."""
    for post in (64, 65):
        case = Case(cplx, [2, int(cplx), post], gap=2)
        slabs = [case.add_src(3, 5, post), case.add_src(3, 2, post)]
        case.add_block(3, post, _random_rows(case, slabs, 4, 3))
        run_and_check(case, mis=mis, tag='mis')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_rows_without_terms_and_shared_blocks(ebackend, cplx):
    """In one launch: a row with term_count = 0 inside a job (zeros over the NaN fill), terms of one row with different src_ld (one of
    them odd), a block of 25 rows shared by two jobs through dst_ld > n_rows post, a job with pre = 0, a block without any term."""
    for post, gap, pad in ((64, 2, 2), (64, 2, 1), (33, 3, 1)):     # (real data: 16-byte form; odd src_ld; odd post and offsets)
        case = Case(cplx, [3, int(cplx), post, pad], gap=gap)
        a, b, c = case.add_src(3, 5, post), case.add_src(3, 3, post, pad=pad), case.add_src(3, 2, post, pad=4)
        rows = _random_rows(case, [a, b, c], 5, 4)
        rows[2] = []
        rows[3] = [(a, 1, _alpha(case)), (b, 2, _alpha(case)), (c, 0, _alpha(case)), (b, 0, _alpha(case)), (a, 4, _alpha(case))]
        case.add_block(3, post, rows)
        case.add_block(3, post, _random_rows(case, [a, b, c], 25, 5), split=[(0, 9), (9, 25)])
        case.add_block(0, post, [[(a, 0, 1.)]])
        case.add_block(2, post, [[], []])
        run_and_check(case, tag='rows')


@pytest.mark.parametrize("odd", ['src_ld', 'dst_ld'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_a_single_odd_stride(ebackend, cplx, odd):
    """A job whose ONLY odd quantity is src_ld (one slab at an even offset whose rows i are an odd number of elements apart), or
    dst_ld (a block at an even offset with one element between its slabs i, which has to stay untouched): post, dst_off, src_off and
    the other stride are even, so for real data the stride alone sends the job to the 8-byte form."""
    case = Case(cplx, [6, int(cplx), odd == 'src_ld'], gap=2)
    a = case.add_src(3, 4, 64, pad=1 if odd == 'src_ld' else 0)
    rows = _random_rows(case, [a], 5, 3)
    case.add_block(3, 64, rows, ld_pad=0 if odd == 'src_ld' else 1)
    (dst_off, _, _, post, _, dst_ld, _, _), = case.jobs
    src_offs, src_lds = {t[0] for t in case.terms}, {t[1] for t in case.terms}
    odd_ones = [n for n, v in (('post', post), ('dst_off', dst_off), ('dst_ld', dst_ld)) if v % 2] + \
        [n for n, vs in (('src_off', src_offs), ('src_ld', src_lds)) if any(v % 2 for v in vs)]
    assert odd_ones == [odd]
    run_and_check(case, tag='odd_' + odd)


def test_job_beyond_the_grid(ebackend):
    """One real job with pre = post = 520: 520 * 260 items of 16 bytes, more than the 512 * 256 threads of the capped grid, so the
    grid-stride loop runs."""
    assert 520 * 260 > CAP
    case = Case(False, [4], gap=2)
    a = case.add_src(520, 2, 520)
    case.add_block(520, 520, [[(a, 1, 0.75), (a, 0, -1.5)]])
    run_and_check(case, tag='big')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(ebackend, cplx):
    """n_jobs = 0 and -1: 0; n_jobs = 65536 and dtype = 2: TPA_E_BADARG; nothing is written in any of them."""
    L = dev.lib()
    W = 2 if cplx else 1
    case = Case(cplx, [5], gap=2)
    a = case.add_src(3, 2, 64)
    case.add_block(3, 64, [[(a, 0, 1.)], [(a, 1, 2.)]])
    sb = _Buf(_flat(case.src_host()))
    db = _Buf(np.full(case.dst_len * W, SENTINEL))
    jd, rd, td = (dev.to_device(np.array(t, dtype=np.int64)) for t in (case.jobs, case.rows, case.terms))
    args = lambda n_jobs: (int(cplx), jd.data_ptr(), n_jobs, rd.data_ptr(), td.data_ptr(), 3 * 64, sb.ptr, db.ptr, dev.stream())
    assert L.tpa_mpo_entry_apply_batch(*args(0)) == 0
    assert L.tpa_mpo_entry_apply_batch(*args(-1)) == 0
    assert L.tpa_mpo_entry_apply_batch(*args(65536)) == _lib.E_BADARG
    assert L.tpa_mpo_entry_apply_batch(2, *args(1)[1:]) == _lib.E_BADARG          # dtype
    assert np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))
    assert L.tpa_mpo_entry_apply_batch(*args(1)) == 0                             # (the same arguments do run)
    assert not np.array_equal(kref.bits(db.get()), kref.bits(np.full(case.dst_len * W, SENTINEL)))


def test_symbol_is_exported():
    assert 'tpa_mpo_entry_apply_batch' in _lib.exported_symbols()
