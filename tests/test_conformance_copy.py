"""Conformance of the batched data-movement entry points (``tpa_copy_batch``, ``tpa_lincomb_batch``, ``tpa_scale_axis_batch``,
``tpa_gather_axis_batch``, ``tpa_axis_sqnorm_batch``, ``tpa_tri_lower_batch``, ``tpa_convert``, ``tpa_fill_zero``) with the statement of
the header (tests/kernel_reference.py), on the numpy emulation (``mock``) and on the HIP kernels (``gpu``), real and complex.

These are batched kernels: blockIdx.y is the job, ``max_job_elems`` sizes blockIdx.x, capped at 512 workgroups of 256 threads.  A batch
therefore mixes jobs of one element, jobs smaller than a workgroup, a job with a zero extent and one job above 512 * 256 elements (the
grid-stride loop runs more than once), 1 to 300 jobs per launch.

Comparisons.  Pure moves (copy, gather, convert, fill_zero, the off-diagonal entries of tri_lower) and the scaling by a REAL vector
(one fp64 product per component) are compared bit for bit.  Derived bounds (u = 2^-53, EPS = 2^-52 = 2 u, ``mag`` = the magnitude sum
of tests/kernel_reference.py):
  * complex scale: product and difference of products, 2 roundings of a term: gamma_2 mag = 2 u / (1 - 2 u) mag <= EPS (1 + EPS) mag;
  * lincomb over T terms: a chain of T (fused) multiply-adds, complex data two products per term: f (T + 2) EPS mag, f = 1 real, 2 complex
    -- the bound of the GEMM chain with K_tot = T;
  * axis_sqnorm: one wavefront per row, lane l adds the squares of elements l, l + 64, ... (p = ceil(pre post / 64) of them, complex
    data two squares each), then the 6-step butterfly: L = (1 or 2) p + 6 and (L + 2) EPS sum |x|^2;
  * diagonal of tri_lower: (Re G_ii - 1) / 2 is one rounding of the difference (the halving is exact): EPS (|G_ii| + 1) / 2.
Destination arenas carry random numbers; every element that no job addresses has to keep its bit pattern."""
import numpy as np
import pytest

import kernel_reference as kref
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

EPS = 2.0**-52
LD = np.longdouble
MAXD = kref.MAXD
GRID_ELEMS = 512 * 256          # threads of the capped grid of one job
BATCHES = ['one_element', 'one_big_job', 'forty_jobs', 'three_hundred_jobs']


def job_sizes(rng, batch):
    """Element counts of the jobs of a batch (0 = a job with a zero extent)."""
    if batch == 'one_element':
        return [1]
    if batch == 'one_big_job':
        return [GRID_ELEMS * 5 // 4]
    n = 40 if batch == 'forty_jobs' else 300
    sizes = [1, 1, 0, 3, 63, 255, 256, 257, 1025] + [int(np.exp(rng.uniform(0, np.log(6000)))) for _ in range(n - 10)]
    sizes.append(GRID_ELEMS * 5 // 4 + int(rng.integers(3000)) if batch == 'three_hundred_jobs' else 20000)
    return [sizes[i] for i in rng.permutation(len(sizes))]


def _rand(rng, n, cplx):
    v = rng.standard_normal(n)
    return v + 1j * rng.standard_normal(n) if cplx else v


def _factor(rng, total, nd):
    """A shape of nd extents whose product is close to `total` (exactly 0 for total = 0: one extent is 0)."""
    if total == 0:
        shape = [int(rng.integers(1, 4)) for _ in range(nd)]
        shape[int(rng.integers(nd))] = 0
        return shape
    shape, rest = [], float(total)
    for d in range(nd - 1):
        e = max(1, min(int(rest), int(round(rest ** (1.0 / (nd - d)) * rng.uniform(0.5, 1.6)))))
        shape.append(e)
        rest = max(1.0, rest / e)
    shape.append(max(1, int(round(rest))))
    return [shape[i] for i in rng.permutation(nd)]


def _report(entry, cplx, batch, ratio=None):
    print("CONFORMANCE %s %s %s %s" % (entry, 'complex' if cplx else 'real', batch,
                                       'bitwise' if ratio is None else 'max_err_over_bound=%.4f' % ratio))


def _ratio(err, lim):
    err, lim = np.atleast_1d(np.asarray(err, LD)), np.atleast_1d(np.asarray(lim, LD))
    assert np.all(err <= lim), "worst err / bound = %.3g" % float(np.max(err / np.maximum(lim, np.finfo(LD).tiny)))
    nz = lim > 0
    return float(np.max(err[nz] / lim[nz])) if nz.any() else 0.0


def _bounded(got, ref, lim_re, lim_im, mask, x0):
    """Elements outside `mask` bit-unchanged, the others within the componentwise bounds -> max err / bound."""
    assert np.array_equal(kref.bits(got[~mask]), kref.bits(x0[~mask])), "an element that no job addresses changed"
    gr, gi = kref.split(got[mask])
    return max(_ratio(np.abs(gr - ref['re'][mask]), lim_re[mask]), _ratio(np.abs(gi - ref['im'][mask]), lim_im[mask]))


class Case:
    pass


# ---- tpa_copy_batch ---------------------------------------------------------------------------------------------------------

def copy_case(rng, cplx, batch):
    """Jobs of 1 to 6 dimensions; source and destination are slices (extents padded by 0 - 2) of parents whose axes are stored in
    independently permuted orders; the conjugation flag is set on about half of the jobs."""
    jobs, s_size, d_size = [], 5, 7
    for total in job_sizes(rng, batch):
        nd = int(rng.integers(1, MAXD + 1))
        shape = _factor(rng, total, nd)
        row = [0, 0, nd, int(rng.integers(2))] + [0] * (3 * MAXD)
        for side, base in ((1, 4 + MAXD), (2, 4 + 2 * MAXD)):
            stride, run = [0] * nd, 1
            for d in rng.permutation(nd):
                stride[d] = run
                run *= shape[d] + int(rng.integers(3))
            row[base:base + nd] = stride
            if side == 1:
                row[0], d_size = d_size, d_size + run + int(rng.integers(1, 9))
            else:
                row[1], s_size = s_size, s_size + run + int(rng.integers(1, 9))
        row[4:4 + nd] = shape
        jobs.append(row)
    c = Case()
    c.cplx, c.jobs = cplx, np.array(jobs, np.int64)
    c.max_elems = max(1, max(int(np.prod(j[4:4 + j[2]])) for j in jobs))
    c.src, c.dst0 = _rand(rng, s_size, cplx), _rand(rng, d_size, cplx)
    return c


def run_copy(c, L=None):
    L = L if L is not None else dev.lib()
    jd, sd, dd = dev.to_device(c.jobs), dev.to_device(c.src), dev.to_device(c.dst0)
    dev.check(L.tpa_copy_batch(int(c.cplx), jd.data_ptr(), len(c.jobs), c.max_elems, sd.data_ptr(), dd.data_ptr(), dev.stream()), "copy_batch")
    return dev.to_host(dd)


def check_copy(c, got):
    want, mask = kref.copy_batch(c.cplx, c.jobs, c.src, c.dst0)
    assert np.array_equal(kref.bits(got), kref.bits(want)), "tpa_copy_batch: %d elements differ" % np.sum(kref.bits(got) != kref.bits(want))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_copy_batch(backend, cplx, batch):
    c = copy_case(np.random.default_rng([1, int(cplx), BATCHES.index(batch)]), cplx, batch)
    if batch in ('forty_jobs', 'three_hundred_jobs'):
        assert set(c.jobs[:, 2]) == set(range(1, MAXD + 1)) and set(c.jobs[:, 3]) == {0, 1}
    if batch in ('one_big_job', 'three_hundred_jobs'):
        assert c.max_elems > GRID_ELEMS
    check_copy(c, run_copy(c))
    _report("tpa_copy_batch", cplx, batch)


# ---- tpa_lincomb_batch ------------------------------------------------------------------------------------------------------

def _lincomb_case(rng, cplx, batch):
    jobs, terms, d_size = [], [], 3
    s_size = 2 * GRID_ELEMS if batch in ('one_big_job', 'three_hundred_jobs') else 60000
    for total in job_sizes(rng, batch):
        rows, cols = _factor(rng, total, 2)
        d_ld = cols + int(rng.integers(3))
        nt = int(rng.integers(0, 6))          # 0 terms: the slab is zeroed
        jobs.append([d_size, rows, cols, d_ld, len(terms), nt, 0, 0])
        d_size += max(rows, 1) * d_ld + int(rng.integers(1, 9))
        for _ in range(nt):
            s_ld = cols + int(rng.integers(4))
            off = int(rng.integers(0, s_size - max(rows, 1) * s_ld - cols))
            a = rng.standard_normal(2)
            terms.append([off, s_ld] + np.array(a).view(np.int64).tolist())
    c = Case()
    c.cplx, c.jobs = cplx, np.array(jobs, np.int64)
    c.terms = np.array(terms if terms else [[0, 1, 0, 0]], np.int64)
    c.max_elems = max(1, int(np.max(c.jobs[:, 1] * c.jobs[:, 2])))
    c.src, c.dst0 = _rand(rng, s_size, cplx), _rand(rng, d_size, cplx)
    return c


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_lincomb_batch(backend, cplx, batch):
    L = dev.lib()
    c = _lincomb_case(np.random.default_rng([2, int(cplx), BATCHES.index(batch)]), cplx, batch)
    if batch in ('one_big_job', 'three_hundred_jobs'):
        assert c.max_elems > GRID_ELEMS
    jd, td, sd, dd = (dev.to_device(x) for x in (c.jobs, c.terms, c.src, c.dst0))
    dev.check(L.tpa_lincomb_batch(int(cplx), jd.data_ptr(), len(c.jobs), td.data_ptr(), c.max_elems, sd.data_ptr(), dd.data_ptr(),
                                  dev.stream()), "lincomb_batch")
    ref = kref.lincomb_batch(cplx, c.jobs, c.terms, c.src, c.dst0)
    f = (2 if cplx else 1) * (ref['nterms'] + 2) * EPS
    _report("tpa_lincomb_batch", cplx, batch, _bounded(dev.to_host(dd), ref, f * ref['mag_re'], f * ref['mag_im'], ref['mask'], c.dst0))


# ---- tpa_scale_axis_batch ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("kind", ['real_x_real_s', 'complex_x_real_s', 'complex_x_complex_s'])
def test_scale_axis_batch(backend, kind, batch):
    L = dev.lib()
    cplx, s_cplx = kind != 'real_x_real_s', kind == 'complex_x_complex_s'
    rng = np.random.default_rng([3, BATCHES.index(batch), int(cplx), int(s_cplx)])
    jobs, x_size, s_size = [], 2, 11
    for total in job_sizes(rng, batch):
        pre, ln, post = _factor(rng, total, 3)
        jobs.append([x_size, pre, ln, post, s_size, 0])          # s_off is never 0
        x_size += pre * ln * post + int(rng.integers(1, 9))
        s_size += ln + int(rng.integers(3))
    jobs = np.array(jobs, np.int64)
    x0, s = _rand(rng, x_size, cplx), _rand(rng, s_size + 1, s_cplx)
    jd, xd, sd = dev.to_device(jobs), dev.to_device(x0), dev.to_device(s)
    dev.check(L.tpa_scale_axis_batch(int(cplx), jd.data_ptr(), len(jobs), max(1, int(np.max(np.prod(jobs[:, 1:4], axis=1)))), xd.data_ptr(),
                                     sd.data_ptr(), int(s_cplx), dev.stream()), "scale_axis_batch")
    got = dev.to_host(xd)
    ref = kref.scale_axis_batch(jobs, x0, s)
    if batch in ('one_big_job', 'three_hundred_jobs'):
        assert np.max(np.prod(jobs[:, 1:4], axis=1)) > GRID_ELEMS
    if s_cplx:
        _report("tpa_scale_axis_batch(%s)" % kind, cplx, batch, _bounded(got, ref, EPS * (1 + EPS) * ref['mag_re'], EPS * (1 + EPS) * ref['mag_im'], ref['mask'], x0))
    else:       # one fp64 product per component
        assert np.array_equal(kref.bits(got), kref.bits(ref['fp64']))
        _report("tpa_scale_axis_batch(%s)" % kind, cplx, batch)


# ---- tpa_gather_axis_batch --------------------------------------------------------------------------------------------------

def gather_case(rng, cplx, batch):
    jobs, idx, d_size, s_size = [], [0, 0, 0], 4, 9          # idx_off is never 0
    for total in job_sizes(rng, batch):
        pre, ld, post = _factor(rng, total, 3)
        ls = max(1, int(ld * rng.uniform(0.4, 1.5)))          # fewer source slices than gathered ones: repeated indices
        jobs.append([d_size, s_size, pre, ls, ld, post, len(idx), 0])
        idx += rng.integers(0, ls, size=ld).tolist()
        d_size += pre * ld * post + int(rng.integers(1, 9))
        s_size += pre * ls * post + int(rng.integers(1, 9))
    c = Case()
    c.cplx, c.jobs, c.idx = cplx, np.array(jobs, np.int64), np.array(idx + [0], np.int64)
    c.max_elems = max(1, int(np.max(c.jobs[:, 2] * c.jobs[:, 4] * c.jobs[:, 5])))
    c.src, c.dst0 = _rand(rng, s_size, cplx), _rand(rng, d_size, cplx)
    return c


def run_gather(c, L=None):
    L = L if L is not None else dev.lib()
    jd, idd, sd, dd = (dev.to_device(x) for x in (c.jobs, c.idx, c.src, c.dst0))
    dev.check(L.tpa_gather_axis_batch(int(c.cplx), jd.data_ptr(), len(c.jobs), c.max_elems, idd.data_ptr(), sd.data_ptr(), dd.data_ptr(),
                                      dev.stream()), "gather_axis_batch")
    return dev.to_host(dd)


def check_gather(c, got):
    want, mask = kref.gather_axis_batch(c.jobs, c.idx, c.src, c.dst0)
    assert np.array_equal(kref.bits(got), kref.bits(want)), "tpa_gather_axis_batch: %d elements differ" % np.sum(kref.bits(got) != kref.bits(want))


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_gather_axis_batch(backend, cplx, batch):
    c = gather_case(np.random.default_rng([4, int(cplx), BATCHES.index(batch)]), cplx, batch)
    assert np.all(c.jobs[:, 6] > 0)
    if batch in ('one_big_job', 'three_hundred_jobs'):
        assert c.max_elems > GRID_ELEMS
    check_gather(c, run_gather(c))
    _report("tpa_gather_axis_batch", cplx, batch)


# ---- tpa_axis_sqnorm_batch --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_axis_sqnorm_batch(backend, cplx):
    """pre * post below, equal to and above the 64 lanes of the wavefront that owns a row; the row table is shuffled and padded to a
    multiple of 4 with job = -1 entries (not only at its end)."""
    L = dev.lib()
    rng = np.random.default_rng([5, int(cplx)])
    shapes = [(1, 1, 1), (1, 7, 1), (4, 5, 8), (8, 3, 8), (64, 2, 1), (1, 3, 64), (5, 4, 13), (16, 4, 9), (70, 3, 50), (3, 130, 2)]
    jobs, rows, x_size, o_size = [], [], 3, 5
    for jb, (pre, ln, post) in enumerate(shapes):
        jobs.append([x_size, pre, ln, post, o_size, 0])
        rows += [[jb, j] for j in range(ln)]
        x_size += pre * ln * post + int(rng.integers(1, 9))
        o_size += ln + int(rng.integers(1, 4))
    rows += [[-1, 0]] * (3 + (-(len(rows) + 3)) % 4)
    rows = np.array(rows, np.int32)[rng.permutation(len(rows))]
    assert len(rows) % 4 == 0 and np.sum(rows[:, 0] < 0) >= 3
    jobs = np.array(jobs, np.int64)
    x, out0 = _rand(rng, x_size, cplx), rng.standard_normal(o_size)
    jd, rd, xd, od = (dev.to_device(a) for a in (jobs, rows, x, out0))
    dev.check(L.tpa_axis_sqnorm_batch(int(cplx), jd.data_ptr(), rd.data_ptr(), len(rows), xd.data_ptr(), od.data_ptr(), dev.stream()), "axis_sqnorm")
    got = dev.to_host(od)
    val, mask, cnt = kref.axis_sqnorm_batch(jobs, rows, x, out0)
    assert np.array_equal(kref.bits(got[~mask]), kref.bits(out0[~mask]))
    chain = (2 if cplx else 1) * -(-cnt[mask] // 64) + 6
    _report("tpa_axis_sqnorm_batch", cplx, 'rows=%d' % len(rows), _ratio(np.abs(got[mask].astype(LD) - val[mask]), (chain + 2) * EPS * val[mask]))


# ---- tpa_tri_lower_batch ----------------------------------------------------------------------------------------------------

def tri_case(rng, cplx, sizes):
    jobs, g_size = [], 6
    for n in sizes:
        jobs.append([g_size, n])
        g_size += n * n + int(rng.integers(1, 9))
    c = Case()
    c.cplx, c.jobs, c.g0 = cplx, np.array(jobs, np.int64), _rand(rng, g_size, cplx)
    for g_off, n in jobs[::2]:          # every second job: a Gram matrix of nearly orthonormal rows, diagonal close to 1
        c.g0[g_off + np.arange(n) * (n + 1)] = 1 + 1e-3 * _rand(rng, n, cplx)
    c.max_elems = max(1, max(n * n for n in sizes))
    return c


def run_tri(c, L=None):
    L = L if L is not None else dev.lib()
    jd, gd = dev.to_device(c.jobs), dev.to_device(c.g0)
    dev.check(L.tpa_tri_lower_batch(int(c.cplx), jd.data_ptr(), len(c.jobs), c.max_elems, gd.data_ptr(), dev.stream()), "tri_lower_batch")
    return dev.to_host(gd)


def check_tri(c, got):
    want, mask, dmask, diag = kref.tri_lower_batch(c.jobs, c.g0)
    assert np.array_equal(kref.bits(got[~dmask] + 0.0), kref.bits(want[~dmask] + 0.0)), "tpa_tri_lower_batch: off-diagonal / untouched elements differ"
    gr, gi = kref.split(got[dmask])
    assert np.all(gi == 0)
    return _ratio(np.abs(gr - diag[dmask]), EPS * (np.abs(c.g0[dmask].real) + 1) / 2)


@pytest.mark.parametrize("sizes", [[1], [400], [1, 2, 0, 17, 64, 3, 65, 1, 400, 31]], ids=['one_element', 'one_big_job', 'ten_jobs'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_tri_lower_batch(backend, cplx, sizes):
    assert 400 * 400 > GRID_ELEMS
    c = tri_case(np.random.default_rng([6, int(cplx), len(sizes)]), cplx, sizes)
    _report("tpa_tri_lower_batch", cplx, 'jobs=%d' % len(sizes), check_tri(c, run_tri(c)))


# ---- tpa_convert / tpa_fill_zero -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 1000, 2048 * 256 + 5])
@pytest.mark.parametrize("conj", [0, 1])
@pytest.mark.parametrize("mode", ['f64_to_f64', 'f64_to_c128', 'c128_to_f64', 'c128_to_c128'])
def test_convert(backend, mode, conj, n):
    """All four modes, with and without the conjugation request (it acts on c128 -> c128 only); 2048 * 256 + 5 elements: more than one
    pass of the capped grid.  The elements behind the n-th keep their bits."""
    L = dev.lib()
    fc, tc = mode.startswith('c128'), mode.endswith('c128')
    rng = np.random.default_rng([7, int(fc), int(tc), n])
    src, dst0 = _rand(rng, n + 2, fc), _rand(rng, n + 3, tc)
    sd, dd = dev.to_device(src), dev.to_device(dst0)
    dev.check(L.tpa_convert(int(fc), int(tc), n, sd.data_ptr(), dd.data_ptr(), conj, dev.stream()), "convert")
    got = dev.to_host(dd)
    assert np.array_equal(kref.bits(got[:n]), kref.bits(kref.convert(fc, tc, src[:n], conj)))
    assert np.array_equal(kref.bits(got[n:]), kref.bits(dst0[n:])) and np.array_equal(kref.bits(dev.to_host(sd)), kref.bits(src))
    _report("tpa_convert(%s,conj=%d)" % (mode, conj), tc, 'n=%d' % n)


@pytest.mark.parametrize("n_bytes,shift", [(0, 0), (1, 0), (7, 1), (13, 3), (24, 8), (1000003, 0), (1000003, 5), (4099, 16)])
def test_fill_zero(backend, n_bytes, shift):
    """Byte counts that are no multiples of 8 or 16, start addresses that are not aligned either; the bytes around stay."""
    L = dev.lib()
    raw0 = np.random.default_rng(n_bytes + shift).integers(1, 256, size=n_bytes + shift + 37, dtype=np.uint8)
    rd = dev.to_device(raw0)
    dev.check(L.tpa_fill_zero(rd.data_ptr() + shift, n_bytes, dev.stream()), "fill_zero")
    want = raw0.copy()
    want[shift:] = kref.fill_zero(raw0[shift:], n_bytes)
    assert np.array_equal(dev.to_host(rd), want)
    _report("tpa_fill_zero", False, 'bytes=%d,shift=%d' % (n_bytes, shift))


# ---- argument limits --------------------------------------------------------------------------------------------------------

def test_job_count_limit(backend):
    """blockIdx.y is the job: 65536 jobs are TPA_E_BADARG before anything is launched (the arenas keep their bits)."""
    L = dev.lib()
    x0 = np.random.default_rng(8).standard_normal(64)
    tab = dev.to_device(np.zeros(64, np.int64))
    xd, yd = dev.to_device(x0), dev.to_device(x0)
    st = dev.stream()
    for n_jobs, want in ((65536, _lib.E_BADARG), (1 << 20, _lib.E_BADARG), (0, 0), (-1, 0)):
        assert L.tpa_copy_batch(0, tab.data_ptr(), n_jobs, 1, xd.data_ptr(), yd.data_ptr(), st) == want
        assert L.tpa_lincomb_batch(0, tab.data_ptr(), n_jobs, tab.data_ptr(), 1, xd.data_ptr(), yd.data_ptr(), st) == want
        assert L.tpa_scale_axis_batch(0, tab.data_ptr(), n_jobs, 1, yd.data_ptr(), xd.data_ptr(), 0, st) == want
        assert L.tpa_tri_lower_batch(0, tab.data_ptr(), n_jobs, 1, yd.data_ptr(), st) == want
        assert L.tpa_gather_axis_batch(0, tab.data_ptr(), n_jobs, 1, tab.data_ptr(), xd.data_ptr(), yd.data_ptr(), st) == want
    assert np.array_equal(kref.bits(dev.to_host(yd)), kref.bits(x0)) and np.array_equal(kref.bits(dev.to_host(xd)), kref.bits(x0))
