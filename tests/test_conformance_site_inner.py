"""Conformance of ``tpa_site_inner_batch`` (out[s, k] = sum over the jobs of column k of <b block| coeff |x block of stack slot s>) with
the extended-precision statement of the header, on the numpy emulation (``mock``) and on the HIP kernel (``gpu``), real and complex,
with the apparatus of ``test_conformance_mpo_cell.py``: sentinels around every buffer, two launches that must agree bit for bit, the
sources compared bitwise afterwards.

Launch geometry (documented next to the kernel in csrc/tpa_site_inner.hip): a thread owns columns (i, item of j) of a job; per group of
8 stack slots it folds conj(b) coeff into d_x values (D = 2, 4, 8 or 16 registers: the smallest D >= max_d) and streams x; an ITEM is 16
bytes (one complex element, or two real elements of one row) when b_base and x_base are 16-byte aligned and, for real data, post, b_off,
b_ld, x_off, x_ld and x_sstride of the job are even -- else one element (decided per job).  256 threads per workgroup, grid
(min(512, ceil(items of max_job_cols / 1024)), n_jobs), grid-stride over the columns.  So the edges are: d_b != d_x out of {1, 2, 3, 16},
n_stack = 1, 7, 8, 9, 65 (below, at and above a group; nine groups), post = 64, 65, 6, 1 and pre = 0, 1, 3, the stack index slowest and
between i and c, each parity quantity as the only odd one, each base 8 bytes off a 16-byte boundary, several jobs on one output column, a
column without a job, a coefficient block with zeros, b aliasing x, a job with several columns per thread (the grid-stride loop), max_d at
and below a job's d.

Bound (derived; u = 2^-53), for an ARBITRARY summation order: out[s, k] is a sum of N = sum_{jobs of k} pre post d_b d_x triple products
conj(b) coeff x.  Real data: a product is rounded at most twice (two multiplications, or one and the multiplication inside a fused
multiply-add) and passes at most N - 1 additions, whatever the order and the grouping (fold over o first, tree over lanes, partials):
|err| <= gamma_n sum |b| |coeff| |x| with n = N + 2, gamma_n = n u / (1 - n u).  Complex data: a component of the result is a sum of 4 N
real triple products, each rounded at most 2 + (4 N - 1) times, and its magnitude sum is below sum (|b_re| + |b_im|)(|c_re| + |c_im|)
(|x_re| + |x_im|): n = 4 (N + 2), the factor 4 of the sibling tests.  A column without a job, and F64's imaginary parts: exact zeros.

Every run prints a ``CONFORMANCE`` line with its worst err / bound.  With ``TPA_WRITE_PROFILES=1`` the module also writes the worst
figure per group of cases to ``profiles/site_inner_conformance.txt`` when its last test has run (the committed file is that of a run on
the MI355X; without the variable the tree is left as it is)."""
import os

import numpy as np
import pytest

import kernel_reference as kref
from measure_fixtures import mbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble


WORST = {}          # (backend, group of cases, dtype) -> [cases, worst err / bound]


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    if os.environ.get('TPA_WRITE_PROFILES') != '1' or not WORST:
        return
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'site_inner_conformance.txt')
    lines = ["tpa_site_inner_batch: worst err / bound per group of cases of tests/test_conformance_site_inner.py",
             "(bound: gamma_n sum |b| |coeff| |x| for an arbitrary summation order, n = N + 2 real, 4 (N + 2) complex)", "",
             "%-8s %-14s %-8s %6s  %s" % ("backend", "group", "dtype", "cases", "max err / bound")]
    lines += ["%-8s %-14s %-8s %6d  %.4f" % (k + tuple(v)) for k, v in WORST.items()]
    with open(path, 'w') as f:
        f.write("\n".join(lines) + "\n")


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one launch.  ``add(pre, d_b, d_x, post, col, layout, ...)`` puts a block pair behind what is there; with
    ``alias`` the b blocks lie in the x buffer."""

    def __init__(self, cplx, seed, n_stack, n_out=1, gap=2, alias=False):
        self.cplx, self.gap, self.n_stack, self.n_out, self.alias = cplx, gap, n_stack, n_out, alias
        self.rng = np.random.default_rng(seed)
        self.jobs, self.coeff, self.want = [], [], []
        self.b_len, self.x_len = gap, gap
        self.b_data, self.x_data = [], []

    def add(self, pre, d_b, d_x, post, col=0, layout='mid', b_lead=0, b_pad=0, x_lead=0, x_pad=0, s_pad=0, C=None):
        """b block (pre, d_b, post) with rows ``d_b post + b_pad`` apart; x block (pre, n_stack, d_x, post) ('mid': the stack between
        i and c, slots ``d_x post + s_pad`` apart, rows ``n_stack`` slots ``+ x_pad``) or (n_stack, pre, d_x, post) ('slow': rows
        ``d_x post + x_pad`` apart, slots ``pre`` rows ``+ s_pad``)."""
        S = self.n_stack
        b_ld = d_b * post + b_pad
        if layout == 'mid':
            x_ss = d_x * post + s_pad
            x_ld = S * x_ss + x_pad
            x_n = max(pre, 1) * x_ld
        else:
            x_ld = d_x * post + x_pad
            x_ss = max(pre, 1) * x_ld + s_pad
            x_n = S * x_ss
        x_off = self.x_len + x_lead
        self.x_data.append((x_off, _rand(self.rng, x_n, self.cplx)))
        self.x_len = x_off + x_n + self.gap
        b_n = max(pre, 1) * b_ld
        if self.alias:
            b_off = self.x_len + b_lead
            self.x_data.append((b_off, _rand(self.rng, b_n, self.cplx)))
            self.x_len = b_off + b_n + self.gap
        else:
            b_off = self.b_len + b_lead
            self.b_data.append((b_off, _rand(self.rng, b_n, self.cplx)))
            self.b_len = b_off + b_n + self.gap
        if C is None:
            C = _rand(self.rng, d_b * d_x, self.cplx).reshape(d_b, d_x)
            C[self.rng.random((d_b, d_x)) < 0.3] = 0            # a coefficient block with zeros
        c_off = len(self.coeff)
        self.coeff += np.asarray(C).reshape(-1).tolist()
        self.jobs.append([b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, c_off, col, 0])
        self.want.append(np.asarray(C))

    def host(self):
        dt = np.complex128 if self.cplx else np.float64
        xh = np.full(self.x_len, np.nan, dtype=dt)
        for off, data in self.x_data:
            xh[off:off + len(data)] = data
        bh = np.full(self.b_len, np.nan, dtype=dt)
        for off, data in self.b_data:
            bh[off:off + len(data)] = data
        return (xh if self.alias else bh), xh

    def reference(self, bh, xh, max_d):
        """(re, im, magnitude sum, number of products) per output (s, k) in extended precision."""
        S, K = self.n_stack, self.n_out
        re, im, mag = np.zeros((S, K), LD), np.zeros((S, K), LD), np.zeros((S, K), LD)
        count = np.zeros(K, dtype=np.int64)
        ss = np.arange(S)[:, None, None, None]
        for (b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, _, col, _), C in zip(self.jobs, self.want):
            if not 0 <= col < K or min(pre, post, d_b, d_x) <= 0:
                continue
            nb, nx = min(d_b, max_d), min(d_x, max_d)
            count[col] += pre * post * nb * nx
            ii, jj = np.arange(pre)[:, None, None], np.arange(post)[None, None, :]
            br, bi = kref.split(bh[b_off + ii * b_ld + np.arange(nb)[None, :, None] * post + jj])
            xr, xi = kref.split(xh[x_off + ii[None] * x_ld + ss * x_ss + np.arange(nx)[None, None, :, None] * post + jj[None]])
            ar, ai = kref.split(C[:nb, :nx])
            tr, ti, tm = np.zeros((pre, nx, post), LD), np.zeros((pre, nx, post), LD), np.zeros((pre, nx, post), LD)
            for o in range(nb):         # t_c = sum_o conj(b_o) a[o, c]
                tr += br[:, o, None, :] * ar[o][None, :, None] + bi[:, o, None, :] * ai[o][None, :, None]
                ti += br[:, o, None, :] * ai[o][None, :, None] - bi[:, o, None, :] * ar[o][None, :, None]
                tm += (np.abs(br[:, o, None, :]) + np.abs(bi[:, o, None, :])) * (np.abs(ar[o]) + np.abs(ai[o]))[None, :, None]
            re[:, col] += np.sum(tr[None] * xr - ti[None] * xi, axis=(1, 2, 3))
            im[:, col] += np.sum(tr[None] * xi + ti[None] * xr, axis=(1, 2, 3))
            mag[:, col] += np.sum(tm[None] * (np.abs(xr) + np.abs(xi)), axis=(1, 2, 3))
        return re, im, mag, count


def launch(case, max_d, bb, xb, ob, work):
    jobs = np.array(case.jobs, dtype=np.int64).reshape(-1, 12)
    coeff = np.array(case.coeff if case.coeff else [0], dtype=np.complex128 if case.cplx else np.float64)
    jd, cd = dev.to_device(jobs), dev.to_device(_flat(coeff))
    max_cols = max(int(np.max(jobs[:, 7] * jobs[:, 8])), 1)
    need = dev.lib().tpa_site_inner_work(len(jobs), case.n_stack, case.n_out, max_cols)
    assert need <= work.numel()
    dev.check(dev.lib().tpa_site_inner_batch(int(case.cplx), jd.data_ptr(), len(jobs), cd.data_ptr(), max_d, case.n_stack, case.n_out,
                                             max_cols, bb.ptr, xb.ptr, ob.ptr, work.data_ptr(), dev.stream()), "site_inner")
    return jd, cd


def run_and_check(case, mis=None, tag='', max_d=None):
    """One launch (twice: bit-identical) into an output pre-filled with NaN between sentinels; -> worst err / bound."""
    cplx = case.cplx
    bh, xh = case.host()
    xb = _Buf(_flat(xh), mis == 'x')
    bb = xb if case.alias else _Buf(_flat(bh), mis == 'b')
    if max_d is None:
        max_d = max(max(j[2], j[6]) for j in case.jobs)
    S, K = case.n_stack, case.n_out
    ob = _Buf(np.full(2 * S * K, np.nan))
    jobs = np.array(case.jobs, dtype=np.int64).reshape(-1, 12)
    n_work = int(dev.lib().tpa_site_inner_work(len(jobs), S, K, max(int(np.max(jobs[:, 7] * jobs[:, 8])), 1)))
    work = dev.to_device(np.full(n_work + 4, SENTINEL))
    res = []
    for _ in range(2):
        ob.reset()
        keep = launch(case, max_d, bb, xb, ob, work)
        res.append(ob.get())
        del keep
        assert np.array_equal(kref.bits(xb.get()), kref.bits(_flat(xh))), "x was written"
        if not case.alias:
            assert np.array_equal(kref.bits(bb.get()), kref.bits(_flat(bh))), "b was written"
    assert np.array_equal(kref.bits(dev.to_host(work)[n_work:]), kref.bits(np.full(4, SENTINEL))), "written behind the work area"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_site_inner_batch is not deterministic"
    got = res[0].reshape(S, K, 2)
    assert not np.isnan(got).any(), "an output was not written"
    re, im, mag, count = case.reference(bh, xh, max_d)
    worst = 0.
    for k in range(K):
        if count[k] == 0:
            assert np.array_equal(kref.bits(got[:, k]), kref.bits(np.zeros(2 * S))), "a column without a job is not zero"
            continue
        lim = gamma((4 if cplx else 1) * (int(count[k]) + 2)) * mag[:, k]
        err_r, err_i = np.abs(got[:, k, 0] - re[:, k]), np.abs(got[:, k, 1] - im[:, k])
        if not cplx:
            assert np.array_equal(kref.bits(got[:, k, 1]), kref.bits(np.zeros(S))), "imaginary part of real data"
        ratio = float(max(np.max(err_r / np.maximum(lim, LD(1e-300))), np.max(err_i / np.maximum(lim, LD(1e-300)))))
        assert np.all(err_r <= lim) and np.all(err_i <= lim), "column %d: worst err / bound = %.3g" % (k, ratio)
        worst = max(worst, ratio)
    print("CONFORMANCE tpa_site_inner_batch(%s) %s jobs=%d n_stack=%d n_out=%d max_d=%d%s%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(case.jobs), S, K, max_d, ' mis=' + mis if mis else '', ' alias' if case.alias else '',
             worst))
    ent = WORST.setdefault(('mock' if hasattr(dev.lib(), 'real') else 'gpu', tag, 'complex' if cplx else 'real'), [0, 0.])
    ent[0], ent[1] = ent[0] + 1, max(ent[1], worst)
    assert worst <= 1
    return worst, got


D_PAIRS = [(1, 2), (2, 1), (2, 3), (3, 2), (3, 16), (16, 3), (1, 16)]


@pytest.mark.parametrize("n_stack", [1, 7, 8, 9, 65])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(mbackend, cplx, n_stack):
    """d_b != d_x out of {1, 2, 3, 16}, post = 64, 65, 6, 1, pre = 0, 1, 3, both stack layouts, everything at even offsets (even post:
    the 16-byte form of real data) and at odd ones (its 8-byte form)."""
    for n, (post, pre, gap) in enumerate(((64, 3, 2), (65, 1, 3), (6, 3, 2), (1, 3, 3), (64, 0, 2))):
        for m, (d_b, d_x) in enumerate(D_PAIRS):
            if n_stack == 65 and (m + n) % 3:       # (nine groups: a third of the combinations, every post and every d among them)
                continue
            case = Case(cplx, [1, int(cplx), post, n_stack, d_b, d_x], n_stack, gap=gap)
            case.add(pre, d_b, d_x, post, layout='mid' if (n + m) % 2 else 'slow')
            case.add(1, d_x, d_b, post, layout='slow' if (n + m) % 2 else 'mid', x_pad=gap, s_pad=gap, b_pad=gap)
            run_and_check(case, tag='shape')


@pytest.mark.parametrize("mis", ['b', 'x'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(mbackend, cplx, mis):
    """b_base / x_base one real element off a 16-byte boundary, with an even and an odd post."""
    for post in (64, 65):
        case = Case(cplx, [2, int(cplx), post], 9)
        case.add(3, 2, 3, post, layout='mid')
        case.add(3, 3, 2, post, layout='slow')
        run_and_check(case, mis=mis, tag='mis')


ODD = ['post', 'b_off', 'b_ld', 'x_off', 'x_ld', 'x_sstride']


@pytest.mark.parametrize("layout", ['mid', 'slow'])
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_a_single_odd_quantity(mbackend, cplx, odd, layout):
    """A job whose ONLY odd quantity is post, b_off, b_ld, x_off, x_ld or x_sstride: everything else is even, so for real data that
    quantity alone sends the job to the 8-byte form.  (Odd post: d_b = d_x = 2 and pre = 2 keep every stride even.)"""
    S = 4
    case = Case(cplx, [6, int(cplx), ODD.index(odd), layout == 'mid'], S, gap=2)
    post = 65 if odd == 'post' else 64
    kw = dict(b_lead=int(odd == 'b_off'), b_pad=int(odd == 'b_ld'), x_lead=int(odd == 'x_off'))
    if layout == 'mid':         # x_ld = S (x_ss) + x_pad
        kw.update(s_pad=2 * int(odd == 'x_sstride'), x_pad=int(odd == 'x_ld'))
        if odd == 'x_sstride':
            kw.update(s_pad=1)  # (S = 4 slots: x_ld stays even)
    else:                       # x_ss = pre x_ld + s_pad
        kw.update(x_pad=int(odd == 'x_ld'), s_pad=int(odd == 'x_sstride'))
    case.add(2, 2, 2, post, layout=layout, **kw)
    b_off, b_ld, _, x_off, x_ld, x_ss, _, _, post_j, _, _, _ = case.jobs[0]
    odd_ones = [n for n, v in zip(ODD, (post_j, b_off, b_ld, x_off, x_ld, x_ss)) if v % 2]
    assert odd_ones == [odd], odd_ones
    run_and_check(case, tag='odd_' + odd)


@pytest.mark.parametrize("alias", [False, True], ids=['apart', 'alias'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_columns_jobs_and_alias(mbackend, cplx, alias):
    """Three output columns: column 0 gets three jobs (one of them with pre = 0, one with a zero coefficient block), column 1 none
    (zeros), column 2 one; a job whose out_col lies outside [0, n_out) contributes nothing; with ``alias`` b and x are one buffer."""
    case = Case(cplx, [3, int(cplx), alias], 9, n_out=3, alias=alias)
    case.add(3, 2, 3, 64, col=0, layout='mid')
    case.add(2, 3, 1, 33, col=0, layout='slow', x_pad=1)
    case.add(0, 2, 2, 64, col=0)
    case.add(3, 2, 2, 6, col=0, C=np.zeros((2, 2)))
    case.add(3, 1, 2, 65, col=2, layout='slow')
    case.add(3, 2, 2, 8, col=3)
    case.add(3, 2, 2, 8, col=-1)
    _, got = run_and_check(case, tag='jobs')
    assert np.all(got[:, 1] == 0)


def test_job_beyond_the_grid(mbackend):
    """One real job with pre = post = 520, n_stack = 2: 520 * 260 items of 16 bytes over the 512 workgroups of the capped grid (more
    than one column per thread: the grid-stride loop runs)."""
    assert 520 * 260 > 512 * 256
    case = Case(False, [4], 2)
    case.add(520, 2, 1, 520, layout='slow')
    run_and_check(case, tag='big')


@pytest.mark.parametrize("max_d", [2, 3, 5, 16])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_max_d_at_and_below_d(mbackend, cplx, max_d):
    """Jobs with d = (5, 3) and (2, 5) under max_d = 2, 3 (below), 5 (at) and 16 (above): the terms with o >= max_d or c >= max_d are
    left out, the coefficient rows stay d_x apart."""
    case = Case(cplx, [7, int(cplx), max_d], 9)
    case.add(3, 5, 3, 64, layout='mid')
    case.add(2, 2, 5, 33, layout='slow')
    run_and_check(case, tag='max_d', max_d=max_d)


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(mbackend, cplx):
    """dtype = 2, max_d = 0 and 17, n_stack = 0, n_out = 0, no output, n_jobs = 65536, a NULL table: TPA_E_BADARG and nothing written;
    n_jobs = 0 and -1: zeros in out[0 : 2 n_stack n_out] and nothing else."""
    L = dev.lib()
    S, K = 3, 2
    case = Case(cplx, [5, int(cplx)], S, n_out=K)
    case.add(3, 2, 2, 64, col=1)
    bh, xh = case.host()
    bb, xb = _Buf(_flat(bh)), _Buf(_flat(xh))
    ob = _Buf(np.full(2 * S * K + 2, SENTINEL))
    jobs = np.array(case.jobs, dtype=np.int64)
    jd, cd = dev.to_device(jobs), dev.to_device(_flat(np.array(case.coeff, dtype=np.complex128 if cplx else np.float64)))
    work = dev.to_device(np.full(int(L.tpa_site_inner_work(1, S, K, 3 * 64)) + 4, SENTINEL))

    def args(n_jobs=1, code=int(cplx), max_d=2, n_stack=S, n_out=K, out=True, jp=True, wp=True):
        return (code, jd.data_ptr() if jp else None, n_jobs, cd.data_ptr(), max_d, n_stack, n_out, 3 * 64, bb.ptr, xb.ptr,
                ob.ptr if out else None, work.data_ptr() if wp else None, dev.stream())
    bad = [args(code=2), args(max_d=0), args(max_d=_lib.MPO_APPLY_MAXD + 1), args(n_stack=0), args(n_out=0), args(out=False),
           args(n_jobs=65536), args(jp=False), args(wp=False), args(n_jobs=0, max_d=0), args(n_jobs=0, n_stack=0)]
    for a in bad:
        assert L.tpa_site_inner_batch(*a) == _lib.E_BADARG, a
    untouched = np.full(2 * S * K + 2, SENTINEL)
    assert np.array_equal(kref.bits(ob.get()), kref.bits(untouched))
    assert np.array_equal(kref.bits(dev.to_host(work)), kref.bits(np.full(work.numel(), SENTINEL)))
    for n_jobs in (0, -1):
        ob.reset()
        assert L.tpa_site_inner_batch(*args(n_jobs=n_jobs)) == 0
        got = ob.get()
        assert np.array_equal(kref.bits(got[:2 * S * K]), kref.bits(np.zeros(2 * S * K)))
        assert np.array_equal(kref.bits(got[2 * S * K:]), kref.bits(np.full(2, SENTINEL)))
    ob.reset()
    assert L.tpa_site_inner_batch(*args()) == 0                 # (the same tables do run)
    got = ob.get()
    assert np.all(got[:2 * S * K:2 * K] == 0) and np.any(got[:2 * S * K] != 0) and np.all(np.isfinite(got[:2 * S * K]))
    assert np.array_equal(kref.bits(got[2 * S * K:]), kref.bits(np.full(2, SENTINEL)))
    assert L.tpa_site_inner_work(0, S, K, 100) == 0 and L.tpa_site_inner_work(2, S, K, 1) == 2 * 2 * S
    assert L.tpa_site_inner_work(2, S, K, 10**9) == 2 * 2 * 512 * S
