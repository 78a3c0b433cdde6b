"""Conformance of ``tpa_site_rho_batch`` (out[s, e] = sum over the jobs whose tile holds e of sum_{i, j} conj(b[i, o, j]) x[s; i, c, j])
with the extended-precision statement of the header, on the numpy emulation (``mock``) and on the HIP kernel (``gpu``), real and
complex, with the apparatus of ``test_conformance_site_inner.py``: sentinels around every buffer, two launches that must agree bit for
bit, the sources compared bitwise afterwards.

Launch geometry (documented next to the kernel in csrc/tpa_site_rho.hip): a thread owns columns (i, item of j) of a job; per group of S
stack slots it loads the d_b items of b and streams the d_x items of x of every slot into S D D accumulators, D = 1, 2 or 4 the smallest
that holds max_d and S = 8, 4, 2; an ITEM is 16 bytes (one complex element, or two real elements of one row) when b_base and x_base are
16-byte aligned and, for real data, post, b_off, b_ld, x_off, x_ld and x_sstride of the job are even -- else one element (decided per
job).  256 threads per workgroup, grid (min(256, ceil(items of max_job_cols / 1024)), n_jobs), grid-stride over the columns.  So the
edges are: d_b != d_x out of {1, 2, 3, 4}, max_d at and above a job's d, n_stack = 1, S - 1, S, S + 1 and 65 for every D, post = 64, 65,
6, 1 and pre = 0, 1, 3, the stack index slowest and between i and c, each parity quantity as the only odd one, each base 8 bytes off a
16-byte boundary, two jobs on one output tile, a tile without a job, b aliasing x, a job with several columns per thread.

Bound (derived; u = 2^-53), for an ARBITRARY summation order: out[s, e] is a sum of N = sum_{jobs on e} pre post products conj(b) x.
Real data: a product is rounded at most once (a multiplication, or none inside a fused multiply-add) and passes at most N - 1 additions
whatever the order and the grouping (lanes, wavefronts, partials, second pass), plus the rounding of the fused multiply-add that holds
it: |err| <= gamma_n sum |b| |x| with n = N + 1, gamma_n = n u / (1 - n u).  Complex data: a component of the result is a sum of 2 N
real products whose magnitude sum is below sum (|b_re| + |b_im|)(|x_re| + |x_im|): n = 4 (N + 1) covers it with the factor 4 of the
sibling tests.  This is the site-inner derivation without the coefficient factor.  Entries without a job, and F64's imaginary parts:
exact zeros.

Every run prints a ``CONFORMANCE`` line with its worst err / bound.  With ``TPA_WRITE_PROFILES=1`` the module also writes the worst
figure per group of cases to ``profiles/site_rho_conformance.txt`` when its last test has run (the committed file is that of a run on
the MI355X; without the variable the tree is left as it is)."""
import os

import numpy as np
import pytest

import kernel_reference as kref
from rho_fixtures import rbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble
SLOTS = {1: 8, 2: 4, 4: 2}          # D -> S (csrc/tpa_site_rho.hip)

WORST = {}          # (backend, group of cases, dtype) -> [cases, worst err / bound]


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    if os.environ.get('TPA_WRITE_PROFILES') != '1' or not WORST:
        return
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'site_rho_conformance.txt')
    lines = ["tpa_site_rho_batch: worst err / bound per group of cases of tests/test_conformance_site_rho.py",
             "(bound: gamma_n sum |b| |x| for an arbitrary summation order, n = N + 1 real, 4 (N + 1) complex)", "",
             "%-8s %-14s %-8s %6s  %s" % ("backend", "group", "dtype", "cases", "max err / bound")]
    lines += ["%-8s %-14s %-8s %6d  %.4f" % (k + tuple(v)) for k, v in WORST.items()]
    with open(path, 'w') as f:
        f.write("\n".join(lines) + "\n")


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one launch.  ``add(pre, d_b, d_x, post, ob, cx, layout, ...)`` puts a block pair behind what is there, its
    tile at row ``ob`` and column ``cx`` of the ``d x d`` matrix of a slot; with ``alias`` the b blocks lie in the x buffer."""

    def __init__(self, cplx, seed, n_stack, d=4, gap=2, alias=False):
        self.cplx, self.gap, self.n_stack, self.d, self.alias = cplx, gap, n_stack, d, alias
        self.out_size = d * d
        self.rng = np.random.default_rng(seed)
        self.jobs = []
        self.b_len, self.x_len = gap, gap
        self.b_data, self.x_data = [], []

    def add(self, pre, d_b, d_x, post, ob=0, cx=0, layout='mid', b_lead=0, b_pad=0, x_lead=0, x_pad=0, s_pad=0):
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
        self.jobs.append([b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, ob * self.d + cx, self.d, 0])

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
        """(re, im, magnitude sum, number of products) per output (s, e) in extended precision."""
        S, E = self.n_stack, self.out_size
        re, im, mag = np.zeros((S, E), LD), np.zeros((S, E), LD), np.zeros((S, E), LD)
        count = np.zeros(E, dtype=np.int64)
        ss = np.arange(S)[:, None, None]
        for b_off, b_ld, d_b, x_off, x_ld, x_ss, d_x, pre, post, out_off, out_ld, _ in self.jobs:
            if min(pre, post, d_b, d_x) <= 0:
                continue
            nb, nx = min(d_b, max_d), min(d_x, max_d)
            ii, jj = np.arange(pre)[:, None], np.arange(post)[None, :]
            for o in range(nb):
                br, bi = kref.split(bh[b_off + ii * b_ld + o * post + jj])                          # (pre, post)
                for c in range(nx):
                    e = out_off + o * out_ld + c
                    assert 0 <= e < E
                    xr, xi = kref.split(xh[x_off + ii[None] * x_ld + ss * x_ss + c * post + jj[None]])      # (S, pre, post)
                    count[e] += pre * post
                    re[:, e] += np.sum(br[None] * xr + bi[None] * xi, axis=(1, 2))
                    im[:, e] += np.sum(br[None] * xi - bi[None] * xr, axis=(1, 2))
                    mag[:, e] += np.sum((np.abs(br) + np.abs(bi))[None] * (np.abs(xr) + np.abs(xi)), axis=(1, 2))
        return re, im, mag, count


def _tables(case):
    jobs = np.array(case.jobs, dtype=np.int64).reshape(-1, 12)
    return jobs, max(int(np.max(jobs[:, 7] * jobs[:, 8])), 1)


def launch(case, max_d, bb, xb, ob, work):
    jobs, max_cols = _tables(case)
    jd = dev.to_device(jobs)
    need = dev.lib().tpa_site_rho_work(len(jobs), case.n_stack, case.out_size, max_cols)
    assert need <= work.numel()
    dev.check(dev.lib().tpa_site_rho_batch(int(case.cplx), jd.data_ptr(), len(jobs), max_d, case.n_stack, case.out_size, max_cols,
                                           bb.ptr, xb.ptr, ob.ptr, work.data_ptr(), dev.stream()), "site_rho")
    return jd


def run_and_check(case, mis=None, tag='', max_d=None):
    """One launch (twice: bit-identical) into an output pre-filled with NaN between sentinels; -> worst err / bound."""
    cplx = case.cplx
    bh, xh = case.host()
    xb = _Buf(_flat(xh), mis == 'x')
    bb = xb if case.alias else _Buf(_flat(bh), mis == 'b')
    if max_d is None:
        max_d = max(max(j[2], j[6]) for j in case.jobs)
    S, E = case.n_stack, case.out_size
    ob = _Buf(np.full(2 * S * E, np.nan))
    jobs, max_cols = _tables(case)
    n_work = int(dev.lib().tpa_site_rho_work(len(jobs), S, E, max_cols))
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
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_site_rho_batch is not deterministic"
    got = res[0].reshape(S, E, 2)
    assert not np.isnan(got).any(), "an output was not written"
    re, im, mag, count = case.reference(bh, xh, max_d)
    worst = 0.
    for e in range(E):
        if count[e] == 0:
            assert np.array_equal(kref.bits(got[:, e]), kref.bits(np.zeros((S, 2)))), "an entry without a job is not zero"
            continue
        lim = gamma((4 if cplx else 1) * (int(count[e]) + 1)) * mag[:, e]
        err_r, err_i = np.abs(got[:, e, 0] - re[:, e]), np.abs(got[:, e, 1] - im[:, e])
        if not cplx:
            assert np.array_equal(kref.bits(got[:, e, 1]), kref.bits(np.zeros(S))), "imaginary part of real data"
        ratio = float(max(np.max(err_r / np.maximum(lim, LD(1e-300))), np.max(err_i / np.maximum(lim, LD(1e-300)))))
        assert np.all(err_r <= lim) and np.all(err_i <= lim), "entry %d: worst err / bound = %.3g" % (e, ratio)
        worst = max(worst, ratio)
    print("CONFORMANCE tpa_site_rho_batch(%s) %s jobs=%d n_stack=%d d=%d max_d=%d%s%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(case.jobs), S, case.d, max_d, ' mis=' + mis if mis else '', ' alias' if case.alias else '',
             worst))
    ent = WORST.setdefault(('mock' if hasattr(dev.lib(), 'real') else 'gpu', tag, 'complex' if cplx else 'real'), [0, 0.])
    ent[0], ent[1] = ent[0] + 1, max(ent[1], worst)
    assert worst <= 1
    return worst, got


# (D, the d pairs of its cases): D = 1 has d_b = d_x = 1 only; max_d = D is at (or above) every d of the case
D_PAIRS = {1: [(1, 1)], 2: [(1, 2), (2, 1)], 4: [(1, 2), (2, 3), (3, 2), (3, 4), (4, 3), (1, 4), (4, 1)]}
STACKS = [(D, n) for D, S in SLOTS.items() for n in sorted({1, S - 1, S, S + 1, 65})]


@pytest.mark.parametrize("D,n_stack", STACKS, ids=["D%d-n%d" % t for t in STACKS])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(rbackend, cplx, D, n_stack):
    """d_b != d_x out of {1, 2, 3, 4}, post = 64, 65, 6, 1, pre = 0, 1, 3, both stack layouts, everything at even offsets (even post:
    the 16-byte form of real data) and at odd ones (its 8-byte form); n_stack below, at and above a group of S slots and 65; two
    tiles per launch, the rest of the 4 x 4 matrix without a job."""
    for n, (post, pre, gap) in enumerate(((64, 3, 2), (65, 1, 3), (6, 3, 2), (1, 3, 3), (64, 0, 2))):
        for m, (d_b, d_x) in enumerate(D_PAIRS[D]):
            if n_stack == 65 and (m + n) % 3:       # (many groups: a third of the combinations, every post and every d among them)
                continue
            case = Case(cplx, [1, int(cplx), post, n_stack, d_b, d_x], n_stack, gap=gap)
            case.add(pre, d_b, d_x, post, ob=0, cx=4 - d_x, layout='mid' if (n + m) % 2 else 'slow')
            case.add(1, d_x, d_b, post, ob=4 - d_x, cx=0, layout='slow' if (n + m) % 2 else 'mid', x_pad=gap, s_pad=gap, b_pad=gap)
            run_and_check(case, tag='shape_D%d' % D, max_d=D)


@pytest.mark.parametrize("mis", ['b', 'x'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(rbackend, cplx, mis):
    """b_base / x_base one real element off a 16-byte boundary, with an even and an odd post."""
    for post in (64, 65):
        case = Case(cplx, [2, int(cplx), post], 5)
        case.add(3, 2, 3, post, ob=0, cx=0, layout='mid')
        case.add(3, 3, 2, post, ob=1, cx=2, layout='slow')
        run_and_check(case, mis=mis, tag='mis')


ODD = ['post', 'b_off', 'b_ld', 'x_off', 'x_ld', 'x_sstride']


@pytest.mark.parametrize("layout", ['mid', 'slow'])
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_a_single_odd_quantity(rbackend, cplx, odd, layout):
    """A job whose ONLY odd quantity is post, b_off, b_ld, x_off, x_ld or x_sstride: everything else is even, so for real data that
    quantity alone sends the job to the 8-byte form.  (Odd post: d_b = d_x = 2 and pre = 2 keep every stride even.)"""
    S = 4
    case = Case(cplx, [6, int(cplx), ODD.index(odd), layout == 'mid'], S, d=2, gap=2)
    post = 65 if odd == 'post' else 64
    kw = dict(b_lead=int(odd == 'b_off'), b_pad=int(odd == 'b_ld'), x_lead=int(odd == 'x_off'))
    if layout == 'mid':         # x_ld = S (x_ss) + x_pad
        kw.update(s_pad=int(odd == 'x_sstride'), x_pad=int(odd == 'x_ld'))      # (S = 4 slots: x_ld stays even)
    else:                       # x_ss = pre x_ld + s_pad
        kw.update(x_pad=int(odd == 'x_ld'), s_pad=int(odd == 'x_sstride'))
    case.add(2, 2, 2, post, layout=layout, **kw)
    b_off, b_ld, _, x_off, x_ld, x_ss, _, _, post_j, _, _, _ = case.jobs[0]
    odd_ones = [n for n, v in zip(ODD, (post_j, b_off, b_ld, x_off, x_ld, x_ss)) if v % 2]
    assert odd_ones == [odd], odd_ones
    run_and_check(case, tag='odd_' + odd)


@pytest.mark.parametrize("alias", [False, True], ids=['apart', 'alias'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_tiles_jobs_and_alias(rbackend, cplx, alias):
    """Three jobs on the tile at (0, 0) (one of them with pre = 0, two of different extents: the entries both cover get both), one
    job on the tile at (2, 1), the other entries of the 4 x 4 matrix none (exact zeros); with ``alias`` b and x are one buffer."""
    case = Case(cplx, [3, int(cplx), alias], 5, alias=alias)
    case.add(3, 2, 3, 64, ob=0, cx=0, layout='mid')
    case.add(2, 2, 2, 33, ob=0, cx=0, layout='slow', x_pad=1)
    case.add(0, 2, 2, 64, ob=0, cx=0)
    case.add(3, 1, 2, 65, ob=2, cx=1, layout='slow')
    _, got = run_and_check(case, tag='jobs')
    got = got.reshape(5, 4, 4, 2)
    assert np.all(got[:, 3] == 0) and np.all(got[:, 2, 0] == 0) and np.all(got[:, 0, 3] == 0) and np.all(got[:, 0, 0, 0] != 0)


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_one_site_density_matrix(rbackend, cplx):
    """x = b = theta with n_stack = 1 (no stack: x_sstride = 0): out[p', p] = rho[p, p'] -- Hermitian with a real diagonal, here of two
    sectors of widths 1 and 2 on a leg of three states."""
    case = Case(cplx, [8, int(cplx)], 1, d=3, alias=True)
    rng = np.random.default_rng(9)
    for d_s, p0 in ((1, 0), (2, 1)):
        pre, post = 5, 6
        off = case.x_len
        case.x_data.append((off, _rand(rng, pre * d_s * post, cplx)))
        case.x_len = off + pre * d_s * post + case.gap
        case.jobs.append([off, d_s * post, d_s, off, d_s * post, 0, d_s, pre, post, p0 * 3 + p0, 3, 0])
    _, got = run_and_check(case, tag='one_site')
    m = (got[0, :, 0] + 1j * got[0, :, 1]).reshape(3, 3)
    assert np.max(np.abs(m - m.conj().T)) < 1e-13 and np.all(np.diag(m).real > 0) and np.all(m[0, 1:] == 0)


def test_job_beyond_the_grid(rbackend):
    """One real job with pre = post = 520, n_stack = 2: 520 * 260 items of 16 bytes over the 256 workgroups of the capped grid (more
    than one column per thread: the grid-stride loop runs)."""
    assert 520 * 260 > 256 * 256
    case = Case(False, [4], 2, d=2)
    case.add(520, 2, 1, 520, layout='slow')
    run_and_check(case, tag='big')


@pytest.mark.parametrize("max_d", [1, 2, 3, 4])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_max_d_at_above_and_below_d(rbackend, cplx, max_d):
    """Jobs with d = (3, 2) and (2, 3) under max_d = 1, 2 (below: the terms with o >= max_d or c >= max_d are left out), 3 (at) and 4
    (above)."""
    case = Case(cplx, [7, int(cplx), max_d], 5)
    case.add(3, 3, 2, 64, ob=0, cx=0, layout='mid')
    case.add(2, 2, 3, 33, ob=1, cx=1, layout='slow')
    run_and_check(case, tag='max_d', max_d=max_d)


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(rbackend, cplx):
    """dtype = 2, max_d = 0 and 5 (sectors wider than 4 are not served), n_stack = 0, out_size = 0, no output, n_jobs = 65536, a NULL
    table: TPA_E_BADARG and nothing written; n_jobs = 0 and -1: zeros in out[0 : 2 n_stack out_size] and nothing else."""
    L = dev.lib()
    S, E = 3, 4
    case = Case(cplx, [5, int(cplx)], S, d=2)
    case.add(3, 2, 1, 64, ob=0, cx=1)
    bh, xh = case.host()
    bb, xb = _Buf(_flat(bh)), _Buf(_flat(xh))
    ob = _Buf(np.full(2 * S * E + 2, SENTINEL))
    jobs = np.array(case.jobs, dtype=np.int64)
    jd = dev.to_device(jobs)
    work = dev.to_device(np.full(int(L.tpa_site_rho_work(1, S, E, 3 * 64)) + 4, SENTINEL))

    def args(n_jobs=1, code=int(cplx), max_d=2, n_stack=S, out_size=E, out=True, jp=True, wp=True):
        return (code, jd.data_ptr() if jp else None, n_jobs, max_d, n_stack, out_size, 3 * 64, bb.ptr, xb.ptr,
                ob.ptr if out else None, work.data_ptr() if wp else None, dev.stream())
    bad = [args(code=2), args(max_d=0), args(max_d=_lib.SITE_RHO_MAXD + 1), args(n_stack=0), args(out_size=0), args(out=False),
           args(n_jobs=65536), args(jp=False), args(wp=False), args(n_jobs=0, max_d=0), args(n_jobs=0, n_stack=0)]
    for a in bad:
        assert L.tpa_site_rho_batch(*a) == _lib.E_BADARG, a
    untouched = np.full(2 * S * E + 2, SENTINEL)
    assert np.array_equal(kref.bits(ob.get()), kref.bits(untouched))
    assert np.array_equal(kref.bits(dev.to_host(work)), kref.bits(np.full(work.numel(), SENTINEL)))
    for n_jobs in (0, -1):
        ob.reset()
        assert L.tpa_site_rho_batch(*args(n_jobs=n_jobs)) == 0
        got = ob.get()
        assert np.array_equal(kref.bits(got[:2 * S * E]), kref.bits(np.zeros(2 * S * E)))
        assert np.array_equal(kref.bits(got[2 * S * E:]), kref.bits(np.full(2, SENTINEL)))
    ob.reset()
    assert L.tpa_site_rho_batch(*args()) == 0                 # (the same tables do run)
    got = ob.get()
    tile = got[:2 * S * E].reshape(S, 2, 2, 2)
    assert np.all(tile[:, :, 0] == 0) and np.all(tile[:, :, 1, 0] != 0) and np.all(np.isfinite(got[:2 * S * E]))
    assert np.array_equal(kref.bits(got[2 * S * E:]), kref.bits(np.full(2, SENTINEL)))
    assert L.tpa_site_rho_work(0, S, E, 100) == 0 and L.tpa_site_rho_work(2, S, E, 1) == 2 * 2 * S * E
    assert L.tpa_site_rho_work(2, S, 25, 10**9) == 2 * 2 * 256 * S * 16
