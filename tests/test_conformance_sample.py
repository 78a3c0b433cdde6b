"""Conformance of ``tpa_sample_select_batch`` (per row of a stack: Born probabilities, their sequential cdf, the outcome for a given
uniform number and the norm of the chosen slice) and ``tpa_sample_gather_batch`` (chosen slices divided by their norms) with the
extended-precision statement of the header, on the numpy emulation (``mock``) and on the HIP kernels (``gpu``), real and complex, with
the apparatus of ``test_conformance_site_inner.py``: sentinels around every buffer, two launches that must agree bit for bit, the
sources compared bitwise afterwards.

Launch geometry (documented next to the kernels in csrc/tpa_sample.hip): a workgroup of 256 threads (4 wavefronts) takes one row at a
time, grid-stride over the rows with at most 2048 workgroups; thread t sums the items t, t + 256, ... of a slice (seg, c); an ITEM is 16
bytes (one complex element, or two real elements) when x_base is 16-byte aligned and, for real data, post, x_off and x_ld of the seg
are even -- else one real number (decided per seg).  So the edges are: post = 1, 63, 64, 65 (below, at and above a wavefront), 257
(a second pass of the 8-byte form) and 514 (a second pass of the 16-byte form of real data: 257 items), d = 1, 2, 3, 16, dim = 1 and 64,
seg lists of 1 and 4, a group with 0 rows and one with 1 row, n_rows_total = 1, 7, 65, 1000 and 2049 (one more than the grid), x_base 8
bytes off a 16-byte boundary, each of post, x_off, x_ld as the only odd quantity, a padded x_ld.

Bounds (derived; u = 2^-53, gamma_n = n u / (1 - n u)), for an ARBITRARY summation order: p[sigma] is a sum of N = post (2 post for
complex data) non-negative squares, each rounded once (or not at all inside a fused multiply-add) and passing at most N - 1 additions:
|err| <= gamma_{N+1} p.  ``total`` adds the dim values: |err| <= gamma_{N+1+dim} total.  w = sqrt(p): relative error <= gamma_{N+1} / 2
+ u.  sigma must EQUAL the extended-precision choice: every case places its uniform number at least 1e-6 from every exact edge of the
cdf, 1e9 times the error of an edge.  The cases built from powers of two are exact in any order, edges included.

Every run prints a ``CONFORMANCE`` line with its worst err / bound.  With ``TPA_WRITE_PROFILES=1`` the module also writes the worst
figure per group of cases to ``profiles/sample_conformance.txt`` when its last test has run (the committed file is that of a run on
the MI355X; without the variable the tree is left as it is)."""
import os

import numpy as np
import pytest

import kernel_reference as kref
from sample_fixtures import sbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev
from test_conformance_mpo_apply import SENTINEL, _Buf, _flat, _rand

U = 2.0**-53
LD = np.longdouble
MAX_DIM = _lib.SAMPLE_MAX_DIM
WORST = {}          # (backend, group of cases, dtype) -> [cases, worst err / bound]


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    if os.environ.get('TPA_WRITE_PROFILES') != '1' or not WORST:
        return
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sample_conformance.txt')
    lines = ["tpa_sample_select_batch: worst err / bound per group of cases of tests/test_conformance_sample.py",
             "(bounds for an arbitrary summation order: w  gamma_{N+1} / 2 + u,  total  gamma_{N+1+dim},  N = post (2 post complex);",
             " sigma equal to the extended-precision choice and tpa_sample_gather_batch bitwise src / w in every case)", "",
             "%-8s %-14s %-8s %6s  %s" % ("backend", "group", "dtype", "cases", "max err / bound")]
    lines += ["%-8s %-14s %-8s %6d  %.4f" % (k + tuple(v)) for k, v in WORST.items()]
    with open(path, 'w') as f:
        f.write("\n".join(lines) + "\n")


def gamma(n):
    return LD(n) * LD(U) / (1 - LD(n) * LD(U))


class Case:
    """Tables and data of one select launch.  ``group(n_rows, segs)`` puts the rows of one sector behind what is there; a seg is
    ``(d, post, sigma0)`` or a dict with ``lead`` (elements in front of the block) and ``pad`` (elements behind every row) as well."""

    def __init__(self, cplx, seed, dim, gap=2):
        self.cplx, self.dim, self.gap = cplx, dim, gap
        self.rng = np.random.default_rng(seed)
        self.segs, self.groups, self.data = [], [], []
        self.x_len, self.n_rows = gap, 0

    def group(self, n_rows, segs, fill=None):
        first = len(self.segs)
        for s in segs:
            s = dict(d=s[0], post=s[1], sigma0=s[2]) if isinstance(s, tuple) else dict(s)
            d, post = s['d'], s['post']
            x_ld = d * post + s.get('pad', 0)
            x_off = self.x_len + s.get('lead', 0)
            n = max(n_rows, 1) * x_ld
            data = _rand(self.rng, n, self.cplx) if fill is None else np.full(n, fill, dtype=np.complex128 if self.cplx else np.float64)
            self.data.append((x_off, data))
            self.x_len = x_off + n + self.gap
            self.segs.append([x_off, x_ld, d, post, s['sigma0'], 0, 0, 0])
        self.groups.append([first, len(segs), self.n_rows, n_rows])
        self.n_rows += n_rows

    def host(self):
        xh = np.full(self.x_len, np.nan, dtype=np.complex128 if self.cplx else np.float64)
        for off, data in self.data:
            xh[off:off + len(data)] = data
        return xh

    def probabilities(self, xh):
        """(p [rows, dim] in extended precision, N [rows, dim]: the squares behind every p)."""
        p = np.zeros((self.n_rows, self.dim), LD)
        N = np.ones((self.n_rows, self.dim), dtype=np.int64)
        for first, count, r0, nr in self.groups:
            for x_off, x_ld, d, post, sigma0, *_ in self.segs[first:first + count]:
                if nr == 0:
                    continue
                idx = x_off + np.arange(nr)[:, None, None] * x_ld + np.arange(d)[None, :, None] * post + np.arange(post)[None, None, :]
                re, im = kref.split(xh[idx])
                p[r0:r0 + nr, sigma0:sigma0 + d] = np.sum(re * re + im * im, axis=2)
                N[r0:r0 + nr, sigma0:sigma0 + d] = (2 if self.cplx else 1) * post
        return p, N

    @staticmethod
    def choice(p, u):
        """The statement of the header in extended precision: (sigma, total) per row."""
        total = np.zeros(len(p), LD)
        for s in range(p.shape[1]):
            total = total + p[:, s]
        ok = total > 0
        run, count, last = np.zeros(len(p), LD), np.zeros(len(p), dtype=np.int64), np.zeros(len(p), dtype=np.int64)
        safe = np.where(ok, total, LD(1))
        for s in range(p.shape[1]):
            run = run + p[:, s]
            count += (run / safe <= np.asarray(u, dtype=LD))
            last[p[:, s] > 0] = s
        return np.where(ok, np.minimum(count, last), -1), total

    def uniforms(self, p):
        """One uniform number per row, at least 1e-6 (and at least a tenth of the interval) inside the interval of an outcome drawn at
        random among those with p > 1e-4 total."""
        total = np.sum(p, axis=1)
        u = np.zeros(self.n_rows)
        for r in range(self.n_rows):
            if not total[r] > 0:
                u[r] = self.rng.random()
                continue
            cdf = np.cumsum(p[r]) / total[r]
            lo = np.concatenate([[LD(0)], cdf[:-1]])
            wide = np.nonzero(cdf - lo > 1.e-4)[0]
            k = int(self.rng.choice(wide))
            t = 0.1 + 0.8 * self.rng.random()
            u[r] = float(lo[k] + (cdf[k] - lo[k]) * t)
            assert min(u[r] - lo[k], cdf[k] - u[r]) >= 1.e-6 and 0 <= u[r] < 1
        return u


def launch(case, xb, ub, ob, dim=None):
    segs = np.array(case.segs if case.segs else [[0] * 8], dtype=np.int64)
    groups = np.array(case.groups if case.groups else [[0] * 4], dtype=np.int64)
    sd, gd = dev.to_device(segs), dev.to_device(groups)
    dev.check(dev.lib().tpa_sample_select_batch(int(case.cplx), sd.data_ptr(), len(case.segs), gd.data_ptr(), len(case.groups),
                                                case.dim if dim is None else dim, case.n_rows, xb.ptr, ub.ptr, ob.ptr, dev.stream()),
              "sample_select")
    return sd, gd


def run_and_check(case, tag, mis=False, u=None, exact=None):
    """One launch (twice: bit-identical) into an output pre-filled with NaN between sentinels; -> (worst err / bound, out)."""
    xh = case.host()
    p, N = case.probabilities(xh)
    if u is None:
        u = case.uniforms(p)
    xb, ub = _Buf(_flat(xh), mis), _Buf(np.asarray(u, dtype=np.float64))
    ob = _Buf(np.full(4 * case.n_rows, np.nan))
    res = []
    for _ in range(2):
        ob.reset()
        keep = launch(case, xb, ub, ob)
        res.append(ob.get())
        del keep
        assert np.array_equal(kref.bits(xb.get()), kref.bits(_flat(xh))), "x was written"
        assert np.array_equal(kref.bits(ub.get()), kref.bits(np.asarray(u, dtype=np.float64))), "u was written"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_sample_select_batch is not deterministic"
    got = res[0].reshape(case.n_rows, 4)
    assert not np.isnan(got).any(), "an output was not written"
    want_sigma, total = case.choice(p, u)
    assert np.array_equal(got[:, 0].astype(np.int64), want_sigma) and np.all(got[:, 0] == np.round(got[:, 0])), "sigma differs from the extended-precision choice"
    assert np.all(got[:, 3] == 0)
    rows = np.arange(case.n_rows)
    live = want_sigma >= 0
    assert np.all(got[~live, 1] == 0)
    worst = 0.
    if np.any(live):
        sg = want_sigma[live]
        p_sel, n_sel = p[rows[live], sg], N[rows[live], sg]
        w_ld = np.sqrt(p_sel)
        lim_w = (gamma(n_sel + 1) / 2 + LD(U)) * w_ld
        err_w = np.abs(got[live, 1] - w_ld)
        n_tot = np.max(N, axis=1)[live] + 1 + case.dim
        lim_t = gamma(n_tot) * total[live]
        err_t = np.abs(got[live, 2] - total[live])
        if exact:       # (p and total exactly; w = sqrt(p) rounded once)
            assert np.all(err_t == 0) and np.all(err_w <= LD(U) * w_ld), "a case of powers of two is not exact"
        else:
            worst = float(max(np.max(err_w / lim_w), np.max(err_t / lim_t)))
            assert np.all(err_w <= lim_w) and np.all(err_t <= lim_t), "worst err / bound = %.3g" % worst
    print("CONFORMANCE tpa_sample_select_batch(%s) %s rows=%d segs=%d groups=%d dim=%d%s max_err_over_bound=%.4f"
          % (tag, 'complex' if case.cplx else 'real', case.n_rows, len(case.segs), len(case.groups), case.dim, ' mis' if mis else '', worst))
    ent = WORST.setdefault(('mock' if hasattr(dev.lib(), 'real') else 'gpu', tag, 'complex' if case.cplx else 'real'), [0, 0.])
    ent[0], ent[1] = ent[0] + 1, max(ent[1], worst)
    return worst, got


CPLX = pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])


@pytest.mark.parametrize("post", [1, 63, 64, 65, 257, 514])
@CPLX
def test_post_and_d(sbackend, cplx, post):
    """Every post with d = 1, 2, 3, 16 in one group of 7 rows (seg list of 4, dim = 22), at even offsets (even post: the 16-byte form
    of real data) and, second case, with the blocks one element further on (its 8-byte form)."""
    for lead in (0, 1):
        case = Case(cplx, [1, int(cplx), post, lead], 22)
        case.group(7, [dict(d=1, post=post, sigma0=0, lead=lead), dict(d=2, post=post, sigma0=1), dict(d=3, post=post, sigma0=3),
                       dict(d=16, post=post, sigma0=6)])
        run_and_check(case, 'shape')


@pytest.mark.parametrize("n_rows", [1, 7, 65, 1000, 2049])
@CPLX
def test_rows_groups_and_dim(sbackend, cplx, n_rows):
    """n_rows_total = 1, 7, 65, 1000, 2049 (one more than the capped grid: a workgroup takes a second row) split over groups with a
    seg list of 1 and of 4, among them a group with 0 rows and one with 1 row; dim = TPA_SAMPLE_MAX_DIM with sigmas that no seg
    covers, and dim = 1."""
    case = Case(cplx, [2, int(cplx), n_rows], MAX_DIM, gap=3)
    a = (n_rows - 1) // 2
    case.group(a, [(16, 5, 48)])
    case.group(0, [(2, 4, 0)])
    case.group(1, [(1, 6, 0), (3, 6, 1), (16, 6, 20), (2, 6, 62)])
    case.group(n_rows - 1 - a, [(MAX_DIM, 2, 0)])
    assert case.n_rows == n_rows
    run_and_check(case, 'rows')
    one = Case(cplx, [3, int(cplx), n_rows], 1)
    one.group(min(n_rows, 65), [(1, 9, 0)])
    _, got = run_and_check(one, 'rows')
    assert np.all(got[:, 0] == 0)


@pytest.mark.parametrize("odd", ['post', 'x_off', 'x_ld', 'none'])
@pytest.mark.parametrize("mis", [False, True], ids=['aligned', 'mis'])
@CPLX
def test_alignment_and_a_single_odd_quantity(sbackend, cplx, mis, odd):
    """x_base on and 8 bytes off a 16-byte boundary; a seg whose ONLY odd quantity is post (d = 2: x_ld stays even), x_off or x_ld
    (a padded x_ld), next to an all-even seg with a padded x_ld: for real data that quantity alone sends the seg to the 8-byte form."""
    case = Case(cplx, [4, int(cplx), int(mis), ['post', 'x_off', 'x_ld', 'none'].index(odd)], 6, gap=2)
    post = 65 if odd == 'post' else 66
    case.group(5, [dict(d=2, post=post, sigma0=0, lead=int(odd == 'x_off'), pad=int(odd == 'x_ld')), dict(d=4, post=64, sigma0=2, pad=2)])
    x_off, x_ld, _, post_s = case.segs[0][:4]
    assert [n for n, v in zip(('post', 'x_off', 'x_ld'), (post_s, x_off, x_ld)) if v % 2] == ([] if odd == 'none' else [odd])
    run_and_check(case, 'mis' if mis else 'odd_' + odd, mis=mis)


def _exact_case(cplx, rows_of_slices, dim, segs):
    """One group whose rows are given slice by slice as lists of numbers (post = 2); ``segs`` = [(d, sigma0)]."""
    case = Case(cplx, [5], dim)
    n = len(rows_of_slices)
    case.group(n, [(d, 2, s0) for d, s0 in segs], fill=0.)
    xh = case.host()
    for r, slices in enumerate(rows_of_slices):
        k = 0
        for x_off, x_ld, d, post, *_ in case.segs:
            for c in range(d):
                a, b = slices[k]
                xh[x_off + r * x_ld + c * post: x_off + r * x_ld + (c + 1) * post] = (1j * a, b) if cplx else (a, b)
                k += 1
    case.data = [(0, xh)]
    case.x_len = len(xh)
    return case


@CPLX
def test_exact_cases_of_powers_of_two(sbackend, cplx):
    """All sums exact in any order.  p = (1/4, 1/4, 1/2): u = 1/4 lies ON the first edge and gives sigma = 1 (``side='right'``);
    p = (0, 1/2, 1/2) with u = 0 skips sigma = 0; u = 1 - 2^-53 gives the last sigma with p > 0 although a sigma with p = 0 follows
    (and so does u = 1, outside the contract of the caller but inside the formula); a row of zeros gives sigma = -1, w = 0."""
    q, h, z = (.5, 0.), (.5, .5), (0., 0.)
    case = _exact_case(cplx, [[q, q, h, z], [z, h, h, z], [q, q, h, z], [q, q, h, z], [z, z, z, z], [q, q, h, z]], 4, [(4, 0)])
    u = [0.25, 0., 1. - 2.**-53, 1., 0.3, 0.5]
    _, got = run_and_check(case, 'exact', u=u, exact=True)
    assert got[:, 0].tolist() == [1, 1, 2, 2, -1, 2]
    assert got[0, 1] == .5 and got[4, 1] == 0.
    assert got[:, 2].tolist() == [1., 1., 1., 1., 0., 1.]


@CPLX
def test_a_sigma_without_a_seg_is_never_chosen(sbackend, cplx):
    """dim = 4, segs for sigma = 0 and sigma = 2, 3: p = (1/4, 0, 1/4, 1/2) exactly.  u = 1/4 lies on the edges of sigma = 0 AND of the
    uncovered sigma = 1 and gives sigma = 2; no u gives 1."""
    q, h = (.5, 0.), (.5, .5)
    us = [0., 0.2, 0.25, 0.4, 0.5, 0.75, 1. - 2.**-53]
    case = _exact_case(cplx, [[q, q, h]] * len(us), 4, [(1, 0), (2, 2)])
    _, got = run_and_check(case, 'exact', u=us, exact=True)
    assert got[:, 0].tolist() == [0, 0, 2, 2, 3, 3, 3]
    assert got[:, 2].tolist() == [1.] * len(us)


@CPLX
def test_rows_outside_every_group(sbackend, cplx):
    """n_rows_total = 5 with groups for the rows 1 .. 3 only: the rows 0 and 4 get {-1, 0, 0, 0}."""
    case = Case(cplx, [6, int(cplx)], 3)
    case.n_rows = 1
    case.group(3, [(3, 5, 0)])
    case.n_rows = 5
    xh = case.host()
    xb, ub, ob = _Buf(_flat(xh)), _Buf(np.full(5, 0.5)), _Buf(np.full(20, np.nan))
    keep = launch(case, xb, ub, ob)
    got = ob.get().reshape(5, 4)
    del keep
    assert got[0].tolist() == [-1, 0, 0, 0] and got[4].tolist() == [-1, 0, 0, 0]
    assert np.all(got[1:4, 0] >= 0) and np.all(got[1:4, 1] > 0) and np.all(got[1:4, 2] > 0)


@CPLX
def test_select_arguments(sbackend, cplx):
    """dtype = 2, dim = 0 and TPA_SAMPLE_MAX_DIM + 1, negative table sizes, a NULL pointer: TPA_E_BADARG and nothing written;
    n_rows_total = 0 and -1: 0 and nothing written; the same tables do run."""
    L = dev.lib()
    case = Case(cplx, [7, int(cplx)], 4)
    case.group(3, [(4, 8, 0)])
    xh = case.host()
    xb, ub, ob = _Buf(_flat(xh)), _Buf(np.full(3, 0.5)), _Buf(np.full(12 + 2, SENTINEL))
    sd, gd = dev.to_device(np.array(case.segs, dtype=np.int64)), dev.to_device(np.array(case.groups, dtype=np.int64))

    def args(code=int(cplx), n_segs=1, n_groups=1, dim=4, n_rows=3, sp=True, gp=True, xp=True, up=True, op=True):
        return (code, sd.data_ptr() if sp else None, n_segs, gd.data_ptr() if gp else None, n_groups, dim, n_rows, xb.ptr if xp else None,
                ub.ptr if up else None, ob.ptr if op else None, dev.stream())
    bad = [args(code=2), args(dim=0), args(dim=MAX_DIM + 1), args(n_segs=-1), args(n_groups=-1), args(sp=False), args(gp=False),
           args(xp=False), args(up=False), args(op=False), args(n_rows=0, dim=0), args(n_rows=-1, code=3)]
    for a in bad:
        assert L.tpa_sample_select_batch(*a) == _lib.E_BADARG, a
    for n_rows in (0, -1):
        assert L.tpa_sample_select_batch(*args(n_rows=n_rows)) == 0
        assert L.tpa_sample_select_batch(*args(n_rows=n_rows, sp=False, op=False)) == 0
    assert np.array_equal(kref.bits(ob.get()), kref.bits(np.full(14, SENTINEL)))
    assert L.tpa_sample_select_batch(*args()) == 0
    got = ob.get()
    assert np.all(np.isfinite(got[:12])) and np.all(got[:12:4] >= 0) and np.array_equal(kref.bits(got[12:]), kref.bits(np.full(2, SENTINEL)))


def _gather_case(cplx, seed, lens, mis_src=False, mis_dst=False):
    """Rows of the lengths ``lens`` at odd and even offsets of src, written to dst in permuted order with gaps, ``out_row`` a
    permutation that differs from the row index; -> (rows, src, out table, dst length)."""
    rng = np.random.default_rng(seed)
    n = len(lens)
    src_off, pos = [], 1
    for ln in lens:
        src_off.append(pos)
        pos += ln + int(rng.integers(0, 3))
    src = _rand(rng, pos + 1, cplx)
    order = rng.permutation(n)
    dst_off, dpos = np.zeros(n, dtype=np.int64), 0
    for k in order:
        dpos += int(rng.integers(0, 3))
        dst_off[k] = dpos
        dpos += lens[k]
    out_row = (np.arange(n) * 7 + 3) % (n + 2)      # (n + 2 rows of the out table; 7 and n + 2 share no factor for the n used here)
    assert len(set(out_row.tolist())) == n and np.any(out_row != np.arange(n))
    out = np.zeros((n + 2, 4))
    out[:, 0], out[:, 1], out[:, 2] = rng.integers(0, 4, n + 2), 0.25 + rng.random(n + 2), 1.
    rows = np.stack([np.array(src_off), np.array(lens), dst_off, out_row], axis=1).astype(np.int64)
    return rows, src, out, dpos + 1


@pytest.mark.parametrize("mis", ['none', 'src', 'dst', 'both'])
@CPLX
def test_gather_is_a_true_division(sbackend, cplx, mis):
    """dst = src / w bit for bit (component by component for complex data) for len = 1, 2, 65 and a row of 300 (more than one pass of a
    wavefront), odd offsets, dst rows in permuted order, out_row != the row index; a row with len = 0 writes nothing; everything
    between the rows of dst keeps its contents; src and out are unchanged; either base 8 bytes off a 16-byte boundary."""
    lens = [1, 2, 65, 0, 300, 2, 1, 64, 3]
    rows, src, out, n_dst = _gather_case(cplx, [8, int(cplx)], lens)
    cw = 2 if cplx else 1
    sb, ob = _Buf(_flat(src), mis in ('src', 'both')), _Buf(out.reshape(-1))
    db = _Buf(np.full(cw * n_dst, SENTINEL), mis in ('dst', 'both'))
    rd = dev.to_device(rows)
    want = np.full(cw * n_dst, SENTINEL)
    for s_off, ln, d_off, o_row in rows.tolist():
        want[cw * d_off: cw * (d_off + ln)] = _flat(src)[cw * s_off: cw * (s_off + ln)] / out[o_row, 1]
    res = []
    for _ in range(2):
        db.reset()
        dev.check(dev.lib().tpa_sample_gather_batch(int(cplx), rd.data_ptr(), len(rows), sb.ptr, ob.ptr, db.ptr, dev.stream()), "sample_gather")
        res.append(db.get())
        assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src))) and np.array_equal(kref.bits(ob.get()), kref.bits(out.reshape(-1)))
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1]))
    assert np.array_equal(kref.bits(res[0]), kref.bits(want)), "tpa_sample_gather_batch is not bitwise src / w"
    print("CONFORMANCE tpa_sample_gather_batch %s rows=%d mis=%s bitwise" % ('complex' if cplx else 'real', len(rows), mis))
    ent = WORST.setdefault(('mock' if hasattr(dev.lib(), 'real') else 'gpu', 'gather', 'complex' if cplx else 'real'), [0, 0.])
    ent[0] += 1


@CPLX
def test_gather_arguments(sbackend, cplx):
    """dtype = 2, a NULL pointer, src_base == dst_base: TPA_E_BADARG and nothing written; n_rows = 0 and -1: 0 and nothing written."""
    L = dev.lib()
    rows, src, out, n_dst = _gather_case(cplx, [9, int(cplx)], [3, 5])
    cw = 2 if cplx else 1
    sb, ob, db = _Buf(_flat(src)), _Buf(out.reshape(-1)), _Buf(np.full(cw * n_dst, SENTINEL))
    rd = dev.to_device(rows)

    def args(code=int(cplx), n=2, rp=True, sp=True, op=True, dp=True, same=False):
        return (code, rd.data_ptr() if rp else None, n, sb.ptr if sp else None, ob.ptr if op else None,
                (sb.ptr if same else db.ptr) if dp else None, dev.stream())
    for a in (args(code=2), args(rp=False), args(sp=False), args(op=False), args(dp=False), args(same=True), args(code=-1, n=0)):
        assert L.tpa_sample_gather_batch(*a) == _lib.E_BADARG, a
    for n in (0, -1):
        assert L.tpa_sample_gather_batch(*args(n=n)) == 0 and L.tpa_sample_gather_batch(*args(n=n, rp=False, dp=False)) == 0
    assert np.array_equal(kref.bits(db.get()), kref.bits(np.full(cw * n_dst, SENTINEL)))
    assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src)))
    assert L.tpa_sample_gather_batch(*args()) == 0
    assert np.any(db.get() != SENTINEL)
