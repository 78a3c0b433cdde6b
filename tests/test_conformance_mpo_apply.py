"""Conformance of ``tpa_mpo_apply_batch`` (dst slab (pre, d_out, post) = sum_t M_t on the middle index of src_t slab (pre, d_in_t, post))
with the extended-precision statement of the header, on the numpy emulation (``mock``) and on the HIP kernel (``gpu``), real and
complex, in the style of ``test_conformance_project.py``.

Launch geometry (documented next to the kernel in csrc/tpa_copy.hip and repeated by ``geometry`` below).  A thread owns one column
(i, item of j) of a job and keeps d_out accumulators; an ITEM is 16 bytes (one complex element, or two real elements of one row) when
src_base and dst_base are 16-byte aligned and, for real data, post, dst_off and every src_off of the job are even -- else one element
(decided per job).  The kernel is compiled for D = 2, 4, 8, 16 accumulators: the smallest D >= max_d.  256 threads per workgroup,
grid (min(512, ceil(max_job_elems / (256 max_d))), n_jobs), grid-stride over the columns.  So the edges are: post = 1, one wavefront
(63, 64, 65), more than a workgroup (257), odd post (real: 8-byte form), a base 8 bytes off a 16-byte boundary, d at and between the
compiled sizes, jobs of very different size under one grid, and a job with more columns than 512 * 256 threads.

Bound (derived; EPS = 2^-52 = 2 u).  A component of dst is one chain of sum_t d_in_t (real) or 2 sum_t d_in_t (complex) fused
multiply-adds, so a term is rounded at most that often:  |err| <= R (sum_t d_in_t + 1) EPS sum |coeff| |x|  per component, R = 1 real,
2 complex (the emulation adds rounded products in the same order: the same bound holds).  term_count = 0: exact zeros."""
import numpy as np
import pytest

import kernel_reference as kref
from mpo_apply_fixtures import bbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

EPS = 2.0**-52
LD = np.longdouble
GUARD = 4                   # doubles in front of and behind every payload (even: the payload keeps its alignment)
SENTINEL = -7.25e300
CAP = 512 * 256             # threads of the capped grid of one job


def geometry(cplx, max_d, max_elems, job, src_offs, misaligned):
    """(D, 16-byte form for this job, workgroups per job) of the module docstring; job = (dst_off, pre, d_out, post)."""
    D = next(d for d in (2, 4, 8, 16) if d >= max_d)
    dst_off, pre, d_out, post = job
    vec = not misaligned and (cplx or (post % 2 == 0 and dst_off % 2 == 0 and all(o % 2 == 0 for o in src_offs)))
    g = min(512, max(1, -(-(max_elems // max_d) // 256)))
    return D, vec, g


def test_geometry():
    assert geometry(False, 3, 3 * 3 * 64, (0, 3, 3, 64), [0, 576], False) == (4, True, 1)
    assert geometry(False, 3, 3 * 3 * 65, (0, 3, 3, 65), [0], False)[1] is False                  # odd post: 8-byte form
    assert geometry(False, 2, 600, (1, 3, 2, 64), [0], False)[1] is False                         # odd dst_off
    assert geometry(True, 16, 3 * 16 * 257, (1, 3, 16, 257), [3], False) == (16, True, 4)
    assert geometry(True, 16, 3 * 16 * 257, (1, 3, 16, 257), [3], True)[1] is False               # base off a 16-byte boundary
    assert geometry(False, 2, 300003, (0, 3, 1, 100001), [0], False)[2] == 512                    # capped: 300003 columns loop


def _rand(rng, n, cplx):
    v = rng.standard_normal(n)
    return v + 1j * rng.standard_normal(n) if cplx else v


def _flat(x):
    return np.ascontiguousarray(x).view(np.float64).reshape(-1)


class _Buf:
    """A payload of doubles between guards on the device, optionally 8 bytes off a 16-byte boundary."""

    def __init__(self, payload, off8=False):
        self.lead = GUARD + (1 if off8 else 0)
        self.host = np.concatenate([np.full(self.lead, SENTINEL), payload, np.full(GUARD, SENTINEL)])
        self.dev = dev.to_device(self.host)
        self.n = len(payload)

    @property
    def ptr(self):
        return self.dev.data_ptr() + 8 * self.lead

    def reset(self):
        self.dev.copy_(dev.to_device(self.host))

    def get(self):
        got = dev.to_host(self.dev)
        assert np.array_equal(kref.bits(got[:self.lead]), kref.bits(self.host[:self.lead])), "written in front of the payload"
        assert np.array_equal(kref.bits(got[self.lead + self.n:]), kref.bits(self.host[self.lead + self.n:])), "written behind the payload"
        return got[self.lead:self.lead + self.n].copy()


def build(cplx, specs, rng, gap):
    """Tables and data of one launch.  specs: [(pre, d_out, post, [d_in of every term])]; slabs of dst are ``gap`` elements apart,
    the slabs of src and the matrices lie back to back in the order of the terms."""
    jobs, terms, mats, xs = [], [], [], []
    dst_off = gap
    src_off = c_off = 0
    for pre, d_out, post, d_ins in specs:
        jobs.append([dst_off, pre, d_out, post, len(terms), len(d_ins), 0, 0])
        dst_off += pre * d_out * post + gap
        for d_in in d_ins:
            terms.append([src_off, d_in, c_off, 0])
            mats.append(_rand(rng, d_out * d_in, cplx).reshape(d_out, d_in))
            xs.append(_rand(rng, pre * d_in * post, cplx).reshape(pre, d_in, post))
            src_off += pre * d_in * post
            c_off += d_out * d_in
    jobs = np.array(jobs, dtype=np.int64).reshape(-1, 8)
    terms = np.array(terms, dtype=np.int64).reshape(-1, 4)
    return jobs, terms, mats, xs, dst_off, max(src_off, 1), max(c_off, 1)


def reference(jobs, mats, xs):
    """Per job: (re, im, magnitude sums of the two components, chain length sum_t d_in_t) in extended precision."""
    out = []
    for dst_off, pre, d_out, post, t0, nt, _, _ in jobs.tolist():
        shape = (pre, d_out, post)
        re, im, mr, mi = (np.zeros(shape, LD) for _ in range(4))
        chain = 0
        for t in range(t0, t0 + nt):
            ar, ai = kref.split(mats[t])
            xr, xi = kref.split(xs[t])
            chain += mats[t].shape[1]
            for c in range(mats[t].shape[1]):
                a_r, a_i = ar[None, :, c, None], ai[None, :, c, None]
                x_r, x_i = xr[:, None, c, :], xi[:, None, c, :]
                re += a_r * x_r - a_i * x_i
                im += a_r * x_i + a_i * x_r
                mr += np.abs(a_r * x_r) + np.abs(a_i * x_i)
                mi += np.abs(a_r * x_i) + np.abs(a_i * x_r)
        out.append((re, im, mr, mi, chain))
    return out


def run_and_check(cplx, specs, gap=3, mis=None, max_d=None, tag=''):
    """One launch (twice: bit-identical), everything the header promises checked; -> worst err / bound."""
    L = dev.lib()
    W = 2 if cplx else 1
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng([sum(map(ord, 'mpo_apply' + tag)), int(cplx), len(specs), gap] + [s[2] for s in specs])
    jobs, terms, mats, xs, n_dst, n_src, n_coeff = build(cplx, specs, rng, gap)
    src_host = np.full(n_src, np.nan, dtype=dt)
    for (off, _, _, _), x in zip(terms.tolist(), xs):
        src_host[off:off + x.size] = x.reshape(-1)
    coeff_host = np.zeros(n_coeff, dtype=dt)
    for (_, _, off, _), m in zip(terms.tolist(), mats):
        coeff_host[off:off + m.size] = m.reshape(-1)
    sb = _Buf(_flat(src_host), mis == 'src')
    cb = _Buf(_flat(coeff_host))
    db = _Buf(np.full(n_dst * W, SENTINEL), mis == 'dst')
    jd, td = dev.to_device(jobs), dev.to_device(terms if len(terms) else np.zeros((1, 4), np.int64))
    elems = jobs[:, 1] * jobs[:, 2] * jobs[:, 3]
    max_elems = int(elems.max())
    if max_d is None:
        max_d = int(max([1] + [s[1] for s in specs] + [d for s in specs for d in s[3]]))
    res = []
    for _ in range(2):
        db.reset()
        dev.check(L.tpa_mpo_apply_batch(int(cplx), jd.data_ptr(), len(jobs), td.data_ptr(), cb.ptr, max_d, max_elems, sb.ptr, db.ptr,
                                        dev.stream()), "mpo_apply")
        res.append(db.get())
        assert np.array_equal(kref.bits(sb.get()), kref.bits(_flat(src_host))), "src was written"
        assert np.array_equal(kref.bits(cb.get()), kref.bits(_flat(coeff_host))), "coeff was written"
    assert np.array_equal(kref.bits(res[0]), kref.bits(res[1])), "tpa_mpo_apply_batch is not deterministic"
    got = res[0].view(dt) if cplx else res[0]
    written = np.zeros(n_dst, dtype=bool)
    R = 2 if cplx else 1
    worst = 0.
    for (dst_off, pre, d_out, post, _, _, _, _), (re, im, mr, mi, chain) in zip(jobs.tolist(), reference(jobs, mats, xs)):
        n = pre * d_out * post
        assert not written[dst_off:dst_off + n].any()
        written[dst_off:dst_off + n] = True
        gr, gi = kref.split(got[dst_off:dst_off + n].reshape(re.shape))
        lim_r, lim_i = R * (chain + 1) * EPS * mr, R * (chain + 1) * EPS * mi
        err_r, err_i = np.abs(gr - re), np.abs(gi - im)
        ratio = float(max(np.max(err_r / np.maximum(lim_r, LD(1e-300)), initial=0.), np.max(err_i / np.maximum(lim_i, LD(1e-300)), initial=0.)))
        assert np.all(err_r <= lim_r) and np.all(err_i <= lim_i), "job at %d: worst err / bound = %.3g" % (dst_off, ratio)
        worst = max(worst, ratio)
    untouched = np.repeat(~written, W)
    assert np.array_equal(kref.bits(res[0][untouched]), kref.bits(np.full(int(untouched.sum()), SENTINEL))), "a gap between the slabs was written"
    print("CONFORMANCE tpa_mpo_apply_batch(%s) %s jobs=%d max_d=%d max_elems=%d gap=%d%s max_err_over_bound=%.4f"
          % (tag, 'complex' if cplx else 'real', len(jobs), max_d, max_elems, gap, ' mis=' + mis if mis else '', worst))
    return worst


DS = [(1, 1), (2, 2), (1, 2), (3, 1), (4, 4), (16, 16), (16, 3)]


@pytest.mark.parametrize("d", DS, ids=lambda d: "%dx%d" % d)
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_shapes(bbackend, cplx, d):
    """Every (d_out, d_in) at every post and pre, one job per launch at offset ``gap``: even gap and even post -> the 16-byte form of
    real data, odd gap or odd post -> its 8-byte form; two terms per job."""
    d_out, d_in = d
    for post in (1, 63, 64, 65, 257):
        for pre in (1, 3):
            run_and_check(cplx, [(pre, d_out, post, [d_in, d_in])], gap=2 + (pre == 3 and post == 64), tag='shape')


@pytest.mark.parametrize("mis", ['src', 'dst'])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_misaligned_base(bbackend, cplx, mis):
    """A base 8 bytes off a 16-byte boundary (an odd offset into a real arena; for complex data the 8-byte form of the whole launch),
    with an odd and an even post."""
    for post in (65, 64):
        run_and_check(cplx, [(3, 3, post, [2, 3])], gap=2, mis=mis, tag='mis')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_term_counts(bbackend, cplx):
    """term_count = 0 (zeros), 1, 2 and 7 in one launch, different d_in inside one job."""
    run_and_check(cplx, [(3, 3, 65, []), (3, 3, 65, [2]), (1, 2, 64, [1, 4]), (3, 3, 66, [1, 2, 3, 4, 1, 2, 3])], gap=2, tag='terms')
    run_and_check(cplx, [(2, 4, 10, [])], gap=1, max_d=4, tag='terms0')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_mixed_jobs(bbackend, cplx):
    """Jobs of very different size under one grid (sized by the largest), zero-extent jobs among them, even and odd offsets (real
    data: both forms in one launch)."""
    specs = [(1, 1, 1, [1]), (3, 2, 256, [2, 1]), (0, 2, 5, [2]), (1, 4, 5000, [4, 2, 1]), (2, 0, 5, [3]), (2, 16, 700, [16, 3]),
             (2, 2, 0, [2]), (5, 3, 7, [3, 3]), (4, 2, 64, [2])]
    run_and_check(cplx, specs, gap=2, tag='mixed')
    run_and_check(cplx, specs, gap=5, tag='mixed')


@pytest.mark.parametrize("post", [100001, 100002])
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_job_beyond_the_grid(bbackend, cplx, post):
    """One job with more columns than the 512 * 256 threads of the capped grid: the grid-stride loop wraps (real data: in the 8-byte
    form with 3 * 100001 columns, in the 16-byte form with 3 * 50001)."""
    assert 3 * (post // 2) > CAP
    run_and_check(cplx, [(3, 1, post, [2])], gap=2, tag='big')


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_arguments(bbackend, cplx):
    """max_d = 0 and 17 and n_jobs = 65536: TPA_E_BADARG; n_jobs = 0: 0; nothing is written in any of them."""
    L = dev.lib()
    W = 2 if cplx else 1
    rng = np.random.default_rng(5)
    jobs, terms, mats, xs, n_dst, n_src, n_coeff = build(cplx, [(3, 2, 64, [2])], rng, 2)
    sb, cb = _Buf(_flat(xs[0])), _Buf(_flat(mats[0]))
    db = _Buf(np.full(n_dst * W, SENTINEL))
    jd, td = dev.to_device(jobs), dev.to_device(terms)
    args = lambda n_jobs, max_d: (int(cplx), jd.data_ptr(), n_jobs, td.data_ptr(), cb.ptr, max_d, 3 * 2 * 64, sb.ptr, db.ptr, dev.stream())
    assert L.tpa_mpo_apply_batch(*args(1, 0)) == _lib.E_BADARG
    assert L.tpa_mpo_apply_batch(*args(1, _lib.MPO_APPLY_MAXD + 1)) == _lib.E_BADARG
    assert L.tpa_mpo_apply_batch(*args(65536, 2)) == _lib.E_BADARG
    assert L.tpa_mpo_apply_batch(*args(0, 2)) == 0
    assert L.tpa_mpo_apply_batch(*args(-1, 2)) == 0
    assert L.tpa_mpo_apply_batch(2, *args(1, 2)[1:]) == _lib.E_BADARG          # dtype
    assert np.array_equal(kref.bits(db.get()), kref.bits(np.full(n_dst * W, SENTINEL)))
    assert L.tpa_mpo_apply_batch(*args(1, 2)) == 0                             # (the same arguments do run)
    assert not np.array_equal(kref.bits(db.get()), kref.bits(np.full(n_dst * W, SENTINEL)))


def test_symbol_is_exported():
    assert 'tpa_mpo_apply_batch' in _lib.exported_symbols()
    assert _lib.MPO_APPLY_MAXD == 16
