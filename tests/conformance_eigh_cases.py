"""Cases, extended-precision reference and checkers of the conformance tests of the Hermitian eigensolver kernels
(tests/test_conformance_eigh.py; the defects of tests/test_conformance_mutations.py run against the same checkers): ``tpa_eigh_batch`` on
every route and ``tpa_eigh_from_svd``.

Everything here is written from the K7 section of ``include/tenpy_amd.h``; nothing knows about Jacobi rounds, workgroups or the numpy
emulation.  Arithmetic of the checkers is ``np.longdouble`` / ``np.clongdouble``.  A case is built once per process and never changed:
the tests of both backends and the mutation tests share it together with its cached reference."""
import copy
import ctypes

import numpy as np

from kernel_reference import bits
from tenpy_amd.linalg import _device as dev

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -53

# ---- the bounds: c * f * EPS * sqrt(n) [* |A|_F], f = 4 for complex data.  c = 8 * (largest ratio LAPACK reaches on the committed
#      cases), rounded up to a power of two; the measured ratios stand in the docstring of tests/test_conformance_eigh.py --------------
C_W = 16             # |w_i - lambda_i|                     <= c f EPS sqrt(n) |A|_F
C_RESIDUAL = 16      # per vector |A v_i - w_i v_i|_2       <= c f EPS sqrt(n) |A|_F
C_ORTH = 64          # largest column norm of V^H V - I     <= c f EPS sqrt(n)
C_ERR = 2            # tpa_eigh_from_svd: |err - err(long double)| <= c f EPS sqrt(n) S_1
REF_OFFDIAG = 2.0 ** -60       # the long double reference: final off-diagonal norm of V^H A V <= this * |A|_F
COS_MIN = 0.05                 # tpa_eigh_from_svd: |Re u_i^H v_i| of every vector with S_i > 0 (the sign decision is well conditioned)


def _f(cplx):
    return 4.0 if cplx else 1.0


def _ld(x):
    return np.asarray(x).astype(CLD if np.iscomplexobj(x) else LD)


def _colnorm(x):
    return np.sqrt(np.sum(np.abs(x) ** 2, axis=0))


def _fro(x):
    return np.sqrt(np.sum(np.abs(_ld(x)) ** 2))


# ---- reference and measures --------------------------------------------------------------------------------------------------

def lower_hermitian(a):
    """The Hermitian matrix an UPLO = 'L' solver sees: the strict lower triangle, its mirror image, the real part of the diagonal."""
    low = np.tril(a, -1)
    h = low + low.conj().T
    d = np.arange(a.shape[0])
    h[d, d] = np.diagonal(a).real
    return h


def _jacobi_ld(T, thr):
    """Cyclic two-sided Jacobi on the Hermitian long double matrix T (in place) until no |T_ij| > thr -> number of sweeps."""
    n = T.shape[0]
    cplx = np.iscomplexobj(T)
    for sweep in range(40):
        up = np.abs(np.triu(T, 1))
        todo = np.argwhere(up > thr)
        if len(todo) == 0:
            return sweep
        for p, q in todo:
            c = T[p, q]
            ac = np.abs(c)
            if not ac > thr:            # (an earlier rotation of this sweep took it away)
                continue
            tau = (T[q, q].real - T[p, p].real) / (2 * ac)
            t = (LD(1) if tau >= 0 else LD(-1)) / (np.abs(tau) + np.sqrt(1 + tau * tau))
            cs = 1 / np.sqrt(1 + t * t)
            sn = t * cs
            ph = np.conj(c) / ac if cplx else (LD(1) if c >= 0 else LD(-1))          # e^{-i phi} of T_pq = |c| e^{i phi}
            # G = [[cs, sn], [-sn e^{-i phi}, cs e^{-i phi}]] on (p, q):  T <- G^H T G
            cp, cq = T[:, p].copy(), T[:, q].copy()
            T[:, p], T[:, q] = cs * cp - sn * ph * cq, sn * cp + cs * ph * cq
            rp, rq = T[p, :].copy(), T[q, :].copy()
            T[p, :], T[q, :] = cs * rp - sn * np.conj(ph) * rq, sn * rp + cs * np.conj(ph) * rq
            T[p, q] = T[q, p] = 0
    raise AssertionError("the long double Jacobi reference did not converge")


def eigenvalues_ld(h):
    """Eigenvalues of the Hermitian double matrix h in long double, ascending -> (lambda, final off-diagonal norm / |h|_F).
    LAPACK's vectors, two Newton-Schulz steps in long double (orthonormal to long double level), T = V^H h V in long double, cyclic
    Jacobi on T until no |T_ij| > 2^-64 |h|_F / n.  The kernel under test takes no part."""
    n = h.shape[0]
    H = _ld(h)
    fro = _fro(h)
    if fro == 0:
        return np.zeros(n, LD), LD(0)
    _, v = np.linalg.eigh(h / float(fro))           # (scaled: LAPACK is only the starting guess)
    V = _ld(v)
    eye = np.eye(n, dtype=LD)
    for _ in range(2):
        V = V @ (1.5 * eye - 0.5 * (V.conj().T @ V))
    T = V.conj().T @ (H / fro) @ V
    T = (T + T.conj().T) / 2
    _jacobi_ld(T, LD(2.0) ** -64 / n)
    off = T - np.diag(np.diagonal(T))
    return np.sort(np.diagonal(T).real) * fro, np.sqrt(np.sum(np.abs(off) ** 2))


def eig_residual(h, w, v):
    """Per vector |h v_i - w_i v_i|_2 in long double."""
    V = _ld(v)
    return _colnorm(_ld(h) @ V - V * np.asarray(w).astype(LD)[None, :])


def orthogonality(v):
    """The largest column 2-norm of V^H V - I."""
    V = _ld(v)
    return np.max(_colnorm(V.conj().T @ V - np.eye(V.shape[1], dtype=LD)))


# ---- data ----------------------------------------------------------------------------------------------------------------------

# (in the order in which they take their blocks: the most demanding first, each on the largest block that is free and on which it acts)
KINDS_REAL = ('gaussian', 'upper_large', 'diagonal', 'upper_nan', 'clusters', 'graded_rank_deficient', 'pm_pairs', 'psd_flat',
              'scaled_up', 'scaled_down', 'zero', 'multiple_of_identity')
KINDS_COMPLEX = KINDS_REAL[:8] + ('diag_imag',) + KINDS_REAL[8:]
MIN_N = {'gaussian': 1, 'upper_large': 2, 'diagonal': 3, 'upper_nan': 2, 'clusters': 6, 'graded_rank_deficient': 8, 'pm_pairs': 4,
         'psd_flat': 3, 'diag_imag': 2, 'scaled_up': 2, 'scaled_down': 2, 'zero': 1, 'multiple_of_identity': 1}
SAME_AS_CLEAN = ('upper_nan', 'upper_large', 'diag_imag')        # stored data that is not Hermitian: only the lower triangle counts


def acts(kind, n):
    return n >= MIN_N[kind]


def _gauss(rng, m, n, cplx):
    g = rng.standard_normal((m, n))
    return g + 1j * rng.standard_normal((m, n)) if cplx else g


def _with_spectrum(rng, lam, cplx):
    q, _ = np.linalg.qr(_gauss(rng, len(lam), len(lam), cplx))
    h = (q * lam) @ q.conj().T
    return 0.5 * (h + h.conj().T)


def _exact_diagonal(rng, n):
    """Integers of both signs, unsorted, whose squares sum to a perfect square: |A|_F, the shift 2 |A|_F and every d_i + shift are then
    exactly representable, so a solver that leaves a diagonal matrix alone returns it exactly."""
    for _ in range(100000):
        d = rng.integers(1, 10, n) * rng.choice([-1, 1], n)
        s = int(np.sum(d * d))
        r = int(round(np.sqrt(s)))
        if r * r == s and d.min() < 0 < d.max() and np.any(np.diff(d) < 0) and np.any(np.diff(d) > 0):
            return d.astype(float)
    raise AssertionError("no exact diagonal of %d entries found" % n)


def make_block(rng, n, cplx, kind):
    """-> the n x n array that is uploaded.  Its lower triangle (with the real part of the diagonal) defines the matrix."""
    x = _gauss(rng, n, n, cplx)
    a = x + x.conj().T                                                   # indefinite, exactly Hermitian
    if kind == 'psd_flat':
        a = x.conj().T @ x / n
    elif kind == 'graded_rank_deficient':
        y = x[:, :n // 2] * np.logspace(0, -8, n // 2)
        a = y @ y.conj().T
    elif kind == 'pm_pairs':
        lam = np.linspace(1, 2, n // 2)
        a = _with_spectrum(rng, np.concatenate([lam, -lam, np.zeros(n % 2)]), cplx)
    elif kind == 'clusters':                                             # multiplicity 3, both signs
        vals = np.array([(-1) ** k * (1 + k / 4) for k in range((n + 2) // 3)])
        a = _with_spectrum(rng, np.repeat(vals, 3)[:n], cplx)
    elif kind == 'diagonal':
        a = np.diag(_exact_diagonal(rng, n)).astype(a.dtype)
    elif kind == 'zero':
        a = np.zeros_like(a)
    elif kind == 'multiple_of_identity':
        a = (0.75 * np.eye(n)).astype(a.dtype)
    elif kind == 'scaled_up':
        a = a * 1e+100
    elif kind == 'scaled_down':
        a = a * 1e-100
    elif kind == 'upper_nan':
        a[np.triu_indices(n, 1)] = complex(np.nan, np.nan) if cplx else np.nan
    elif kind == 'upper_large':
        g = _gauss(rng, n, n, cplx)[np.triu_indices(n, 1)]
        a[np.triu_indices(n, 1)] = 1e8 * float(_fro(lower_hermitian(a))) * (g + np.sign(g.real) + (1j * np.sign(g.imag) if cplx else 0))
    elif kind == 'diag_imag':
        d = np.arange(n)
        a[d, d] = a[d, d].real + 1j * (1 + np.abs(rng.standard_normal(n))) * rng.choice([-1, 1], n)
    else:
        assert kind == 'gaussian', kind
    return np.ascontiguousarray(a)


def assign_kinds(sizes, cplx):
    """Kinds in the order of KINDS_*: each goes to the largest block that is still free and on which it acts; blocks that are left
    over (more blocks than kinds, or too small for what is left) are Gaussian."""
    out = [None] * len(sizes)
    by_size = sorted(range(len(sizes)), key=lambda i: (-sizes[i], i))
    for q in (KINDS_COMPLEX if cplx else KINDS_REAL):
        i = next((i for i in by_size if out[i] is None and acts(q, sizes[i])), None)
        if i is not None:
            out[i] = q
    return [q or 'gaussian' for q in out]


class Block:
    pass


class EighCase:
    """Blocks of one call laid into three unrelated arenas.  ``A``: the input arena (canaries in the gaps); ``W0`` / ``V0``: NaN where
    a block goes, distinct finite canaries everywhere else; ``jobs``: the job table; ``direct`` / ``svd_algorithm``: the values of the
    test hooks tpa_eigh_set_direct / tpa_svd_set_algorithm during the call; ``route``: what tpa_eigh_last_direct has to say."""


def _lay(rng, sizes, order=None):
    """Offsets of blocks of the given sizes in one arena with a gap of 1 .. 6 elements before every block and behind the last."""
    order = range(len(sizes)) if order is None else order
    offs, pos = [0] * len(sizes), 0
    for b in order:
        pos += int(rng.integers(1, 7))
        offs[b] = pos
        pos += sizes[b]
    return offs, pos + int(rng.integers(1, 7))


def _nan(dtype):
    return complex(np.nan, np.nan) if np.dtype(dtype).kind == 'c' else np.nan


def _canaries(total, cplx, seed):
    c = 1000.0 + seed + np.arange(total) / 8.0            # distinct, finite, exactly representable
    return c - 1j * (c + 0.5) if cplx else c


FILLER = [12, 10, 7]           # so that every kind finds a block on which it acts (complex data has one kind more: one filler more)
FILLER_C = [12, 10, 8, 7]
SMALL = [94, 64, 33, 32, 31, 9, 3, 2, 1]
BOUNDARY = [95, 40, 1]
LARGE = [161, 130, 128, 97, 96, 64, 33, 2, 1]
DECLINED = [130, 96, 33]
DYN_OFF = 1 << 24              # tpa_svd_set_algorithm: no activity-driven rounds -> the direct request of a real call is declined

# name -> (complex, data set, block sizes, tpa_eigh_set_direct, tpa_svd_set_algorithm, route = tpa_eigh_last_direct after the call)
EIGH_CASES = {
    'small_b32': (False, 'small', SMALL, 1, 0, 0),
    'small_c': (True, 'small', SMALL, 1, 0, 0),
    'two_sided_boundary_real': (False, 'boundary', BOUNDARY, 1, 0, 1),
    'two_sided_boundary_complex': (True, 'boundary', BOUNDARY, 1, 0, 1),
    'two_sided_real': (False, 'large', LARGE, 1, 0, 1),
    'two_sided_complex': (True, 'large', LARGE, 1, 0, 1),
    'one_sided_gram_real': (False, 'large', LARGE, 0, 0, 0),
    'one_sided_gram_complex': (True, 'large', LARGE, 0, 0, 0),
    'two_sided_declined_real': (False, 'declined', DECLINED, 1, DYN_OFF, 0),
}
EVERY_KIND = ('small', 'large')          # data sets with enough blocks for every kind

_cases, _data = {}, {}


def _make_data(key, cplx, sizes):
    rng = np.random.default_rng([1707, sorted(['small', 'boundary', 'large', 'declined']).index(key), int(cplx)])
    dt = np.complex128 if cplx else np.float64
    sizes = list(sizes) + (FILLER_C if cplx else FILLER)
    c = EighCase()
    c.cplx, c.dtype, c.blocks = cplx, dt, []
    for n, kind in zip(sizes, assign_kinds(sizes, cplx)):
        b = Block()
        b.n, b.kind = n, kind
        b.a = make_block(rng, n, cplx, kind)
        b.h = lower_hermitian(b.a)
        b.fro = _fro(b.h)
        b.lam = b.offdiag = None
        c.blocks.append(b)
    nb = len(c.blocks)
    a_offs, a_total = _lay(rng, [b.n * b.n for b in c.blocks], order=rng.permutation(nb))
    w_offs, w_total = _lay(rng, [b.n for b in c.blocks], order=rng.permutation(nb))
    v_offs, v_total = _lay(rng, [b.n * b.n for b in c.blocks])
    c.A = np.array(_canaries(a_total, cplx, 0), dtype=dt)
    c.W0, c.V0 = np.array(_canaries(w_total, False, 1), dtype=np.float64), np.array(_canaries(v_total, cplx, 2), dtype=dt)
    c.w_mask, c.v_mask = np.zeros(w_total, bool), np.zeros(v_total, bool)
    for b, ao, wo, vo in zip(c.blocks, a_offs, w_offs, v_offs):
        b.a_off, b.w_off, b.v_off = ao, wo, vo
        c.A[ao:ao + b.n * b.n] = b.a.reshape(-1)
        c.w_mask[wo:wo + b.n] = True
        c.v_mask[vo:vo + b.n * b.n] = True
    c.W0[c.w_mask], c.V0[c.v_mask] = np.nan, _nan(dt)
    c.jobs = np.array([[b.a_off, b.n, b.w_off, b.v_off, 0, 0, 0, 0] for b in c.blocks], np.int64)
    return c


def eigh_case(name):
    if name not in _cases:
        cplx, key, sizes, direct, alg, route = EIGH_CASES[name]
        if (key, cplx) not in _data:
            _data[key, cplx] = _make_data(key, cplx, sizes)
        c = copy.copy(_data[key, cplx])          # (the blocks, with their cached references, are shared between the routes)
        c.name, c.direct, c.svd_algorithm, c.route = name, direct, alg, route
        _cases[name] = c
    return _cases[name]


def reference(b):
    if b.lam is None:
        b.lam, b.offdiag = eigenvalues_ld(b.h)
    return b.lam


# ---- running -------------------------------------------------------------------------------------------------------------------

class eigh_hooks:
    """``with eigh_hooks(L, direct, algorithm):`` -- the process-global test hooks, back to their defaults (1, 0) afterwards."""

    def __init__(self, L, direct=1, algorithm=0):
        self.L, self.direct, self.algorithm = L, direct, algorithm

    def __enter__(self):
        dev.check(self.L.tpa_eigh_set_direct(self.direct), "eigh_set_direct")
        dev.check(self.L.tpa_svd_set_algorithm(self.algorithm), "svd_set_algorithm")

    def __exit__(self, *exc):
        self.L.tpa_eigh_set_direct(1)
        self.L.tpa_svd_set_algorithm(0)


def call_eigh(L, cplx, jobs, A, W0, V0, max_sweeps=60, work_bytes=None, dtype_code=None):
    """Upload, call, download -> dict(rc, A, W, V (the arenas after the call), direct (tpa_eigh_last_direct), sweeps)."""
    jobs = np.ascontiguousarray(np.array(jobs, np.int64).reshape(-1, 8))
    code = int(cplx) if dtype_code is None else dtype_code
    Ad, Wd, Vd = dev.to_device(A), dev.to_device(W0), dev.to_device(V0)
    wb = int(L.tpa_eigh_worksize(int(cplx), jobs.ctypes.data, len(jobs)))
    work = dev.empty((wb + 7) // 8, np.float64)
    sweeps = ctypes.c_int(-1)
    rc = L.tpa_eigh_batch(code, jobs.ctypes.data, len(jobs), Ad.data_ptr(), Wd.data_ptr(), Vd.data_ptr(), work.data_ptr(),
                          wb if work_bytes is None else work_bytes, max_sweeps, 0.0, ctypes.byref(sweeps), dev.stream())
    return dict(rc=rc, A=dev.to_host(Ad), W=dev.to_host(Wd), V=dev.to_host(Vd), direct=int(L.tpa_eigh_last_direct()),
                sweeps=sweeps.value, worksize=wb)


def run_eigh(c, L=None, max_sweeps=60):
    L = L if L is not None else dev.lib()
    with eigh_hooks(L, c.direct, c.svd_algorithm):
        return call_eigh(L, c.cplx, c.jobs, c.A, c.W0, c.V0, max_sweeps)


def untouched(c, out):
    """The input arena and everything the call may not write (the whole of W and V for a call that fails) are bit-identical."""
    return (np.array_equal(bits(c.A), bits(out['A'])) and np.array_equal(bits(c.W0), bits(out['W']))
            and np.array_equal(bits(c.V0), bits(out['V'])))


def bound_factors(n, cplx, shifted):
    """(eigenvalues, residual, orthogonality) bounds in units of eps sqrt(n) [|A|_F].  ``shifted`` = False: LAPACK's class,
    c f.  ``shifted`` = True: the routes of the device, which all iterate on A' = A + mu with mu = 2 |A|_F (derivation in the docstring of
    tests/test_conformance_eigh.py): the remainder the stopping rule leaves, 6 n (eigenvalues) / 6 sqrt(n) (one column: residual), plus
    the rounding of LAPACK's class on A', |A'|_F <= (1 + 2 sqrt(n)) |A|_F.  Orthogonality does not see the shift."""
    f = _f(cplx)
    if not shifted:
        return C_W * f, C_RESIDUAL * f, C_ORTH * f
    grow = 1 + 2 * np.sqrt(n)
    return 6 * n + C_W * f * grow, 6 * np.sqrt(n) + C_RESIDUAL * f * grow, C_ORTH * f


def check_eigh(c, out, shifted=False):
    """The assertions of the conformance tests on one call -> the largest error / bound per measure.  Every block's figures are
    printed (MEASURED lines, in units of eps sqrt(n) |A|_F) before anything is asserted on them."""
    assert out['rc'] == 0, "%s: return code %d" % (c.name, out['rc'])
    assert np.array_equal(bits(c.A), bits(out['A'])), "%s: the A arena changed" % c.name
    W, V = out['W'], out['V']
    assert np.array_equal(bits(W[~c.w_mask]), bits(c.W0[~c.w_mask])), "%s: an element outside of every W_b changed" % c.name
    assert np.array_equal(bits(V[~c.v_mask]), bits(c.V0[~c.v_mask])), "%s: an element outside of every V_b changed" % c.name
    worst = dict(eigenvalues=0.0, residual=0.0, orthogonality=0.0)
    failures = []
    for i, b in enumerate(c.blocks):
        n = b.n
        tag = "%s: block %d (n = %d, %s)" % (c.name, i, n, b.kind)
        w = W[b.w_off:b.w_off + n]
        v = V[b.v_off:b.v_off + n * n].reshape(n, n)
        assert not np.isnan(w).any(), tag + ": W_b is not written completely"
        assert not np.isnan(v.view(np.float64)).any(), tag + ": V_b is not written completely"
        assert np.isfinite(w).all() and np.isfinite(v.view(np.float64)).all(), tag + ": Inf in the output"
        assert np.all(w[1:] >= w[:-1]), tag + ": the eigenvalues do not ascend"
        lam = reference(b)
        unit = EPS * np.sqrt(LD(n))
        bw, br, bo = bound_factors(n, c.cplx, shifted)
        err_w = np.max(np.abs(w.astype(LD) - lam))
        res = np.max(eig_residual(b.h, w, v))
        orth = orthogonality(v)
        if b.fro == 0:          # the zero matrix: nothing to scale with -- eigenvalues and residuals are exactly zero
            assert err_w == 0 and res == 0, tag + ": a non-zero eigenvalue of the zero matrix"
            uw = ur = 0.0
        else:
            uw, ur = float(err_w / (unit * b.fro)), float(res / (unit * b.fro))
        uo = float(orth / unit)
        print("MEASURED %s: eigenvalues %.3g (bound %.4g) residual %.3g (bound %.4g) orthogonality %.3g (bound %.4g)"
              % (tag, uw, bw, ur, br, uo, bo))
        for key, u, bnd in (('eigenvalues', uw, bw), ('residual', ur, br), ('orthogonality', uo, bo)):
            worst[key] = max(worst[key], u / bnd)
            if u > bnd:
                failures.append("%s: %s / bound = %.3g" % (tag, key, u / bnd))
        if b.kind == 'diagonal':
            assert np.array_equal(w, np.sort(np.diagonal(b.a).real)), tag + ": w is not exactly the sorted diagonal"
            av = np.abs(v)
            assert np.all((av == 0) | (av == 1)) and np.all(av.sum(0) == 1) and np.all(av.sum(1) == 1) and not np.any(v.imag), \
                tag + ": V is not a signed permutation of exact 0 / +-1"
    assert not failures, "\n".join(failures)
    return worst


def check_repeatable(c, out, again):
    assert np.array_equal(bits(out['W']), bits(again['W'])), "%s: a second identical call gives another W" % c.name
    assert np.array_equal(bits(out['V']), bits(again['V'])), "%s: a second identical call gives another V" % c.name


# ---- tpa_eigh_from_svd -----------------------------------------------------------------------------------------------------------

FROM_SVD_N = [1, 2, 63, 64, 65, 129, 130]          # one call: the grid is sized by the largest job
FROM_SVD_KINDS_REAL = ('aligned', 'rotated_pairs', 'rank_deficient', 'nan_vector')
FROM_SVD_KINDS_COMPLEX = FROM_SVD_KINDS_REAL + ('phase',)
NAN_JOB, NAN_AT = 4, (3, 64)          # nan_vector: U[3, 64] of the n = 65 job (a vector of the second workgroup along the vectors)
STALE_ERR = (np.inf, np.nan, 1e308)   # what err_dev holds before the call: bit patterns a missing clear would let through


class FromSvdCase:
    pass


def from_svd_case(kind, cplx):
    key = ('from_svd', kind, cplx)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng([1708, FROM_SVD_KINDS_COMPLEX.index(kind), int(cplx)])
    dt = np.complex128 if cplx else np.float64
    c = FromSvdCase()
    c.name, c.kind, c.cplx, c.dtype, c.blocks = "from_svd_%s_%s" % (kind, 'complex' if cplx else 'real'), kind, cplx, dt, []
    for j, n in enumerate(FROM_SVD_N):
        b = Block()
        b.n = n
        u, _ = np.linalg.qr(_gauss(rng, n, n, cplx))
        b.s = np.sort(rng.uniform(0.5, 2.0, n))[::-1].copy()
        d = rng.choice([-1., 1.], n)
        v = u * d                                        # v_i = d_i u_i bit for bit
        if kind == 'rotated_pairs':                      # pairs (2k, 2k + 1) mixed by known angles: Re u_i^H v_i = d_i cos(theta_k)
            theta = np.where(rng.random(n // 2) < 0.3, 1e-8, 1.0) * rng.uniform(0.1, 1.2, n // 2)
            if j % 2:                                    # ... every other job: the large angles (and the maximum) among the last vectors
                theta[:n // 4] *= 1e-8
            for k, th in enumerate(theta):
                i, l = 2 * k, 2 * k + 1
                v[:, i] = d[i] * (np.cos(th) * u[:, i] + np.sin(th) * u[:, l])
                v[:, l] = d[l] * (-np.sin(th) * u[:, i] + np.cos(th) * u[:, l])
        elif kind == 'rank_deficient' and n >= 3:        # trailing S = 0 with zero vectors
            r = n - n // 3
            b.s[r:], u[:, r:], v[:, r:] = 0, 0, 0
        elif kind == 'phase':                            # v_i = e^{i phi_i} u_i, cos(phi_i) of both signs and away from zero
            phi = rng.uniform(0.0, 1.4, n) + np.pi * rng.integers(0, 2, n)
            v = u * np.exp(1j * phi)
        elif kind == 'nan_vector' and j == NAN_JOB:
            u[NAN_AT] = np.nan
        b.u, b.vh = np.ascontiguousarray(u), np.ascontiguousarray(v.conj().T)
        # the long double reference of the definition: d_i = sign(Re u_i^H v_i), err = max_i S_i |v_i - d_i u_i|
        U, V = _ld(b.u), _ld(b.vh).conj().T
        b.cos = np.real(np.sum(U.conj() * V, axis=0))
        b.d = np.where(b.cos < 0, -1., 1.)
        b.err_i = b.s.astype(LD) * _colnorm(V - U * b.d.astype(LD)[None, :])
        c.blocks.append(b)
    nb = len(c.blocks)
    sq, ln = [b.n * b.n for b in c.blocks], [b.n for b in c.blocks]
    c.arena0, c.off = {}, {}
    for i, (name, sizes, cx) in enumerate((('U', sq, cplx), ('VH', sq, cplx), ('S', ln, False), ('lam', ln, False))):
        offs, total = _lay(rng, sizes, order=rng.permutation(nb))
        c.arena0[name] = np.array(_canaries(total, cx, 3 * i), dtype=dt if cx else np.float64)
        c.off[name] = offs
    c.lam_mask = np.zeros(len(c.arena0['lam']), bool)
    for j, b in enumerate(c.blocks):
        c.arena0['U'][c.off['U'][j]:c.off['U'][j] + b.n * b.n] = b.u.reshape(-1)
        c.arena0['VH'][c.off['VH'][j]:c.off['VH'][j] + b.n * b.n] = b.vh.reshape(-1)
        c.arena0['S'][c.off['S'][j]:c.off['S'][j] + b.n] = b.s
        c.lam_mask[c.off['lam'][j]:c.off['lam'][j] + b.n] = True
    c.arena0['lam'][c.lam_mask] = np.nan
    c.arena0['err'] = np.array([STALE_ERR[j % 3] for j in range(nb)] + [77.0, 78.0])       # two canaries behind the jobs' words
    assert c.off['U'] != c.off['VH'] and c.off['S'] != c.off['lam']
    c.jobs = np.array([[c.off['U'][j], b.n, c.off['S'][j], c.off['VH'][j], c.off['lam'][j], 0, 0, 0]
                       for j, b in enumerate(c.blocks)], np.int64)
    _cases[key] = c
    return c


def call_from_svd(L, cplx, jobs, arena0, dtype_code=None):
    jobs = np.ascontiguousarray(np.array(jobs, np.int64).reshape(-1, 8))
    d = {k: dev.to_device(a) for k, a in arena0.items()}
    rc = L.tpa_eigh_from_svd(int(cplx) if dtype_code is None else dtype_code, jobs.ctypes.data, len(jobs), d['U'].data_ptr(),
                             d['S'].data_ptr(), d['VH'].data_ptr(), d['lam'].data_ptr(), d['err'].data_ptr(), dev.stream())
    out = {k: dev.to_host(t) for k, t in d.items()}       # (to_host synchronises: the entry point is asynchronous)
    out['rc'] = rc
    return out


def run_from_svd(c, L=None):
    return call_from_svd(L if L is not None else dev.lib(), c.cplx, c.jobs, c.arena0)


def check_from_svd(c, out):
    """-> the largest |err - err(long double)| / bound."""
    assert out['rc'] == 0, "%s: return code %d" % (c.name, out['rc'])
    for k in ('U', 'S', 'VH'):
        assert np.array_equal(bits(out[k]), bits(c.arena0[k])), "%s: the %s arena changed" % (c.name, k)
    lam, err = out['lam'], out['err']
    assert np.array_equal(bits(lam[~c.lam_mask]), bits(c.arena0['lam'][~c.lam_mask])), c.name + ": an element outside of every lam_b changed"
    nb = len(c.blocks)
    assert np.array_equal(bits(err[nb:]), bits(c.arena0['err'][nb:])), c.name + ": an element behind err_dev[n_jobs) changed"
    worst = 0.0
    for j, b in enumerate(c.blocks):
        tag = "%s: job %d (n = %d)" % (c.name, j, b.n)
        got = lam[c.off['lam'][j]:c.off['lam'][j] + b.n]
        poisoned = c.kind == 'nan_vector' and j == NAN_JOB
        live = b.s > 0
        if poisoned:
            live[NAN_AT[1]] = False
            assert abs(got[NAN_AT[1]]) == b.s[NAN_AT[1]], tag + ": lam of the NaN vector is not +-S_i"
            assert not (err[j] < 1e300), tag + ": err = %r of a job with a NaN vector passes a gate" % err[j]
        assert np.all(np.abs(b.cos[live]) >= COS_MIN), tag + ": the sign decision of the input is not well conditioned"
        assert np.array_equal(bits(got[live]), bits((b.d * b.s)[live])), tag + ": lam_i is not d_i S_i bit for bit"
        assert not np.any(got[~live & (b.s == 0)]), tag + ": lam_i != 0 where S_i == 0"
        if poisoned:
            continue
        assert np.isfinite(err[j]) and err[j] >= 0, tag + ": err = %r (stale contents of err_dev?)" % err[j]
        ref = np.max(b.err_i)
        if c.kind in ('aligned', 'rank_deficient', 'nan_vector'):
            assert ref == 0 and err[j] == 0.0 and not np.signbit(err[j]), tag + ": err = %r, v_i = d_i u_i bit for bit" % err[j]
        r = float(np.abs(LD(err[j]) - ref) / (C_ERR * _f(c.cplx) * EPS * np.sqrt(LD(b.n)) * b.s[0]))
        assert r <= 1, tag + ": |err - err(long double)| / bound = %.3g (err = %.17g, reference %.17g)" % (r, err[j], float(ref))
        worst = max(worst, r)
    return worst


def check_from_svd_repeatable(c, out, again):
    for k in ('lam', 'err'):
        assert np.array_equal(bits(out[k]), bits(again[k])), "%s: a second identical call gives another %s" % (c.name, k)
