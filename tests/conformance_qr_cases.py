"""Cases, extended-precision reference and checkers of the Householder / compact-WY conformance tests (tests/test_conformance_qr.py;
the defects of tests/test_conformance_mutations.py run against the same checkers): ``tpa_qr_batch`` on every dispatch path and the
pivoted panel variants of ``tpa_svd_batch``.

Everything here is written from the K5 / K6 sections of ``include/tenpy_amd.h``; nothing knows about panels, workgroups or the numpy
emulation.  Arithmetic of the checkers is ``np.longdouble`` / ``np.clongdouble``.  A case is built once per process and never
changed: the tests of both backends and the mutation tests share it together with its cached reference."""
import ctypes

import numpy as np

import svd_reference
from kernel_reference import bits
from tenpy_amd.linalg import _device as dev

LD, CLD = np.longdouble, np.clongdouble
EPS = 2.0 ** -53
ONEWG_LDS_BYTES = 150 * 1024          # the reflector of the one-workgroup kernel lives in LDS: m <= 19200 (f64) / 9600 (c128)

# ---- the bounds: c * f * EPS * sqrt(.), f = 4 for complex data.  c = 8 * (largest ratio LAPACK reaches on the committed cases),
#      rounded up to a power of two; the measured ratios stand in the docstring of tests/test_conformance_qr.py ----------------------
C_BACKWARD = 64        # per column  ||a_j - Q r_j|| / ||a_j||           <= c f EPS sqrt(k)
C_ORTH = 32            # largest column norm of Q^H Q - I                 <= c f EPS sqrt(m)
C_RFACTOR = 32         # per column  ||r_j - r_j(long double)|| / ||a_j|| <= c f EPS sqrt(k)   (well-conditioned blocks)
C_SVD_S = 2            # |S_i - sigma_i| / sigma_1                        <= c f EPS sqrt(max(m, n))
C_SVD_RESIDUAL = 16    # per column  ||a_j - (U S VH)_j|| / sigma_1       <= c f EPS sqrt(max(m, n))
C_SVD_ORTH = 32        # largest column norm of U^H U - I, VH VH^H - I    <= c f EPS sqrt(max(m, n))
WELL_CONDITIONED = 32.0          # Gaussian blocks whose leading k columns have a 2-norm condition number up to this
PINS_R = ('gaussian', 'negative_real_lead', 'imaginary_lead')      # (Gaussian up to the diagonal, for the two lead kinds)


def _f(cplx):
    return 4.0 if cplx else 1.0


def _ld(x):
    return np.asarray(x).astype(CLD if np.iscomplexobj(x) else LD)


def _colnorm(x):
    return np.sqrt(np.sum(np.abs(x) ** 2, axis=0))


# ---- reference and measures --------------------------------------------------------------------------------------------------

def qr_backward(A, Q, R):
    """Per column j: ||a_j - Q r_j||_2 / ||a_j||_2 (a zero column is scored against 1)."""
    A = _ld(A)
    res = _colnorm(A - _ld(Q) @ _ld(R))
    scale = _colnorm(A)
    return res / np.where(scale > 0, scale, LD(1))


def qr_orthogonality(Q):
    """The largest column 2-norm of Q^H Q - I."""
    Q = _ld(Q)
    return np.max(_colnorm(Q.conj().T @ Q - np.eye(Q.shape[1], dtype=LD)))


def qr_householder_ld(A):
    """R of an unblocked Householder QR in long double with LAPACK's convention (d/zlarfg): beta = -sign(Re x0) ||x|| (sign(0) = +),
    a real diagonal, and H = I where the column is already reduced (nothing below the diagonal, real diagonal entry)."""
    W = _ld(A).copy()
    m, n = W.shape
    k = min(m, n)
    for j in range(k):
        x = W[j:, j].copy()
        s2 = np.sum(np.abs(x[1:]) ** 2)
        if s2 == 0 and np.imag(x[0]) == 0:
            continue
        beta = np.sqrt(np.abs(x[0]) ** 2 + s2)
        if np.real(x[0]) >= 0:
            beta = -beta
        tau = (beta - x[0]) / beta
        v = x / (x[0] - beta)
        v[0] = 1
        W[j:, j + 1:] -= np.conj(tau) * np.outer(v, v.conj() @ W[j:, j + 1:])
        W[j, j], W[j + 1:, j] = beta, 0
    return np.triu(W[:k])


# ---- data ----------------------------------------------------------------------------------------------------------------------

KINDS_REAL = ('gaussian', 'graded', 'zero_column', 'equal_columns', 'triangular', 'scaled_up', 'scaled_down')
KINDS_COMPLEX = KINDS_REAL + ('negative_real_lead', 'imaginary_lead')


def _gauss(rng, m, n, cplx):
    g = rng.standard_normal((m, n))
    return g + 1j * rng.standard_normal((m, n)) if cplx else g


def make_block(rng, m, n, cplx, kind):
    a = _gauss(rng, m, n, cplx)
    d = np.arange(min(m, n))
    if kind == 'graded':
        a = a * np.logspace(0, -14, n)[None, :]
    elif kind == 'zero_column':
        a[:, n // 2] = 0
    elif kind == 'equal_columns':
        a[:, n - 1] = a[:, (n - 1) // 2]
    elif kind == 'triangular':           # already reduced, real diagonal of both signs: every reflector is H = I
        a = np.triu(a)
        a[d, d] = a[d, d].real
    elif kind == 'scaled_up':
        a = a * 1e+100
    elif kind == 'scaled_down':
        a = a * 1e-100
    elif kind == 'negative_real_lead':
        a[d, d] = -np.abs(a[d, d])
    elif kind == 'imaginary_lead':
        lead = np.zeros(len(d), complex)      # Re x0 = +0.0 exactly: LAPACK takes sign(0) = +, so beta = -|x|
        lead.imag = a[d, d].real
        a[d, d] = lead
    else:
        assert kind == 'gaussian', kind
    return np.ascontiguousarray(a)


def acts(kind, m, n):
    """Whether the kind does on an m x n block what it is there for: the special column is one that gets reduced (it is among the
    first min(m, n) and has rows below the diagonal), a triangular block has more than one column to leave alone, the two
    complex lead kinds sit on a tall block whose R is compared with the long double reference."""
    k = min(m, n)
    if kind == 'zero_column':
        return n >= 3 and m > n // 2 + 1
    if kind == 'equal_columns':
        return n >= 3 and m > (n - 1) // 2 + 1
    if kind == 'graded':
        return k >= 3
    if kind == 'triangular':
        return k >= 2
    if kind in ('negative_real_lead', 'imaginary_lead'):
        return n >= 3 and m >= 2 * n
    return m >= 2          # gaussian, scaled_up, scaled_down: a reflector with something below the diagonal


def assign_kinds(shapes, cplx):
    """Every kind at least once over the blocks of a batch, each on a block where it acts (``acts``).  The first (path-defining)
    block is Gaussian; the other kinds go, the most demanding first, to the largest block that is still free and on which they
    act; what is left over takes the kinds in turn where they act and is Gaussian otherwise."""
    kinds = [q for q in (KINDS_COMPLEX if cplx else KINDS_REAL) if q != 'gaussian']
    order = sorted(kinds, key=lambda q: (q not in ('negative_real_lead', 'imaginary_lead'), q != 'zero_column', q != 'equal_columns',
                                         q != 'graded', q != 'triangular'))
    out = ['gaussian'] + [None] * (len(shapes) - 1)
    by_size = sorted(range(1, len(shapes)), key=lambda i: (-shapes[i][0] * shapes[i][1], i))
    for rnd in range(2):
        for q in order:
            i = next((i for i in by_size if out[i] is None and acts(q, *shapes[i])), None)
            assert i is not None or rnd, "no block left on which '%s' acts" % q
            if i is not None:
                out[i] = q
    return [q or 'gaussian' for q in out]


class Block:
    pass


class QrCase:
    """Blocks of one call laid into arenas.  ``A``: list of one or two flat arenas (canaries in the gaps); ``jobs``: the job table
    with ``a_off`` relative to the START of the block's arena -- run_qr turns that into the signed offset from ``a_base`` = lowest
    arena address + ``shift`` elements; ``Q0`` / ``R0``: NaN where a block goes, distinct finite canaries everywhere else."""


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


def make_case(name, cplx, shapes, hook=0, seed=0, shift=0, arena_of=None):
    rng = np.random.default_rng([1701, seed, int(cplx)])
    dt = np.complex128 if cplx else np.float64
    c = QrCase()
    c.name, c.cplx, c.hook, c.shift, c.dtype = name, cplx, hook, shift, dt
    # (a few small tall blocks join every batch, so that every kind finds a block on which it acts -- half of the mixed batch is
    # too small for that; the last one is Gaussian: wide and square Gaussian blocks are often too ill-conditioned to pin R)
    shapes = list(shapes) + SUPPORT
    kinds = assign_kinds(shapes, cplx) + ['gaussian']
    shapes = shapes + [PIN_BLOCK]
    arena_of = [0] * len(shapes) if arena_of is None else list(arena_of) + [0] * (len(SUPPORT) + 1)
    c.blocks = []
    for (m, n), kind, ar in zip(shapes, kinds, arena_of):
        b = Block()
        b.m, b.n, b.k, b.kind, b.arena = m, n, min(m, n), kind, ar
        b.a = make_block(rng, m, n, cplx, kind)
        # R is compared with the long double reference where it is well determined; an already reduced block is reproduced exactly
        b.compare_r = kind == 'triangular' or (kind in PINS_R and np.linalg.cond(b.a[:, :b.k]) <= WELL_CONDITIONED)
        b.r_ref = None
        c.blocks.append(b)
    c.A = []
    for ar in range(max(arena_of) + 1):
        mine = [b for b in c.blocks if b.arena == ar]
        offs, total = _lay(rng, [b.m * b.n for b in mine])
        arena = np.array(_canaries(total, cplx, 7 * ar), dtype=dt)
        for b, off in zip(mine, offs):
            b.a_off = off
            arena[off:off + b.m * b.n] = b.a.reshape(-1)
        c.A.append(arena)
    q_offs, q_total = _lay(rng, [b.m * b.k for b in c.blocks])
    r_offs, r_total = _lay(rng, [b.k * b.n for b in c.blocks], order=rng.permutation(len(c.blocks)))
    c.Q0, c.R0 = np.array(_canaries(q_total, cplx, 1), dtype=dt), np.array(_canaries(r_total, cplx, 2), dtype=dt)
    c.q_mask, c.r_mask = np.zeros(q_total, bool), np.zeros(r_total, bool)
    for b, qo, ro in zip(c.blocks, q_offs, r_offs):
        b.q_off, b.r_off = qo, ro
        c.q_mask[qo:qo + b.m * b.k] = True
        c.r_mask[ro:ro + b.k * b.n] = True
    c.Q0[c.q_mask], c.R0[c.r_mask] = _nan(dt), _nan(dt)
    c.jobs = np.array([[b.a_off, b.m, b.n, b.q_off, b.r_off, 0, 0, 0] for b in c.blocks], np.int64)
    return c


PIN_BLOCK = (12, 5)
SUPPORT = [(24, 10), (20, 9), (14, 7), (13, 6)]      # tall, so that they keep a batch on the one-launch-per-panel path
MIXED = [(1, 1), (1, 5), (5, 1), (7, 3), (3, 7), (9, 8), (16, 16), (17, 33)]
# the one-launch-per-panel path needs every block tall: the tall members of the mixed batch and the wide ones transposed
MIXED_TALL = [(1, 1), (5, 1), (7, 3), (9, 8), (16, 16), (33, 17), (5, 2), (12, 11)]
LA_BATCH = [(2048, 33), (600, 40), (257, 48), (64, 64), (35, 35), (41, 41), (49, 47)]

# name -> (complex, hook value of tpa_qr_set_algorithm, block shapes).  The name is the dispatch path the shapes select on the device.
QR_CASES = {
    'onewg_real': (False, 1, MIXED + [(50, 50), (300, 20), (33, 300)]),
    'onewg_complex': (True, 1, MIXED + [(50, 50), (300, 20), (33, 300)]),
    'onewg_real_k31': (False, 0, [(200, 31), (31, 90), (31, 31)] + MIXED),
    'onewg_complex_k31': (True, 0, [(200, 31), (31, 90), (31, 31)] + MIXED),
    'wy_k32_real': (False, 0, [(200, 32), (32, 32), (32, 90)] + MIXED),
    'wy_k32_complex': (True, 0, [(200, 32), (32, 32), (32, 90)] + MIXED),
    'wy_k32_tall_real': (False, 0, [(200, 32), (32, 32)] + MIXED_TALL),
    'wy_k32_tall_complex': (True, 0, [(200, 32), (32, 32)] + MIXED_TALL),
    'wy_la_real': (False, 0, LA_BATCH + MIXED_TALL),
    'wy_p8_real': (False, 0, LA_BATCH + [(40, 41)] + MIXED),
    'wy_p8_real_hook2': (False, 2, LA_BATCH + MIXED_TALL),
    'wy_p16_real_2049': (False, 0, [(2049, 40)] + MIXED),
    'wy_p16_real_4096': (False, 0, [(4096, 39)] + MIXED),
    'wy_p32_real_4097': (False, 0, [(4097, 40)] + MIXED),
    'wy_p32_real_8192': (False, 0, [(8192, 33)] + MIXED),
    'onewg_real_8193': (False, 0, [(8193, 33)] + MIXED),
    'wy_p4_complex': (True, 0, [(1024, 40), (300, 200), (33, 90)] + MIXED),
    'wy_p8_complex_1025': (True, 0, [(1025, 40)] + MIXED),
    'wy_p8_complex_2048': (True, 0, [(2048, 33)] + MIXED),
    'onewg_complex_2049': (True, 0, [(2049, 33)] + MIXED),
    'wy_wide_beyond_rows_real': (False, 0, [(40, 2100)] + MIXED),
    'wy_wide_beyond_rows_complex': (True, 0, [(40, 1100)] + MIXED),
}
# signed a_off: two arenas in one call, a_base = the lower arena address + ``shift`` elements, so that the blocks in front of it
# have negative offsets -- on one WY path and on the one-workgroup path
_NEG_SHAPES = [(9, 8), (40, 33), (7, 3), (64, 40), (3, 7), (16, 16)]
NEGATIVE_OFFSET_CASES = {
    'negative_a_off_wy_real': (False, 0), 'negative_a_off_wy_complex': (True, 0),
    'negative_a_off_onewg_real': (False, 1), 'negative_a_off_onewg_complex': (True, 1),
}

_cases = {}


def qr_case(name):
    if name not in _cases:
        seed = sorted(list(QR_CASES) + list(NEGATIVE_OFFSET_CASES)).index(name)
        if name in QR_CASES:
            cplx, hook, shapes = QR_CASES[name]
            _cases[name] = make_case(name, cplx, shapes, hook, seed)
        else:
            cplx, hook = NEGATIVE_OFFSET_CASES[name]
            # blocks 0, 1 lie in front of a_base (9 * 8 + 40 * 33 + gaps < 1500 elements of arena 0 precede it)
            _cases[name] = make_case(name, cplx, _NEG_SHAPES, hook, seed, shift=1500, arena_of=[0, 0, 0, 1, 1, 0])
    return _cases[name]


# ---- running -------------------------------------------------------------------------------------------------------------------

class qr_algorithm:
    """``with qr_algorithm(v):`` -- the process-global test hook tpa_qr_set_algorithm, back to 0 afterwards (it has no getter)."""

    def __init__(self, v, L=None):
        self.v, self.L = v, L

    def __enter__(self):
        self.L = self.L if self.L is not None else dev.lib()
        dev.check(self.L.tpa_qr_set_algorithm(self.v), "qr_set_algorithm")

    def __exit__(self, *exc):
        dev.check(self.L.tpa_qr_set_algorithm(0), "qr_set_algorithm")


def run_qr(c, L=None):
    """Upload, call, download -> dict(rc, A (the arenas after the call), Q, R, a_off (the signed offsets that were passed))."""
    L = L if L is not None else dev.lib()
    isz = np.dtype(c.dtype).itemsize
    Ad = [dev.to_device(a) for a in c.A]
    Qd, Rd = dev.to_device(c.Q0), dev.to_device(c.R0)
    ptrs = [a.data_ptr() for a in Ad]
    base = min(ptrs) + c.shift * isz
    jobs = c.jobs.copy()
    for j, b in zip(jobs, c.blocks):
        assert (ptrs[b.arena] - base) % isz == 0
        j[0] = (ptrs[b.arena] - base) // isz + b.a_off
    with qr_algorithm(c.hook, L):
        rc = L.tpa_qr_batch(int(c.cplx), jobs.ctypes.data, len(jobs), base, Qd.data_ptr(), Rd.data_ptr(), dev.stream())
        out = dict(rc=rc, A=[dev.to_host(a) for a in Ad], Q=dev.to_host(Qd), R=dev.to_host(Rd), a_off=jobs[:, 0].copy())
    return out


def r_reference(b):
    if b.r_ref is None:
        b.r_ref = qr_householder_ld(b.a)
    return b.r_ref


def check_qr(c, out):
    """Assertions 1 - 5 of the conformance tests on one call -> the largest error / bound per measure."""
    assert out['rc'] == 0, "%s: return code %d" % (c.name, out['rc'])
    for ar, (a0, a1) in enumerate(zip(c.A, out['A'])):
        assert np.array_equal(bits(a0), bits(a1)), "%s: the A arena %d changed" % (c.name, ar)
    Q, R = out['Q'], out['R']
    assert np.array_equal(bits(Q[~c.q_mask]), bits(c.Q0[~c.q_mask])), "%s: an element outside of every Q_b changed" % c.name
    assert np.array_equal(bits(R[~c.r_mask]), bits(c.R0[~c.r_mask])), "%s: an element outside of every R_b changed" % c.name
    f = _f(c.cplx)
    worst = dict(backward=0.0, orthogonality=0.0, rfactor=0.0)
    for i, b in enumerate(c.blocks):
        tag = "%s: block %d (%d x %d, %s)" % (c.name, i, b.m, b.n, b.kind)
        q = Q[b.q_off:b.q_off + b.m * b.k].reshape(b.m, b.k)
        r = R[b.r_off:b.r_off + b.k * b.n].reshape(b.k, b.n)
        assert not np.isnan(q.view(np.float64)).any(), tag + ": Q_b is not written completely"
        assert not np.isnan(r.view(np.float64)).any(), tag + ": R_b is not written completely"
        assert np.isfinite(q.view(np.float64)).all() and np.isfinite(r.view(np.float64)).all(), tag + ": Inf in the output"
        low = r[np.tril_indices(b.k, -1, b.n)]
        assert not bits(low.view(np.float64)).any(), tag + ": R below the diagonal is not +0.0"
        if c.cplx:
            assert np.all(np.diagonal(r).imag == 0), tag + ": the diagonal of R is not real"
        bw = float(np.max(qr_backward(b.a, q, r))) / (C_BACKWARD * f * EPS * np.sqrt(b.k))
        assert bw <= 1, tag + ": backward error / bound = %.3g" % bw
        orth = float(qr_orthogonality(q)) / (C_ORTH * f * EPS * np.sqrt(b.m))
        assert orth <= 1, tag + ": orthogonality / bound = %.3g" % orth
        worst['backward'], worst['orthogonality'] = max(worst['backward'], bw), max(worst['orthogonality'], orth)
        if b.compare_r:
            scale = _colnorm(_ld(b.a))
            err = _colnorm(_ld(r) - r_reference(b)) / np.where(scale > 0, scale, LD(1))
            rf = float(np.max(err)) / (C_RFACTOR * f * EPS * np.sqrt(b.k))
            assert rf <= 1, tag + ": R against the long double Householder reference / bound = %.3g (sign convention?)" % rf
            worst['rfactor'] = max(worst['rfactor'], rf)
    return worst


def check_repeatable(c, out, again):
    assert np.array_equal(bits(out['Q']), bits(again['Q'])), "%s: a second identical call gives another Q" % c.name
    assert np.array_equal(bits(out['R']), bits(again['R'])), "%s: a second identical call gives another R" % c.name


# ---- the pivoted panel variants through tpa_svd_batch ------------------------------------------------------------------------

# name -> (complex, m, n): one call per panel kernel of the rank-revealing QR (chosen from the largest block of the call)
SVD_CASES = {
    'qrp_64x8_real_500x48': (False, 500, 48), 'qrp_64x8_real_48x500': (False, 48, 500),
    'qrp_256x8_real_600x48': (False, 600, 48), 'qrp_256x8_real_48x600': (False, 48, 600),
    'qrp_256x16_real_2100x48': (False, 2100, 48),
    'qrp_256x32_real_48x4200': (False, 48, 4200),
    'qrp_256x4_complex_1000x48': (True, 1000, 48), 'qrp_256x4_complex_48x1000': (True, 48, 1000),
    'qrp_256x8_complex_1100x48': (True, 1100, 48), 'qrp_256x8_complex_48x1100': (True, 48, 1100),
}
SVD_RANK = 24


class SvdCase:
    pass


def sv_reference(a):
    """Extended-precision singular values (svd_reference.sv_reference, which is real: a complex matrix through its real embedding
    [[Re, -Im], [Im, Re]], whose singular values are those of the matrix, each twice)."""
    if not np.iscomplexobj(a):
        return svd_reference.sv_reference(a)
    return svd_reference.sv_reference(np.block([[a.real, -a.imag], [a.imag, a.real]]))[::2]


def svd_case(name):
    if name not in _cases:
        cplx, m, n = SVD_CASES[name]
        rng = np.random.default_rng([1702, sorted(SVD_CASES).index(name)])
        dt = np.complex128 if cplx else np.float64
        c = SvdCase()
        c.name, c.cplx, c.m, c.n, c.k, c.dtype = name, cplx, m, n, min(m, n), dt
        u0, _ = np.linalg.qr(_gauss(rng, m, SVD_RANK, cplx))
        v0, _ = np.linalg.qr(_gauss(rng, n, SVD_RANK, cplx))
        c.a = np.ascontiguousarray((u0 * np.logspace(0, -9, SVD_RANK)) @ v0.conj().T)
        c.sigma = sv_reference(c.a)
        sizes = dict(A=m * n, U=m * c.k, S=c.k, VH=c.k * n)
        c.off, c.arena0, c.mask = {}, {}, {}
        for i, (key, size) in enumerate(sizes.items()):
            (off,), total = _lay(rng, [size])
            arena = np.array(_canaries(total, cplx and key != 'S', 3 * i), dtype=np.float64 if key == 'S' else dt)
            mask = np.zeros(total, bool)
            mask[off:off + size] = True
            arena[mask] = c.a.reshape(-1) if key == 'A' else _nan(arena.dtype)
            c.off[key], c.arena0[key], c.mask[key] = off, arena, mask
        c.jobs = np.array([[c.off['A'], m, n, c.off['U'], c.off['S'], c.off['VH'], 0, 0]], np.int64)
        _cases[name] = c
    return _cases[name]


def run_svd(c, L=None, max_sweeps=60):
    """One call with tol = 0 -> dict(rc, A, U, S, VH: the arenas after the call)."""
    L = L if L is not None else dev.lib()
    d = {key: dev.to_device(c.arena0[key]) for key in ('A', 'U', 'S', 'VH')}
    wb = int(L.tpa_svd_worksize(int(c.cplx), c.jobs.ctypes.data, 1))
    work = dev.empty((wb + 7) // 8, np.float64)
    sweeps = ctypes.c_int()
    rc = L.tpa_svd_batch(int(c.cplx), c.jobs.ctypes.data, 1, d['A'].data_ptr(), d['U'].data_ptr(), d['S'].data_ptr(),
                         d['VH'].data_ptr(), work.data_ptr(), wb, max_sweeps, 0.0, ctypes.byref(sweeps), dev.stream())
    out = {key: dev.to_host(t) for key, t in d.items()}
    out['rc'] = rc
    return out


def check_svd(c, out):
    """The assertions on one call of a pivoted panel variant -> the largest error / bound per measure."""
    assert out['rc'] == 0, "%s: return code %d" % (c.name, out['rc'])
    assert np.array_equal(bits(out['A']), bits(c.arena0['A'])), c.name + ": the A arena changed"
    blk = {}
    for key in ('U', 'S', 'VH'):
        mask = c.mask[key]
        assert np.array_equal(bits(out[key][~mask]), bits(c.arena0[key][~mask])), "%s: an element outside of %s_b changed" % (c.name, key)
        blk[key] = out[key][mask]
        assert np.isfinite(blk[key].view(np.float64)).all(), "%s: %s_b is not written completely (NaN / Inf)" % (c.name, key)
    m, n, k = c.m, c.n, c.k
    u, s, vh = blk['U'].reshape(m, k), blk['S'], blk['VH'].reshape(k, n)
    assert np.all(s >= 0) and np.all(s[:-1] >= s[1:]), c.name + ": S is not descending"
    unit = _f(c.cplx) * EPS * np.sqrt(max(m, n))
    sigma1 = c.sigma[0]
    worst = {}
    worst['S'] = float(np.max(np.abs(s.astype(LD) - c.sigma)) / sigma1) / (C_SVD_S * unit)
    assert worst['S'] <= 1, c.name + ": |S - sigma| / bound = %.3g" % worst['S']
    res = _colnorm(_ld(c.a) - (_ld(u) * s.astype(LD)) @ _ld(vh)) / sigma1
    worst['residual'] = float(np.max(res)) / (C_SVD_RESIDUAL * unit)
    assert worst['residual'] <= 1, c.name + ": residual of U S VH / bound = %.3g" % worst['residual']
    live = s > 0
    assert live.sum() >= SVD_RANK, c.name + ": %d non-zero singular values, the matrix has rank %d" % (live.sum(), SVD_RANK)
    worst['orthogonality'] = max(float(qr_orthogonality(u[:, live])), float(qr_orthogonality(vh[live].conj().T))) / (C_SVD_ORTH * unit)
    assert worst['orthogonality'] <= 1, c.name + ": orthonormality of the vectors of S_i > 0 / bound = %.3g" % worst['orthogonality']
    if not live.all():
        dead = ~live
        assert not np.any(u[:, dead]) and not np.any(vh[dead]), c.name + ": a non-zero vector where S_i == 0"
        fro = np.sqrt(np.sum(np.abs(_ld(c.a)) ** 2))
        assert np.all(c.sigma[dead] <= np.sqrt(LD(k)) * 1e-15 * fro * 1.01), \
            c.name + ": a singular value above the rank threshold sqrt(k) 1e-15 |A|_F was set to zero"
    return worst


def svd_used_pivoted_qr(L):
    """The last row of the call log says that the call took the pivoted-QR path."""
    log = (ctypes.c_int64 * 8)()
    return L.tpa_svd_call_log(log, 1, 0) == 1 and log[4] == 1
