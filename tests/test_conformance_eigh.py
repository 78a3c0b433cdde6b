"""Conformance of the Hermitian eigensolver kernels (K7 of include/tenpy_amd.h; csrc/tpa_svd.hip): ``tpa_eigh_batch`` on every route,
``tpa_eigh_worksize``, ``tpa_eigh_set_direct`` and ``tpa_eigh_from_svd``.  Every case runs on the numpy emulation (LAPACK) and, marked
``gpu``, on the HIP kernels; the test id names the route of the device, and the gpu half asserts through ``tpa_eigh_last_direct`` that
the call took it.

What one call is held to (tests/conformance_eigh_cases.py::check_eigh): A, W and V are three unrelated arenas with canaries in every
gap and mutually unrelated offsets; W and V start NaN-filled where a block goes; every element of every block is written; all canaries
and the whole A arena are bit-identical; the eigenvalues ascend exactly and are compared with a long double reference of the matrix the
LOWER triangle defines (upper triangle NaN / 1e8 |A|_F of garbage / imaginary parts on the diagonal change nothing); residual per
vector and orthogonality in long double; a diagonal block comes out exactly; a second identical call is bit-identical.

BOUNDS.  eps = 2^-53, f = 4 for complex data, |A|_F of the matrix defined by the lower triangle:
    |w_i - lambda_i| <= c_w f eps sqrt(n) |A|_F,   |A v_i - w_i v_i|_2 <= c_r f eps sqrt(n) |A|_F,   |V^H V - I|_col <= c_o f eps sqrt(n).
c is calibrated on the REFERENCE implementation, never on the kernels: the committed cases run through the emulation (LAPACK syevd /
heevd), c = 8 x (the largest ratio LAPACK reaches), rounded up to a power of two.  The margin of 8 covers the summation order on the
matrix cores and Jacobi against tridiagonalisation.  Measured with LAPACK (OpenBLAS, x86-64), largest over all committed cases (the
mock halves of the tests print them as CALIBRATION lines and assert the margin):

    measure                                   LAPACK ratio   x 8      c
    eigenvalues against long double           1.13           9.03     16
    residual per vector                       1.96           15.6     16
    orthogonality of V                        5.48           43.8     64
    from_svd: err against long double         0.126          1.01     2

THE DEVICE ROUTES.  Orthogonality and the err of tpa_eigh_from_svd are held to the bounds above on the device too.  Eigenvalues and
residuals are not: every route of tpa_eigh_batch iterates on A' = A + mu, mu = 2 |A|_F, and stops when no
|S_ij| > 2^-52 sqrt(n) sqrt(S_ii S_jj) is left (include/tenpy_amd.h; the kernels' constant is DBL_EPSILON = 2^-52 = 2 eps, csrc/tpa_svd_b32.inc
`2.220446049250313e-16 * sqrt(L)`).  What that rule guarantees, in units u = eps sqrt(n) |A|_F with eps = 2^-53:
  - the spectrum of A' lies in [|A|_F, 3 |A|_F], so every off-diagonal element that is left is <= 2 * 3 u = 6 u; the remainder E has
    at most n (n - 1) of them, |E|_2 <= |E|_F <= 6 n u, and by Weyl's theorem that is what the eigenvalues (diag S - mu) may be off
    by; one column of E has norm <= 6 sqrt(n) u: the residual of one vector;
  - the transformations act on A', whose norm is |A'|_F <= |A|_F + mu sqrt(n) = (1 + 2 sqrt(n)) |A|_F: rounding errors of LAPACK's
    class ON THAT MATRIX are c f (1 + 2 sqrt(n)) u, with the c of the table.
  => |w_i - lambda_i| <= (6 n + c_w f (1 + 2 sqrt(n))) u,   |A v_i - w_i v_i|_2 <= (6 sqrt(n) + c_r f (1 + 2 sqrt(n))) u.
This is what the gpu halves assert (conformance_eigh_cases.bound_factors); the shift costs a factor ~2 sqrt(n) against LAPACK's class
on A itself, and the header says so.  (A first version of this derivation took the rule's constant for 2^-53 and had 3 n / 3 sqrt(n):
the 64-row graded rank-deficient block of two_sided_real, residual 297 u on the MI355X, stood 0.3 % above that bound of 296 u; with
the constant the kernels use the bound is 320 u.  That block is the one closest to its bound: its 32-fold eigenvalue mu of A' keeps
the rotations going at rounding level for many sweeps.)  Measured on the MI355X, largest over the blocks of two_sided_real (units u):
eigenvalues 297 (n = 64, graded), 128 (n = 96, clusters), 79 (n = 161, Gaussian), where LAPACK reaches 1 - 2.
"""
import os

import numpy as np
import pytest

import conformance_eigh_cases as ce
from kernel_reference import bits
from tenpy_amd import _lib
from tenpy_amd.linalg import _device as dev

_C = dict(eigenvalues=ce.C_W, residual=ce.C_RESIDUAL, orthogonality=ce.C_ORTH, err=ce.C_ERR)


def _report(what, inst, ratios):
    print("CONFORMANCE %s %s %s" % (what, inst, " ".join("%s=%.4f" % kv for kv in sorted(ratios.items()))))


def _lapack_calibration(what, name, ratios):
    """The emulation is LAPACK: c was chosen a factor 8 .. 16 above the largest ratio it reaches over the cases, so every case stays
    a factor 8 below its bound.  (Asserted with a factor 4: another build of LAPACK sums in another order.)  The printed lines
    are what the table in the docstring was made from."""
    for key, v in sorted(ratios.items()):
        print("CALIBRATION %s %s %s: LAPACK ratio %.3f, c = %d" % (what, name, key, v * _C[key], _C[key]))
    assert all(v <= 1 / 4 for v in ratios.values()), (name, ratios)


# ---- the cases and the reference themselves (no device) ---------------------------------------------------------------------------

def test_long_double_reference_on_exactly_known_spectra():
    """A diagonal matrix and 2 x 2 blocks with integer entries whose eigenvalues are integers: the reference returns them to
    long double rounding, with the off-diagonal norm it promises."""
    d = np.array([3., -7., 0., 12., 5., -1.])
    lam, off = ce.eigenvalues_ld(np.diag(d))
    assert np.array_equal(lam, np.sort(d).astype(ce.LD)) and off == 0
    # [[a, b], [b, c]] with (a - c)^2 + 4 b^2 a perfect square: [[1, 2], [2, -2]] -> -3, 2;  [[6, 12], [12, -1]] -> -10, 15;
    # complex [[2, 3 + 4i], [3 - 4i, 2]] -> -3, 7
    for cplx in (False, True):
        h = np.zeros((6, 6), complex if cplx else float)
        h[0:2, 0:2] = [[1, 2], [2, -2]]
        h[2:4, 2:4] = [[6, 12], [12, -1]]
        h[4:6, 4:6] = [[2, 3 + 4j], [3 - 4j, 2]] if cplx else [[2, 5], [5, 2]]
        perm = np.random.default_rng(1).permutation(6)
        h = h[np.ix_(perm, perm)]
        lam, off = ce.eigenvalues_ld(h)
        want = np.array([-10, -3, -3, 2, 7, 15], ce.LD)
        assert np.max(np.abs(lam - want)) <= 8 * np.finfo(ce.LD).eps * 15 and off <= ce.REF_OFFDIAG
        # the measures on an exact decomposition: LAPACK's vectors of a diagonal matrix
        w, v = np.linalg.eigh(np.diag(d).astype(h.dtype))
        assert np.max(ce.eig_residual(np.diag(d), w, v)) == 0 and ce.orthogonality(v) == 0


def test_reference_converged_on_every_committed_block():
    assert np.finfo(ce.LD).eps <= 2.0 ** -63, "the checkers need an extended-precision long double"
    for name in ce.EIGH_CASES:
        for b in ce.eigh_case(name).blocks:
            ce.reference(b)
            assert b.offdiag <= ce.REF_OFFDIAG, (name, b.n, b.kind, float(b.offdiag))


def test_every_kind_sits_on_a_block_where_it_acts():
    for name, (cplx, key, sizes, direct, alg, route) in ce.EIGH_CASES.items():
        c = ce.eigh_case(name)
        kinds = ce.KINDS_COMPLEX if cplx else ce.KINDS_REAL
        # the data sets with few blocks hold the leading kinds (the triangle that is read, diagonal, multiplicities)
        for kind in (kinds if key in ce.EVERY_KIND else kinds[:5]):
            assert [b for b in c.blocks if b.kind == kind and ce.acts(kind, b.n)], "%s: no block on which '%s' acts" % (name, kind)
        assert [b.n for b in c.blocks[:len(sizes)]] == list(sizes) and c.blocks[0].kind == 'gaussian'
        for b in c.blocks:          # the properties, not the labels
            n, a, lam = b.n, b.a, np.asarray(ce.reference(b), float)
            fro = float(b.fro)
            up, low = a[np.triu_indices(n, 1)], a[np.tril_indices(n)]
            assert np.isfinite(low.view(np.float64)).all()
            if b.kind not in ce.SAME_AS_CLEAN:
                assert np.array_equal(np.tril(a, -1), np.tril(b.h, -1)) and np.allclose(a, b.h, rtol=0, atol=4 * ce.EPS * fro)
            if b.kind == 'gaussian' and n >= 3:
                assert lam[0] < 0 < lam[-1]
            elif b.kind == 'psd_flat':
                assert lam[0] >= -ce.EPS * fro and lam[-1] > 0
            elif b.kind == 'graded_rank_deficient':
                assert np.sum(np.abs(lam) <= 1e-15 * fro) >= n - n // 2 and lam[-1] / lam[n - n // 2 + 1] >= 1e8
            elif b.kind == 'pm_pairs':
                assert lam[0] < -0.9 and np.max(np.abs(lam + lam[::-1])) <= 1e-14 * fro
            elif b.kind == 'clusters':
                trip = [k for k in range(n - 2) if lam[k + 2] - lam[k] <= 1e-14 * fro]
                assert any(lam[k] > 0.5 for k in trip) and any(lam[k] < -0.5 for k in trip)
            elif b.kind == 'diagonal':
                d = np.diagonal(a).real
                assert not (a - np.diag(np.diagonal(a))).any() and d.min() < 0 < d.max() and np.any(np.diff(d) < 0)
                assert np.sqrt(np.sum(d * d)) == np.round(np.sqrt(np.sum(d * d))) and np.array_equal(d, np.round(d))
            elif b.kind == 'zero':
                assert not a.any()
            elif b.kind == 'multiple_of_identity':
                assert np.array_equal(a, a[0, 0] * np.eye(n)) and a[0, 0] != 0
            elif b.kind == 'scaled_up':
                assert fro > 1e97
            elif b.kind == 'scaled_down':
                assert 0 < fro < 1e-97
            elif b.kind == 'upper_nan':
                assert len(up) and np.isnan(up.view(np.float64)).all()
            elif b.kind == 'upper_large':
                assert len(up) and np.isfinite(up.view(np.float64)).all() and np.min(np.abs(up)) >= 1e8 * fro
            elif b.kind == 'diag_imag':
                assert np.all(np.diagonal(a).imag != 0) and not np.diagonal(b.h).imag.any()
        assert np.isnan(c.W0[c.w_mask]).all() and np.isfinite(c.W0[~c.w_mask]).all()
        assert np.isnan(c.V0[c.v_mask].view(np.float64)).all() and np.isfinite(c.V0[~c.v_mask].view(np.float64)).all()
        for mask in (c.w_mask, c.v_mask):      # a canary in front of, between and behind the blocks
            assert not mask[0] and not mask[-1] and len(np.flatnonzero(mask[1:] & ~mask[:-1])) == len(c.blocks)
        # the three offsets are mutually unrelated: the blocks stand in another order in every arena
        order = [list(np.argsort(c.jobs[:, k])) for k in (0, 2, 3)]
        assert order[0] != order[1] and order[1] != order[2] and order[0] != order[2], name


# ---- tpa_eigh_batch on every route ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", list(ce.EIGH_CASES))
def test_eigh_batch(backend, path):
    c = ce.eigh_case(path)
    if backend == 'gpu':       # (tpa_eigh_batch reads TPA_EIGH_DIRECT on every call, the library TPA_SVD_DYN when it is loaded)
        assert 'TPA_EIGH_DIRECT' not in os.environ and 'TPA_SVD_DYN' not in os.environ, "the test ids name the routes of the default switches"
    out = ce.run_eigh(c)
    if backend == 'gpu':
        assert out['direct'] == c.route, "%s: tpa_eigh_last_direct() = %d, the id names the other route" % (path, out['direct'])
    ratios = ce.check_eigh(c, out, shifted=(backend == 'gpu'))
    _report("tpa_eigh_batch[%s]" % backend, path, ratios)
    if backend == 'mock':
        _lapack_calibration("eigh", path, ratios)
    ce.check_repeatable(c, out, ce.run_eigh(c))


# ---- argument behaviour ---------------------------------------------------------------------------------------------------------

def _small_call(cplx, ns=(5, 3)):
    """A well-formed call of two small blocks -> (jobs, A, W0, V0); outputs NaN-filled with a canary behind."""
    dt = np.complex128 if cplx else np.float64
    rng = np.random.default_rng(21)
    blocks = [ce.make_block(rng, n, cplx, 'gaussian') for n in ns]
    A = np.concatenate([b.reshape(-1) for b in blocks])
    W0 = np.concatenate([np.full(sum(ns), np.nan), [5.0]])
    V0 = np.concatenate([np.full(len(A), ce._nan(dt), dt), np.array([7.0], dt)])
    jobs, ao, wo = [], 0, 0
    for n in ns:
        jobs.append([ao, n, wo, ao, 0, 0, 0, 0])
        ao, wo = ao + n * n, wo + n
    return jobs, A, W0, V0


def _bit_untouched(out, A, W0, V0):
    return np.array_equal(bits(out['A']), bits(A)) and np.array_equal(bits(out['W']), bits(W0)) and np.array_equal(bits(out['V']), bits(V0))


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_eigh_arguments(backend, cplx):
    L = dev.lib()
    jobs, A, W0, V0 = _small_call(cplx)
    out = ce.call_eigh(L, cplx, jobs, A, W0, V0)
    assert out['rc'] == 0 and not np.isnan(out['W'][:-1]).any() and out['W'][-1] == 5.0          # the call itself is well-formed
    out = ce.call_eigh(L, cplx, [], A, W0, V0)                                                   # n_jobs = 0
    assert out['rc'] == 0 and _bit_untouched(out, A, W0, V0) and out['worksize'] > 0
    for n in (0, -3):
        out = ce.call_eigh(L, cplx, [jobs[0], [25, n, 5, 25, 0, 0, 0, 0]], A, W0, V0)
        assert out['rc'] == _lib.E_BADARG and _bit_untouched(out, A, W0, V0), "outputs written before the argument check"
    out = ce.call_eigh(L, cplx, jobs, A, W0, V0, dtype_code=2)
    assert out['rc'] == _lib.E_BADARG and _bit_untouched(out, A, W0, V0)
    out = ce.call_eigh(L, cplx, jobs, A, W0, V0, work_bytes=out['worksize'] - 1)
    assert out['rc'] == _lib.E_BADARG and _bit_untouched(out, A, W0, V0)
    with pytest.raises(ValueError):
        _lib.check(out['rc'], "eigh")


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_eigh_worksize_does_not_depend_on_the_hook(backend, cplx):
    L = dev.lib()
    sizes = []
    for direct in (0, 1):
        with ce.eigh_hooks(L, direct, 0):
            sizes.append([int(L.tpa_eigh_worksize(int(cplx), ce.eigh_case(name).jobs.ctypes.data, len(ce.eigh_case(name).jobs)))
                          for name in ('small_c' if cplx else 'small_b32', 'two_sided_complex' if cplx else 'two_sided_real')])
    assert sizes[0] == sizes[1] and min(sizes[0]) > 0
    assert int(L.tpa_eigh_worksize(int(cplx), None, 0)) > 0


# ---- non-finite input in the triangle that is read: TPA_E_NAN, decided by the norm ----------------------------------------------

@pytest.mark.parametrize("which", ['n9_real', 'n9_complex', 'diagonal_n100_real'])
def test_eigh_nan_in_the_lower_triangle(backend, which):
    """K5's rule: NaN / Inf in the data that is read is TPA_E_NAN (-> ValueError), outputs untouched.  The diagonal block of 100 rows
    with one NaN below the diagonal is the case that used to pass silently: no pair of it needs a rotation on the two-sided route, and
    its eigenvalues are the (finite) diagonal."""
    L = dev.lib()
    cplx = which.endswith('complex')
    rng = np.random.default_rng(22)
    if which.startswith('n9'):
        a, (i, j), bad = ce.make_block(rng, 9, cplx, 'gaussian'), (6, 2), (np.inf if cplx else np.nan)
    else:
        a, (i, j), bad = ce.make_block(rng, 100, cplx, 'diagonal'), (70, 3), np.nan
    n, dt = a.shape[0], a.dtype
    W0, V0 = np.full(n + 1, np.nan), np.full(n * n + 1, ce._nan(dt), dt)
    W0[-1], V0[-1] = 5.0, 7.0
    below, above = a.copy(), a.copy()
    below[i, j], above[j, i] = bad, bad
    out = ce.call_eigh(L, cplx, [[0, n, 0, 0, 0, 0, 0, 0]], below.reshape(-1), W0, V0)
    assert out['rc'] == _lib.E_NAN, "return code %d" % out['rc']
    assert _bit_untouched(out, below.reshape(-1), W0, V0)
    with pytest.raises(ValueError):
        _lib.check(out['rc'], "eigh")
    out = ce.call_eigh(L, cplx, [[0, n, 0, 0, 0, 0, 0, 0]], above.reshape(-1), W0, V0)      # the same above the diagonal is no error
    assert out['rc'] == 0 and np.isfinite(out['W'][:-1]).all() and np.isfinite(out['V'][:-1].view(np.float64)).all()
    assert out['W'][-1] == 5.0 and out['V'][-1] == 7.0


# ---- max_sweeps exhausted (the emulation has no sweeps) ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_eigh_max_sweeps_exhausted(cplx):
    _lib.require_gpu()
    L = dev.lib()
    dt = np.complex128 if cplx else np.float64
    a = ce.make_block(np.random.default_rng(23), 40, cplx, 'gaussian')
    A = np.concatenate([np.array([11.0, 12.0], dt), a.reshape(-1), np.array([13.0], dt)])
    W0, V0 = np.full(40 + 3, np.nan), np.full(1600 + 4, ce._nan(dt), dt)
    W0[[0, -2, -1]], V0[[0, 1, 2, -1]] = [1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0]
    out = ce.call_eigh(L, cplx, [[2, 40, 1, 3, 0, 0, 0, 0]], A, W0, V0, max_sweeps=1)
    assert out['rc'] == _lib.E_NOCONV, "return code %d" % out['rc']
    assert np.array_equal(bits(out['A']), bits(A)), "the A arena changed"
    assert np.array_equal(bits(out['W'][[0, -2, -1]]), bits(W0[[0, -2, -1]])) and np.array_equal(bits(out['V'][[0, 1, 2, -1]]), bits(V0[[0, 1, 2, -1]]))
    with pytest.raises(np.linalg.LinAlgError):
        _lib.check(out['rc'], "eigh")
    out = ce.call_eigh(L, cplx, [[2, 40, 1, 3, 0, 0, 0, 0]], A, W0, V0)          # the same call with sweeps to spare
    assert out['rc'] == 0 and out['sweeps'] > 1 and np.isfinite(out['W']).all()


# ---- tpa_eigh_from_svd --------------------------------------------------------------------------------------------------------

FROM_SVD = [(k, False) for k in ce.FROM_SVD_KINDS_REAL] + [(k, True) for k in ce.FROM_SVD_KINDS_COMPLEX]


@pytest.mark.parametrize("kind,cplx", FROM_SVD, ids=["%s_%s" % (k, 'complex' if c else 'real') for k, c in FROM_SVD])
def test_eigh_from_svd(backend, kind, cplx):
    c = ce.from_svd_case(kind, cplx)
    assert [b.n for b in c.blocks] == ce.FROM_SVD_N and np.array_equal(bits(c.arena0['err'][:3]), bits(np.array(ce.STALE_ERR)))
    out = ce.run_from_svd(c)
    worst = ce.check_from_svd(c, out)
    _report("tpa_eigh_from_svd[%s]" % backend, c.name, dict(err=worst))
    if backend == 'mock':
        _lapack_calibration("eigh_from_svd", c.name, dict(err=worst))
    ce.check_from_svd_repeatable(c, out, ce.run_from_svd(c))


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_eigh_from_svd_arguments(backend, cplx):
    L = dev.lib()
    c = ce.from_svd_case('aligned', cplx)
    out = ce.call_from_svd(L, cplx, [], c.arena0)                        # n_jobs = 0
    assert out['rc'] == 0 and all(np.array_equal(bits(out[k]), bits(c.arena0[k])) for k in c.arena0)
    for n in (0, -2):
        jobs = c.jobs.copy()
        jobs[-1, 1] = n
        out = ce.call_from_svd(L, cplx, jobs, c.arena0)
        assert out['rc'] == _lib.E_BADARG
        assert np.array_equal(bits(out['lam']), bits(c.arena0['lam'])), "lam written before the argument check"
    out = ce.call_from_svd(L, cplx, c.jobs, c.arena0, dtype_code=2)
    assert out['rc'] == _lib.E_BADARG and np.array_equal(bits(out['lam']), bits(c.arena0['lam']))
