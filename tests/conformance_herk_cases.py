"""Seeded cases, runner and checker of the conformance suite of ``tpa_herk_chain`` (tests/test_conformance_herk.py).

A case is ONE launch: job tables and arenas as host numpy arrays.
  * The operand arena is NaN everywhere except on the elements that some link addresses (``conformance_gemm_cases.Arena``: guard zones
    of more than one operand tile around and between the blocks, NaN in the padding of a leading dimension); the weight vector is
    NaN outside the entries that some link addresses.  A kernel that reads one row, one k or one weight too far brings a NaN into C.
  * The C arena carries NaN on the elements of ``accumulate = 0`` tasks and numbers elsewhere (Hermitian with a real diagonal where a
    Hermitian task or a whole sector accumulates); every element that no task addresses (``ldc`` padding, gaps) keeps its bits.
  * Tasks of one launch: a Hermitian task over the whole operand (m x m); the same operand as a charge sector of two pipe slices --
    two Hermitian tasks on the diagonal and one general task below it whose mirror fills the rectangle above; and a general task
    without a mirror against a second operand.  ``split``: Abase and Bbase are two allocations (with the same contents) or one.

Tolerance (derived, not measured).  As in ``conformance_gemm_cases``: an element of C is a sum of K_tot = sum_l k_l products (complex
data: 2 K_tot real products per component) plus, when accumulating, C0, and whatever the order of the fused multiply-adds its
rounding error obeys gamma_N sum |terms|; that suite asserts |C - ref| <= f (K_tot + 2) EPS sum |terms| with f = 1 (real), 2
(complex), EPS = 2^-52.  Here every term is (s a) conj(b) with the weight multiplied into a first: fl(s a) = s a (1 + d), |d| <= EPS / 2,
which changes every term by at most EPS / 2 of its modulus -- one more EPS on the same magnitude sum is twice that.  So, per component,
        |C - ref| <= (f (K_tot + 2) + 1) EPS (sum |s| |a| |b| + |C0|)
evaluated on the case's own magnitude sum.  K_tot = 0 is exact: zeros, or C0 itself."""
import ctypes

import numpy as np

import conformance_gemm_cases as cg
import herk_reference as href
import kernel_reference as kref
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import _herk

EPS = 2.0**-52
WGUARD = 64
SEED = 20240911

M_LEVELS = (1, 15, 16, 17, 63, 64, 65, 129)
K_LEVELS = (1, 3, 4, 5, 16, 17)
LIVE_LINKS = (1, 2, 3, 5, 7)          # with the inserted empty link: chains of 1 .. 8 table rows, 1 .. 7 of them live
EMPTY_AT = ('none', 'first', 'middle', 'last')
WEIGHTS = ('absent', 'scalar', 'periodic', 'zeros', 'negative')
LAYOUTS = ('kfast', 'rowfast')
W_LEN, W_INNER = (2, 3), (1, 5)
FACTORS = dict(m=M_LEVELS, k=K_LEVELS, live=LIVE_LINKS, empty=EMPTY_AT, weights=WEIGHTS, lay=LAYOUTS, acc=(0, 1))


def design():
    """Rows of factor levels: the full (m, layout, accumulate) grid, the other factors on counters of coprime periods (6, 5, 4, 5),
    shifted per m so that they do not run in step with it.  Asserts that every level of every factor occurs, and every level of k,
    of the chain length, of the empty link and of the weights with both layouts and with both values of accumulate."""
    rows, i = [], 0
    for a, m in enumerate(M_LEVELS):
        for lay in LAYOUTS:
            for acc in (0, 1):
                rows.append(dict(m=m, lay=lay, acc=acc, k=K_LEVELS[(i + a) % 6], live=LIVE_LINKS[(i + 3 * a) % 5],
                                 empty=EMPTY_AT[(i // 2 + i + a) % 4], weights=WEIGHTS[(i + 2 * a) % 5]))
                i += 1
    for f in ('k', 'live', 'empty', 'weights'):
        for g in ('lay', 'acc'):
            seen = {(r[f], r[g]) for r in rows}
            assert all((x, y) in seen for x in FACTORS[f] for y in FACTORS[g]), (f, g)
    return rows


class Weights:
    """NaN-filled weight vector; only addressed entries get numbers."""

    def __init__(self, rng):
        self.rng, self.vals, self.size = rng, [], WGUARD

    def link(self, kind):
        """-> (w_off, w_len, w_inner) of a link whose weights are of `kind`."""
        rng = self.rng
        if kind == 'absent':
            return -1, int(rng.integers(1, 4)), int(rng.integers(1, 6))          # (w_len, w_inner are not looked at)
        w_inner = int(rng.choice(W_INNER))
        if kind == 'scalar':
            v = rng.standard_normal(1)
        elif kind == 'negative':
            v = -np.abs(rng.standard_normal(1)) - 0.1
        elif kind == 'periodic':
            v = rng.standard_normal(int(rng.choice(W_LEN)))
        else:                          # exact zeros: a zero scalar, or a period with a zero in it
            v = np.zeros(1) if rng.integers(3) == 0 else rng.standard_normal(int(rng.choice(W_LEN)))
            v[int(rng.integers(len(v)))] = 0.0
        off = self.size
        self.vals.append((off, v))
        self.size = off + len(v) + WGUARD
        return off, len(v), w_inner

    def build(self):
        w = np.full(self.size, np.nan)
        for off, v in self.vals:
            w[off:off + len(v)] = v
        return w


def _hermitian(rng, cplx, m):
    x = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if cplx else 0)
    x = np.tril(x) + np.tril(x, -1).conj().T
    x[np.arange(m), np.arange(m)] = x[np.arange(m), np.arange(m)].real
    return x


def make_case(cplx, row, rng, bt, shuffle=False, split=False, label=None):
    m, acc = row['m'], row['acc']
    X, W = cg.Arena(cplx, rng), Weights(rng)
    n2 = int(rng.choice([x for x in M_LEVELS if x <= 65]))
    m1 = int(rng.integers(1, m)) if m > 1 else 0          # the sector of m rows as two pipe slices of m1 and m - m1 rows

    def lay(name):
        return {'kfast': 'kfast', 'rowfast': 'outerfast'}[name]
    specs = [(row['k'], lay(row['lay']), row['weights'])]
    for _ in range(row['live'] - 1):
        specs.insert(int(rng.integers(len(specs) + 1)),
                     (int(rng.choice(K_LEVELS)), str(rng.choice(['kfast', 'outerfast', 'padded'])), str(rng.choice(WEIGHTS))))
    if row['empty'] != 'none':
        specs.insert({'first': 0, 'middle': max(1, len(specs) // 2), 'last': len(specs)}[row['empty']], (0, None, None))
    chain_h, chain_lo, chain_x, chain_g = [], [], [], []      # whole operand / second slice / second against first slice / against B
    for k, la, wk in specs:
        if k == 0:      # an empty link points into the leading NaN guard zones: whoever used it would bring NaN into C
            e = _herk.link_row(int(rng.integers(cg.GUARD // 2)), int(rng.integers(cg.GUARD // 2)), 0, 1, 1, 1, 1,
                               int(rng.integers(WGUARD // 2)), 1, 1)
            for ch in (chain_h, chain_lo, chain_x, chain_g):
                ch.append(list(e))
            continue
        a_off, a_rs, a_ks = X.block(m, k, la)
        b_off, b_rs, b_ks = X.block(n2, k, str(rng.choice(['kfast', 'outerfast', 'padded'])))
        w = W.link(wk)
        chain_h.append(_herk.link_row(a_off, a_off, k, a_rs, a_ks, a_rs, a_ks, *w))
        chain_lo.append(_herk.link_row(a_off + m1 * a_rs, a_off + m1 * a_rs, k, a_rs, a_ks, a_rs, a_ks, *w))
        chain_x.append(_herk.link_row(a_off + m1 * a_rs, a_off, k, a_rs, a_ks, a_rs, a_ks, *w))
        chain_g.append(_herk.link_row(a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, *w))
    nl = len(specs)
    links = chain_h + chain_lo + chain_x + chain_g

    # ---- C arena: [gap] whole block [gap] sector block [gap] general block [gap]
    acc_s, acc_g = 1 - acc, int(rng.integers(2))
    pieces, size = [], int(rng.integers(1, 40))

    def block(rows, cols, acc_, herm):
        nonlocal size
        ldc = cols + int(rng.integers(1, 8))
        v = rng.standard_normal((rows, ldc)) + (1j * rng.standard_normal((rows, ldc)) if cplx else 0)
        if not acc_:
            v[:, :cols] = np.nan
        elif herm:
            v[:, :cols] = _hermitian(rng, cplx, rows)
        off = size
        pieces.append((off, v.reshape(-1)))
        size += rows * ldc + int(rng.integers(1, 40))
        return off, ldc
    o1, ld1 = block(m, m, acc, True)
    tasks = [_herk.task_row(o1, m, m, ld1, 0, nl, acc, 1)]
    if m > 1:
        o2, ld2 = block(m, m, acc_s, True)
        tasks.append(_herk.task_row(o2, m1, m1, ld2, 0, nl, acc_s, 1))
        tasks.append(_herk.task_row(o2 + m1 * ld2 + m1, m - m1, m - m1, ld2, nl, nl, acc_s, 1))
        tasks.append(_herk.task_row(o2 + m1 * ld2, m - m1, m1, ld2, 2 * nl, nl, acc_s, 0, o2 + m1, ld2))
    o3, ld3 = block(m, n2, acc_g, False)
    tasks.append(_herk.task_row(o3, m, n2, ld3, 3 * nl, nl, acc_g, 0))
    C0 = rng.standard_normal(size) + (1j * rng.standard_normal(size) if cplx else 0)
    for off, v in pieces:
        C0[off:off + len(v)] = v

    c = cg.Case()
    c.cplx, c.split = cplx, split
    order = rng.permutation(len(tasks))                    # the tasks of one sector are not neighbours in the task table
    c.tasks = np.array([tasks[i] for i in order], np.int64)
    c.links = np.array(links, np.int64)
    c.tiles = _herk.tile_table(c.tasks, c.links, bt)
    if shuffle:
        c.tiles = c.tiles[rng.permutation(len(c.tiles))]
    c.A, c.w, c.C0 = X.build(), W.build(), C0
    c.label = label or ('%s split=%d ' % ('complex' if cplx else 'real', split) + ' '.join('%s=%s' % kv for kv in row.items()))
    return c


def tile_rows(cplx):
    from tenpy_amd import _lib
    bt = ctypes.c_int()
    _lib.load().tpa_herk_tile_shape(int(cplx), ctypes.byref(bt))
    return bt.value


def cases(cplx, seed=SEED):
    """The seeded cases of one dtype: the design plus all-empty chains (accumulate 0 and 1)."""
    bt = tile_rows(cplx)
    rng = np.random.default_rng([seed, int(cplx)])
    for i, row in enumerate(design()):
        yield make_case(cplx, row, rng, bt, shuffle=bool(i % 2), split=bool((i // 2) % 2))
    for acc in (0, 1):
        row = dict(m=65, lay='kfast', acc=acc, k=0, live=1, empty='none', weights='scalar')
        c = make_case(cplx, dict(row, k=3), rng, bt)
        c.links[:, 2] = 0                                  # every link empty: zeros over the NaN-filled C / C bit-identical
        c.tiles = _herk.tile_table(c.tasks, c.links, bt)
        c.label = 'all links empty acc=%d' % acc
        yield c


def run_case(c, L=None):
    """Upload, launch, download -> the C arena after the launch."""
    L = L if L is not None else dev.lib()
    d = [dev.to_device(x) for x in (c.tasks, c.links, c.tiles, c.A, c.w, c.C0)]
    B = dev.to_device(c.A) if c.split else d[3]
    dev.check(L.tpa_herk_chain(int(c.cplx), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(c.tiles), d[3].data_ptr(),
                               B.data_ptr(), d[4].data_ptr(), d[5].data_ptr(), dev.stream()), "herk_chain")
    return dev.to_host(d[5])


def reference(c):
    if getattr(c, 'ref', None) is None:
        c.ref = href.herk_chain(c.cplx, c.tasks, c.links, c.A, c.A, c.w, c.C0)
    return c.ref


def bound(c):
    ref = reference(c)
    return ((2 if c.cplx else 1) * (ref['ktot'] + 2) + 1) * EPS * ref['mag']


def check_case(c, C):
    """-> largest error / bound of the case (0.0 when every bound is zero); raises AssertionError with the case's label."""
    ref = reference(c)
    mask = ref['mask']
    assert C.shape == c.C0.shape and C.dtype == c.C0.dtype, c.label
    assert np.array_equal(kref.bits(C[~mask]), kref.bits(c.C0[~mask])), "an element that no task addresses changed: " + c.label
    got = C[mask]
    assert np.all(np.isfinite(got.view(np.float64))), "NaN / Inf in the output: " + c.label
    lim = bound(c)[mask]
    gr, gi = kref.split(got)
    err = np.maximum(np.abs(gr - ref['re'][mask]), np.abs(gi - ref['im'][mask]))
    bad = err > lim
    assert not bad.any(), "%d elements beyond the bound, worst err / bound = %.3g: %s" % (
        bad.sum(), float(np.max(err[bad] / np.maximum(lim[bad], np.finfo(np.longdouble).tiny))), c.label)
    exact = ref['ktot'][mask] == 0       # an all-empty chain: zeros, or C0 bit for bit
    if exact.any():
        want = np.where(ref['acc'][mask][exact], c.C0[mask][exact], 0)
        assert np.array_equal(kref.bits(got[exact] + 0.0), kref.bits(want + 0.0)), "an all-empty chain is not exact: " + c.label
    for c_off, m, ldc in ref['herm']:    # Hermitian bit for bit, the diagonal exactly real
        blk = C[c_off + np.arange(m)[:, None] * ldc + np.arange(m)[None, :]]
        lo = np.tril_indices(m, -1)
        assert np.array_equal(kref.bits(blk.T[lo]), kref.bits(blk[lo].conj())), "C[j,i] != conj(C[i,j]) in bits: " + c.label
        if c.cplx:
            assert np.all(np.diagonal(blk).imag == 0.0), "Im C[i,i] != 0: " + c.label
    for c_off, m, n, ldc, m_off, m_ld in ref['mirrors']:
        blk = C[c_off + np.arange(m)[:, None] * ldc + np.arange(n)[None, :]]
        mir = C[m_off + np.arange(n)[:, None] * m_ld + np.arange(m)[None, :]]
        assert np.array_equal(kref.bits(mir.T.copy()), kref.bits(blk.conj())), "the mirror is not conj(C)^T in bits: " + c.label
    nz = lim > 0
    return float(np.max(err[nz] / lim[nz])) if nz.any() else 0.0
