"""Seeded cases, runner and checker of the GEMM conformance suite (tests/test_conformance_gemm.py; the mutation test in
tests/test_conformance_mutations.py drives the same checker with a deliberately broken device library).

A case is a set of job tables and arenas (host numpy arrays):
  * A / B arenas are NaN everywhere except on the elements that some link addresses: the padding of a leading dimension, the guard
    zones of GUARD elements (more than one 128 x 16 operand tile) around and between the operand blocks.  A kernel that reads one row,
    one column or one k beyond an operand block brings a NaN into C;
  * the C arena carries NaN on the elements of ``accumulate = 0`` tasks, random numbers elsewhere; every element that no task
    addresses (``ldc`` padding, gaps between blocks) has to keep its bit pattern.

Tolerance (derived, not measured).  Every element of C is a sum of K_tot = sum_l k_l products (complex data: 2 K_tot real products per
component) plus, when accumulating, C0.  Whatever the order of the fused multiply-adds, the rounding error of such a sum obeys
``gamma_N sum |terms|`` with ``gamma_N = N u / (1 - N u)``, N the number of additions and u = 2^-53 (Higham, Accuracy and Stability of
Numerical Algorithms, section 3.1).  With EPS = 2^-52 = 2 u the test asserts, per component,
        |C - ref| <= f (K_tot + 2) EPS (sum |a| |b| + |C0|),        f = 1 (real), 2 (complex),
which is that bound with a factor of about two in hand (N = f K_tot + 1 additions; the factor also covers the 2^-64 rounding of the
longdouble reference and of the float64 moduli |a|, |b|).  K_tot = 0 is exact: zeros, or C0 itself."""
import ctypes
import itertools
import os

import numpy as np

import kernel_reference as kref
from tenpy_amd.linalg import _device as dev

EPS = 2.0**-52
GUARD = 2304

M_LEVELS = (1, 15, 16, 17, 31, 33, 63, 64, 65, 127, 128, 129, 191, 193)
K_LEVELS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 100)
LAYOUTS = ('kfast', 'outerfast', 'padded', 'general', 'unit_unit')
EXTRA_LINKS = (0, 1, 3, 10)                 # links besides the focus link (and besides the inserted empty link): chains of 1 .. 12
EMPTY_AT = ('none', 'first', 'middle', 'last')
SEEDS = (20240607,)

# name in the test id -> (complex, cfg, tpa_gemm_set_variant); see the dispatch at the end of csrc/tpa_gemm.hip
INSTANTIATIONS = {
    'chain2_128x64x4x2_real_cfg0': (False, 0, 0),
    'chain_64x64x1x2_real_cfg1': (False, 1, 0),
    'chain2_64x64x2x2_real_cfg1_variant': (False, 1, 1),
    'chain_64x32x2x1_complex_cfg1': (True, 1, 0),
    'chain_128x64x4x2_complex_cfg0': (True, 0, 0),
}


def factor_levels(cplx):
    return dict(m=M_LEVELS, n=M_LEVELS, k=K_LEVELS, lay_a=LAYOUTS, lay_b=LAYOUTS, flags=(0, 1, 2, 3) if cplx else (0, 3),
                acc=(0, 1), extra=EXTRA_LINKS, empty=EMPTY_AT)


def pairwise_design(cplx, seed):
    """Rows of factor levels such that every pair of levels of two different factors occurs in at least one row: the full (m, n) grid
    with the other factors on shifted diagonals, then rows that pack the pairs that are still missing.  Asserts the coverage."""
    rng = np.random.default_rng(seed)
    lv = factor_levels(cplx)
    names = list(lv)
    rows = []
    # the full (m, n) grid; factor X takes level perm_X[(a_X i + b_X j) mod 14] with a_X, b_X units of Z_14: every level of X meets
    # every m (j runs) and every n (i runs); different (a, b) per factor decorrelate the factors from each other
    mult = [(1, 1), (1, 3), (1, 5), (1, 9), (1, 11), (1, 13), (3, 1)]
    L = len(M_LEVELS)
    perm = {f: [lv[f][i % len(lv[f])] for i in rng.permutation(L)] for f in names[2:]}
    for i, m in enumerate(M_LEVELS):
        for j, n in enumerate(M_LEVELS):
            rows.append(dict(m=m, n=n, **{f: perm[f][(a * i + b * j) % L] for f, (a, b) in zip(names[2:], mult)}))

    def missing():
        seen = set()
        for r in rows:
            for f, g in itertools.combinations(names, 2):
                seen.add((f, r[f], g, r[g]))
        return [(f, a, g, b) for f, g in itertools.combinations(names, 2) for a in lv[f] for b in lv[g] if (f, a, g, b) not in seen]
    todo = missing()
    while todo:
        r = {}
        for f, a, g, b in todo:          # as many of the missing pairs as fit into one row
            if r.get(f, a) == a and r.get(g, b) == b:
                r[f], r[g] = a, b
        for h in names:
            r.setdefault(h, lv[h][int(rng.integers(len(lv[h])))])
        rows.append(r)
        todo = missing()
    assert not missing()
    assert 150 <= len(rows) <= 260, len(rows)
    return rows


class Arena:
    """NaN-filled operand arena; blocks are separated by guard zones and only addressed elements get numbers."""

    def __init__(self, cplx, rng):
        self.cplx, self.rng, self.chunks, self.size = cplx, rng, [], GUARD

    def block(self, outer, k, layout):
        """Place an operand of `outer` rows (A) / columns (B) and k >= 1 contraction indices -> (offset, outer stride, k stride)."""
        rng = self.rng
        if layout == 'kfast':
            so, sk = k, 1
        elif layout == 'outerfast':
            so, sk = 1, outer
        elif layout == 'padded':
            if rng.integers(2):
                so, sk = k + int(rng.integers(1, 9)), 1
            else:
                so, sk = 1, outer + int(rng.integers(1, 9))
        elif layout == 'general':
            if rng.integers(2):
                sk = int(rng.integers(2, 4))
                so = sk * k + int(rng.integers(0, 3))
            else:
                so = int(rng.integers(2, 4))
                sk = so * outer + int(rng.integers(0, 3))
        else:                      # both strides 1: element (i, kk) is arena[off + i + kk] (legal: operands are only read)
            so, sk = 1, 1
        off = self.size
        idx = np.unique((np.arange(outer)[:, None] * so + np.arange(k)[None, :] * sk).reshape(-1))
        self.chunks.append((off, idx))
        self.size = off + int(idx[-1]) + 1 + GUARD
        return off, so, sk

    def build(self):
        dt = np.complex128 if self.cplx else np.float64
        arr = np.full(self.size, np.nan, dtype=dt)
        for off, idx in self.chunks:
            v = self.rng.standard_normal(len(idx))
            arr[off + idx] = v + 1j * self.rng.standard_normal(len(idx)) if self.cplx else v
        return arr


class Case:
    pass


def tile_table(tasks, bm, bn, rng, w=None):
    tiles = [[t, i, j, 0] for t, tk in enumerate(tasks) for i in range(-(-tk[1] // bm)) for j in range(-(-tk[2] // bn))]
    tiles = np.array(tiles, np.int32).reshape(-1, 4)
    if w is not None:
        tiles[:, 3] = [w(t, i) for t, i, _, _ in tiles]
    return tiles[rng.permutation(len(tiles))]


def c_arena(cplx, rng, tasks_mn_acc):
    """-> (C0, [(c_off, ldc)]): blocks with ldc > n, gaps between them; NaN where a task overwrites, random numbers elsewhere."""
    offs, size = [], int(rng.integers(1, 40))
    for m, n, acc in tasks_mn_acc:
        ldc = n + int(rng.integers(1, 8))
        offs.append((size, ldc))
        size += m * ldc + int(rng.integers(1, 40))
    C0 = rng.standard_normal(size)
    if cplx:
        C0 = C0 + 1j * rng.standard_normal(size)
    for (m, n, acc), (off, ldc) in zip(tasks_mn_acc, offs):
        if not acc:
            idx = off + np.arange(m)[:, None] * ldc + np.arange(n)[None, :]
            C0[idx] = np.nan
    return C0, offs


def make_case(cplx, cfg, rows, rng, bm, bn, sub_tasks=(0, 3), label=None):
    """One launch out of rows of factor levels (one row in the small cases).  Per row: the focus link carries (k, lay_a, lay_b,
    flags); `extra` more links of random k / layout / flags around it; an empty link (k = 0) at the stated place; a task (m, n,
    acc) over the whole chain and `sub_tasks` = [lo, hi) further tasks over the same links (sub-blocks m' <= m, n' <= n of the same
    operands, over a sub-range of the chain, with their own `accumulate`)."""
    rows = [rows] if isinstance(rows, dict) else rows
    A, B = Arena(cplx, rng), Arena(cplx, rng)
    flag_levels = factor_levels(cplx)['flags']
    links, shapes = [], []
    for row in rows:
        m, n = row['m'], row['n']

        def link(k, la, lb, fl):
            if k == 0:      # an empty link points into the leading NaN guard zones: whoever used it would bring NaN into C
                return [int(rng.integers(GUARD // 2)), int(rng.integers(GUARD // 2)), 0, 1, 1, 1, 1, fl]
            a_off, a_rs, a_ks = A.block(m, k, la)
            b_off, b_ns, b_ks = B.block(n, k, lb)
            return [a_off, b_off, k, a_rs, a_ks, b_ks, b_ns, fl]
        chain = [link(row['k'], row['lay_a'], row['lay_b'], row['flags'])]
        for _ in range(row['extra']):
            k = int(rng.choice(K_LEVELS))
            same = [p for p in chain if p[2] == k]
            if k and same and rng.integers(4) == 0:          # a link that shares its operands with an earlier one
                l = list(same[-1])
            else:
                l = link(k, str(rng.choice(LAYOUTS)), str(rng.choice(LAYOUTS)), int(rng.choice(flag_levels)))
            chain.insert(int(rng.integers(len(chain) + 1)), l)
        if row['empty'] != 'none':
            pos = {'first': 0, 'middle': max(1, len(chain) // 2), 'last': len(chain)}[row['empty']]
            chain.insert(pos, link(0, None, None, int(rng.choice(flag_levels))))
        l0, nl = len(links), len(chain)
        links += chain
        shapes.append((m, n, row['acc'], l0, nl))
        for _ in range(int(rng.integers(*sub_tasks))):
            lb = int(rng.integers(nl))
            shapes.append((int(rng.integers(1, m + 1)), int(rng.integers(1, n + 1)), int(rng.integers(2)), l0 + lb,
                           int(rng.integers(1, nl - lb + 1))))
    order = rng.permutation(len(shapes))          # the tasks of one chain are not neighbours in the task table
    shapes = [shapes[i] for i in order]
    C0, offs = c_arena(cplx, rng, [(s[0], s[1], s[2]) for s in shapes])
    c = Case()
    c.cplx, c.cfg = cplx, cfg
    c.tasks = np.array([[off, s[0], s[1], ldc, s[3], s[4], s[2], 0] for s, (off, ldc) in zip(shapes, offs)], np.int64)
    c.links = np.array(links, np.int64)
    c.tiles = tile_table(c.tasks.tolist(), bm, bn, rng)
    c.A, c.B, c.C0 = A.build(), B.build(), C0
    c.label = label or ' '.join('%s=%s' % kv for kv in rows[0].items())
    return c


def tile_shape(cplx, cfg):
    from tenpy_amd import _lib
    bm, bn = ctypes.c_int(), ctypes.c_int()
    _lib.load().tpa_gemm_tile_shape(int(cplx), cfg, ctypes.byref(bm), ctypes.byref(bn))
    return bm.value, bn.value


def small_cases(name, seeds=SEEDS):
    """The seeded cases of one instantiation: the pairwise design plus the two all-empty chains."""
    cplx, cfg, _ = INSTANTIATIONS[name]
    bm, bn = tile_shape(cplx, cfg)
    for seed in seeds:
        rng = np.random.default_rng([seed, int(cplx), cfg])
        for row in pairwise_design(cplx, seed):
            yield make_case(cplx, cfg, row, rng, bm, bn)
        for acc in (0, 1):      # all links empty: zeros over the NaN-filled C / C bit-identical
            row = dict(m=65, n=33, k=0, lay_a='kfast', lay_b='kfast', flags=0, acc=acc, extra=0, empty='last')
            yield make_case(cplx, cfg, row, rng, bm, bn)


class variant:
    """``with variant(v):`` -- the process-global tuning hook of the real kernel, restored to the environment's value afterwards
    (the hook has no getter)."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        dev.check(dev.lib().tpa_gemm_set_variant(self.v), "set_variant")

    def __exit__(self, *exc):
        dev.check(dev.lib().tpa_gemm_set_variant(int(os.environ.get('TPA_GEMM_VARIANT', 0))), "set_variant")


def run_case(c, L=None, task_pad=None):
    """Upload, launch, download -> the C arena after the launch."""
    L = L if L is not None else dev.lib()
    tasks = c.tasks if task_pad is None else task_pad
    d = [dev.to_device(x) for x in (tasks, c.links, c.tiles, c.A, c.B, c.C0)]
    dev.check(L.tpa_gemm_chain(int(c.cplx), c.cfg, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(c.tiles), d[3].data_ptr(),
                               d[4].data_ptr(), d[5].data_ptr(), dev.stream()), "gemm_chain")
    return dev.to_host(d[5])


def reference(c):
    if getattr(c, 'ref', None) is None:
        c.ref = kref.gemm_chain(c.cplx, c.tasks, c.links, c.A, c.B, c.C0)
    return c.ref


def bound(c):
    ref = reference(c)
    return (2 if c.cplx else 1) * (ref['ktot'] + 2) * EPS * ref['mag']


def check_case(c, C):
    """-> (largest error / bound of the case, or 0.0 when every bound is zero); raises AssertionError with the case's label."""
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
    nz = lim > 0
    return float(np.max(err[nz] / lim[nz])) if nz.any() else 0.0
