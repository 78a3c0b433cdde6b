"""Conformance of ``tpa_gemm_chain_ex`` (include/tenpy_amd.h: second source, scale, unit factor in ``link.flags``) on every kernel
it dispatches to: the eight-wave ``gemm_chain_kernel`` (cfg 1, <= 1024 tiles), ``gemm_chain2_kernel<64,64,2,2>`` (cfg 1, > 1024
tiles) and ``gemm_chain2_kernel<128,64,4,2>`` (cfg 0).  Arenas, reference and bound are those of ``conformance_gemm_cases`` /
``kernel_reference`` (NaN outside the addressed elements; |C - ref| <= (K_tot + 2) EPS (sum |a| |b| + |C0|), derived there): the
extended case is MATERIALISED -- second-source blocks moved into one arena, scaled blocks copied and scaled by ``tpa_lincomb_batch``
-- and the reference is taken on the materialised operands; a unit-factor link adds ``alpha a`` to the reference, its modulus to the
magnitude and one to K_tot (one more rounded addition).

Beyond the bound: a task without a unit-factor link is BIT-EQUAL to ``tpa_gemm_chain`` on the materialised case, and a launch without
any extended link is bit-equal to ``tpa_gemm_chain``.  Complex data is not built: TPA_E_BADARG.

Shapes: blocks with m, n in {1, 17, 64, 65, 130} (all 25 pairs), K in {1, 15, 16, 17, 40}, chains of 1 - 4 links mixing the four
kinds, chains of unit-factor links only, all five operand layouts of the suite (``outerfast`` = a transposed view), both values of
``accumulate``."""
import numpy as np
import pytest

import conformance_gemm_cases as cg
import kernel_reference as kref
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc

MN = (1, 17, 64, 65, 130)
KS = (1, 15, 16, 17, 40)
A2, UNIT = 4, 8
ALPHAS = np.array([1., 0., -0.5, 0., 0.7310585786300049, 0., 3.0, 0., -1.e-3, 0.])      # pairs; index 0 is never used by a link


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def xbackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_device_ex
        mock_device_ex.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


def _rows(rng, repeats):
    rows = []
    for rep in range(repeats):
        for i, m in enumerate(MN):
            for j, n in enumerate(MN):
                unit_only = (i + 2 * j + rep) % 7 == 0
                rows.append(dict(m=m, n=n, k=0 if unit_only else KS[(i + j + rep) % 5], lay_a=cg.LAYOUTS[(i + 3 * j + rep) % 5],
                                 lay_b=cg.LAYOUTS[(2 * i + j + rep) % 5], flags=0, acc=(i + j + rep) % 2,
                                 extra=0 if unit_only else (i * 5 + j + rep) % 4, empty='none'))
    return rows


def _span(m, k, rs, ks):
    return (m - 1) * rs + (k - 1) * ks + 1


def ex_case(cfg, repeats, seed, extended=True):
    """-> (c, x): the plain case ``c`` whose links have lost their K levels above 40, and the extended tables ``x`` made from it."""
    rng = np.random.default_rng(seed)
    bm, bn = cg.tile_shape(False, cfg)
    rows = _rows(rng, repeats)
    # (make_case draws the k of the extra links from its own levels: keep those of this suite)
    saved = cg.K_LEVELS
    cg.K_LEVELS = KS
    try:
        c = cg.make_case(False, cfg, rows, rng, bm, bn, sub_tasks=(0, 1))
    finally:
        cg.K_LEVELS = saved
    U = cg.Arena(False, rng)
    src_of = {}                      # a_off -> 0 / 1: a block lives in ONE of the two sources
    links, tasks = [], c.tasks.copy()
    has_unit = np.zeros(len(tasks), dtype=bool)
    kind_no = 0
    for t, tk in enumerate(c.tasks.tolist()):
        m, n = tk[1], tk[2]
        begin = len(links)
        for l in c.links[tk[4]:tk[4] + tk[5]].tolist():
            if not extended:
                links.append(l)
                continue
            if l[2] == 0:            # the placeholder of a chain of unit-factor links only
                continue
            kind = kind_no % 4       # plain, scaled, second source, second source and scaled
            kind_no += 1
            src = src_of.setdefault(l[0], 1 if kind >= 2 else 0)
            l[7] = (l[7] & 3) | (A2 if src else 0) | ((1 + (kind_no % 4) if kind in (1, 3) else 0) << 16)
            links.append(l)
        n_unit = 0 if not extended else (2 if len(links) == begin else int((t % 3) == 0))
        for u in range(n_unit):
            off, rs, cs = U.block(m, n, cg.LAYOUTS[(t + u) % 5])
            links.insert(begin + int(rng.integers(len(links) - begin + 1)),
                         [-1 - off, 0, 0, rs, cs, 0, 0, UNIT | (A2 if (t + u) % 2 else 0) | (((t + u) % 5) << 16)])
            has_unit[t] = True
        tasks[t, 4], tasks[t, 5] = begin, len(links) - begin
    Ua = U.build()
    links = np.array(links, dtype=np.int64).reshape(-1, 8)
    unit = links[:, 0] < 0
    # the two sources: every block in one of them, NaN in the other; unit blocks behind the operands of their source
    A1, A2a = c.A.copy(), np.full(len(c.A), np.nan)
    moved = []
    for tk in tasks.tolist():
        for l in links[tk[4]:tk[4] + tk[5]].tolist():
            if l[0] >= 0 and (l[7] & A2):
                moved.append(l[0] + np.arange(tk[1])[:, None] * l[3] + np.arange(l[2])[None, :] * l[4])
    for idx in moved:
        A2a[idx] = c.A[idx]
    for idx in moved:
        A1[idx] = np.nan
    base = len(c.A)
    A1 = np.concatenate([A1, Ua])
    A2a = np.concatenate([A2a, Ua.copy()])
    for r in np.nonzero(unit)[0]:
        off = -1 - links[r, 0]
        links[r, 0] = base + off
        m, n = [(tk[1], tk[2]) for tk in tasks.tolist() if tk[4] <= r < tk[4] + tk[5]][0]
        idx = base + off + np.arange(m)[:, None] * links[r, 3] + np.arange(n)[None, :] * links[r, 4]
        (A1 if links[r, 7] & A2 else A2a)[idx] = np.nan
    x = cg.Case()
    x.tasks, x.links, x.tiles, x.A, x.A2, x.B, x.C0, x.cfg, x.has_unit = tasks, links, c.tiles, A1, A2a, c.B, c.C0, cfg, has_unit
    x.label = 'ex cfg=%d tasks=%d tiles=%d' % (cfg, len(tasks), len(c.tiles))
    return c, x


def run_ex(x):
    d = [dev.to_device(a) for a in (x.tasks, x.links, x.tiles, x.A, x.A2, x.B, x.C0, ALPHAS)]
    dev.check(dev.lib().tpa_gemm_chain_ex(0, x.cfg, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(x.tiles), d[3].data_ptr(),
                                          d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), dev.stream()), "gemm_chain_ex")
    return dev.to_host(d[6])


def materialise(x):
    """The plain case that the extended one stands for: one arena [A | A2 | scaled copies], the copies made by ``tpa_lincomb_batch``
    on the device; unit-factor links stay in the table as the empty links they are for ``tpa_gemm_chain``."""
    links = x.links.copy()
    nA = len(x.A)
    jobs, terms, extra = [], [], 0
    for t, tk in enumerate(x.tasks.tolist()):
        for r in range(tk[4], tk[4] + tk[5]):
            l = links[r]
            if l[7] & UNIT:
                links[r, 7] = 0
                continue
            src = l[0] + (nA if l[7] & A2 else 0)
            ia = (l[7] >> 16) & 0xffff
            if ia:
                sp = _span(tk[1], l[2], l[3], l[4])
                jobs.append([2 * nA + extra, 1, sp, sp, len(terms), 1, 0, 0])
                terms.append([src, sp, np.array(ALPHAS[2 * ia]).view(np.int64), 0])
                src = 2 * nA + extra
                extra += sp
            links[r, 0], links[r, 7] = src, 0
    arena = dev.to_device(np.concatenate([x.A, x.A2, np.zeros(extra)]))
    if jobs:
        jobs, terms = np.array(jobs, dtype=np.int64), np.array(terms, dtype=np.int64)
        jd, td = dev.to_device(jobs), dev.to_device(terms)
        dev.check(dev.lib().tpa_lincomb_batch(0, jd.data_ptr(), len(jobs), td.data_ptr(), int(jobs[:, 2].max()), arena.data_ptr(),
                                              arena.data_ptr(), dev.stream()), "lincomb")
    p = cg.Case()
    p.cplx, p.cfg, p.tasks, p.links, p.tiles, p.A, p.B, p.C0, p.label = False, x.cfg, x.tasks, links, x.tiles, dev.to_host(arena), x.B, x.C0, x.label
    return p


def reference_ex(x, p):
    """``kernel_reference.gemm_chain`` on the materialised case plus the unit-factor links."""
    ref = kref.gemm_chain(False, p.tasks, p.links, p.A, p.B, p.C0)
    LD = kref.LD
    for tk in x.tasks.tolist():
        ic = (tk[0] + np.arange(tk[1])[:, None] * tk[3] + np.arange(tk[2])[None, :]).reshape(-1)
        for l in x.links[tk[4]:tk[4] + tk[5]].tolist():
            if l[7] & UNIT:
                src = x.A2 if l[7] & A2 else x.A
                ia = (l[7] >> 16) & 0xffff
                al = ALPHAS[2 * ia] if ia else 1.0
                a = src[l[0] + np.arange(tk[1])[:, None] * l[3] + np.arange(tk[2])[None, :] * l[4]].reshape(-1)
                ref['re'][ic] += LD(al) * a.astype(LD)
                ref['mag'][ic] += np.abs(LD(al) * a.astype(LD))
                ref['ktot'][ic] += 1
    p.ref = ref
    return ref


CASES = {'chain_64x64x1x2_ex_cfg1': (1, 1), 'chain2_64x64x2x2_ex_cfg1_over1024tiles': (1, 18), 'chain2_128x64x4x2_ex_cfg0': (0, 1)}


@pytest.mark.parametrize("name", list(CASES))
def test_gemm_chain_ex(xbackend, name):
    cfg, repeats = CASES[name]
    if xbackend == 'mock' and repeats > 1:
        repeats = 2                     # (the emulation has one code path: the tile count selects nothing there)
    _, x = ex_case(cfg, repeats, [cg.SEEDS[0], cfg, repeats])
    if xbackend == 'gpu':
        assert (len(x.tiles) > 1024) == ('over1024' in name), len(x.tiles)
    flags = x.links[:, 7]
    assert np.any(flags & UNIT) and np.any((flags & A2) != 0) and np.any((flags >> 16) != 0) and np.any((flags & ~3) == 0)
    unit_only = [tk for tk in x.tasks.tolist() if all(l[7] & UNIT for l in x.links[tk[4]:tk[4] + tk[5]].tolist())]
    assert unit_only and any(tk[1] % 64 and tk[2] % 64 for tk in unit_only)
    with cg.variant(0):
        C = run_ex(x)
        p = materialise(x)
        C_plain = cg.run_case(p)
    reference_ex(x, p)
    worst = cg.check_case(p, C)
    print("%s: %d tasks, %d links, %d tiles, worst err / bound = %.3g" % (name, len(x.tasks), len(x.links), len(x.tiles), worst))
    assert worst <= 1.0
    # tasks without a unit-factor link: the bits of tpa_gemm_chain on the block that tpa_lincomb_batch scaled (on the device: the
    # emulation multiplies with numpy, whose summation order follows the memory layout of the operand)
    if xbackend != 'gpu':
        return
    n_cmp = 0
    for tk, hu in zip(x.tasks.tolist(), x.has_unit):
        if not hu:
            ic = tk[0] + np.arange(tk[1])[:, None] * tk[3] + np.arange(tk[2])[None, :]
            assert np.array_equal(kref.bits(C[ic]), kref.bits(C_plain[ic])), "scaled / second-source links are not bit-equal: m=%d n=%d" % (tk[1], tk[2])
            n_cmp += 1
    assert n_cmp >= 10


@pytest.mark.parametrize("name", list(CASES))
def test_no_extended_link_is_bit_equal(xbackend, name):
    cfg, repeats = CASES[name]
    if xbackend == 'mock' and repeats > 1:
        repeats = 2
    c, x = ex_case(cfg, repeats, [cg.SEEDS[0], cfg, repeats, 1], extended=False)
    assert not np.any(x.links[:, 7] & ~3) and len(x.links) == len(c.links)      # (the same chains, stored in the order of the tasks)
    with cg.variant(0):
        C, C_plain = run_ex(x), cg.run_case(c)
    assert np.array_equal(kref.bits(C), kref.bits(C_plain))
    assert cg.check_case(c, C) <= 1.0


@pytest.mark.gpu
def test_complex_is_not_built():
    from tenpy_amd import _lib
    _lib.require_gpu()
    _, x = ex_case(1, 1, [cg.SEEDS[0], 7])
    d = [dev.to_device(a) for a in (x.tasks, x.links, x.tiles, x.A, x.A2, x.B, x.C0, ALPHAS)]
    with pytest.raises(ValueError):
        dev.check(dev.lib().tpa_gemm_chain_ex(1, 1, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(x.tiles), d[3].data_ptr(),
                                              d[4].data_ptr(), d[5].data_ptr(), d[6].data_ptr(), d[7].data_ptr(), dev.stream()), "gemm_chain_ex")
