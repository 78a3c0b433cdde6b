"""Conformance of ``tpa_gemm_chain`` -- every instantiation of the dispatch at the end of csrc/tpa_gemm.hip -- with the extended-precision
statement of the header (tests/kernel_reference.py), on the numpy emulation (``mock``, CPU) and on the HIP kernels (``gpu``).

Cases, canaries and the derivation of the tolerance: tests/conformance_gemm_cases.py.  The instantiation is part of every test id:

    chain2_128x64x4x2_real_cfg0            gemm_chain2_kernel<128,64,4,2>          real data, cfg 0
    chain_64x64x1x2_real_cfg1              gemm_chain_kernel<false,64,64,1,2,16>   real data, cfg 1, <= 1024 tiles
    chain2_64x64x2x2_real_cfg1_variant     gemm_chain2_kernel<64,64,2,2>           real data, cfg 1, tpa_gemm_set_variant(1)
    chain2_64x64x2x2_real_cfg1_over1024*   gemm_chain2_kernel<64,64,2,2>           real data, cfg 1, > 1024 tiles (the production route)
    chain_64x32x2x1_complex_cfg1           gemm_chain_kernel<true,64,32,2,1,16>    complex data, cfg 1
    chain_128x64x4x2_complex_cfg0          gemm_chain_kernel<true,128,64,4,2,16>   complex data, cfg 0
"""
import numpy as np
import pytest

import conformance_gemm_cases as cg
import kernel_reference as kref
from tenpy_amd.linalg import _device as dev

INST = list(cg.INSTANTIATIONS)


def _report(what, inst, n_cases, ratio):
    print("CONFORMANCE %s %s cases=%d max_err_over_bound=%.4f" % (what, inst, n_cases, ratio))


@pytest.mark.parametrize("inst", INST)
def test_gemm_small_cases(backend, inst):
    """The pairwise design over (m, n, k, layout of A, layout of B, flags, accumulate, chain length, place of an empty link) plus the
    two all-empty chains.  Real data: flags 3 (the conjugation bits are "complex only") must give the flags-0 result bit for bit."""
    cplx, cfg, var = cg.INSTANTIATIONS[inst]
    worst, count = 0.0, 0
    with cg.variant(var):
        for c in cg.small_cases(inst):
            C = cg.run_case(c)
            worst = max(worst, cg.check_case(c, C))
            count += 1
            if not cplx and c.links[:, 7].any():
                plain = cg.Case()
                plain.__dict__.update(c.__dict__)
                plain.links = c.links.copy()
                plain.links[:, 7] = 0
                assert np.array_equal(kref.bits(cg.run_case(plain)), kref.bits(C)), "flags change a real product: " + c.label
    assert 150 <= count <= 260
    assert worst <= 1.0
    _report("tpa_gemm_chain", inst, count, worst)


def _many_rows(rng, n_groups):
    lv = cg.factor_levels(False)
    small = dict(lv, m=(1, 15, 16, 17, 31, 33, 63, 64, 65, 129), n=(1, 15, 16, 17, 31, 33, 63, 64, 65, 129), extra=(0, 1, 3),
                 k=(0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33))
    return [{f: small[f][int(rng.integers(len(small[f])))] for f in small} for _ in range(n_groups)]


def test_gemm_chain2_64x64x2x2_real_cfg1_over1024tiles_many_tasks(backend):
    """Route (a) to gemm_chain2_kernel<64,64,2,2>, as in production: ONE launch of more than 1024 tiles at cfg 1 -- about 1100 small
    tasks of mixed shapes in 280 chains that share their links and operands."""
    rng = np.random.default_rng(cg.SEEDS[0] + 1)
    bm, bn = cg.tile_shape(False, 1)
    c = cg.make_case(False, 1, _many_rows(rng, 280), rng, bm, bn, sub_tasks=(2, 5), label='many tasks')
    assert len(c.tiles) > 1024 and 1000 <= len(c.tasks) <= 1400, (len(c.tiles), len(c.tasks))
    with cg.variant(0):
        worst = cg.check_case(c, cg.run_case(c))
    assert worst <= 1.0
    _report("tpa_gemm_chain", "chain2_64x64x2x2_real_cfg1_over1024tiles_many_tasks(tasks=%d,tiles=%d)" % (len(c.tasks), len(c.tiles)), 1, worst)


def test_gemm_chain2_64x64x2x2_real_cfg1_over1024tiles_one_block(backend):
    """Route (a) with ONE C block of 33 x 33 tiles (2049 x 2053: a partial last tile row and column), chain 16 + 0 + 5."""
    rng = np.random.default_rng(cg.SEEDS[0] + 2)
    bm, bn = cg.tile_shape(False, 1)
    row = dict(m=2049, n=2053, k=16, lay_a='padded', lay_b='outerfast', flags=0, acc=1, extra=0, empty='last')
    c = cg.make_case(False, 1, row, rng, bm, bn, sub_tasks=(0, 1))
    # a second non-empty link behind the empty one (k = 5: a partial k-tile at the end of the chain)
    extra = cg.make_case(False, 1, dict(row, k=5, lay_a='outerfast', lay_b='kfast', empty='none'), rng, bm, bn, sub_tasks=(0, 1))
    lk = extra.links[0].copy()
    lk[0] += len(c.A)
    lk[1] += len(c.B)
    c.A, c.B = np.concatenate([c.A, extra.A]), np.concatenate([c.B, extra.B])
    c.links = np.concatenate([c.links, lk[None, :]])
    c.tasks[0, 5] = len(c.links)
    assert len(c.tiles) == 33 * 33 > 1024 and c.links[:, 2].tolist() == [16, 0, 5]
    with cg.variant(0):
        worst = cg.check_case(c, cg.run_case(c))
    assert worst <= 1.0
    _report("tpa_gemm_chain", "chain2_64x64x2x2_real_cfg1_over1024tiles_one_block(tiles=%d)" % len(c.tiles), 1, worst)


# ---- identity-row skip ------------------------------------------------------------------------------------------------------

def _identity_case(cplx, cfg, rng, bm, bn, m, n, lay_a, lay_b):
    """Task 0: C = Q B with Q m x m; the rows of Q that the tile rows `ident` need are unit vectors e_row.  Its tiles carry
    tile.w = 1 + (tile row + 2), except one ordinary tile row with tile.w = 0.  Task 1: an ordinary product whose tiles carry a
    tile.w > 0 but whose task[7] is 0.  -> (case, tile rows with unit vectors, tile rows without a word)"""
    rows = [dict(m=m, n=n, k=m, lay_a=lay_a, lay_b=lay_b, flags=0, acc=0, extra=0, empty='last'),
            dict(m=65, n=33, k=17, lay_a='kfast', lay_b='kfast', flags=0, acc=0, extra=1, empty='none')]
    c = cg.make_case(cplx, cfg, rows, rng, bm, bn, sub_tasks=(0, 1), label='identity rows m=%d n=%d %s %s' % (m, n, lay_a, lay_b))
    t0 = int(np.flatnonzero((c.tasks[:, 1] == m) & (c.links[c.tasks[:, 4], 2] == m))[0])
    lk = c.links[c.tasks[t0, 4]]
    assert lk[2] == m
    T = -(-m // bm)
    ident = [i for i in range(T) if i % 2 == (T - 1) % 2]          # the last tile row (partial unless bm | m), every second one before it
    no_word = [i for i in range(T) if i not in ident][:1]
    for i in ident:
        for r in range(i * bm, min(m, (i + 1) * bm)):
            c.A[lk[0] + r * lk[3] + np.arange(m) * lk[4]] = 0
            c.A[lk[0] + r * lk[3] + r * lk[4]] = 1
    for tl in c.tiles:
        tl[3] = (0 if tl[1] in no_word else 1 + tl[1] + 2) if tl[0] == t0 else 5
    return c, t0, ident


@pytest.mark.parametrize("inst", INST)
def test_gemm_identity_rows(backend, inst):
    """The identity-row skip (include/tenpy_amd.h, "identity-row skip"): where the word of a tile is 0 -- and the rows of A it needs
    really are unit vectors -- the tile of C is a copy of the first link's B rows, bit for bit; and because a product with exact zeros
    and ones is exact, the same launch with that word non-zero gives the same bits."""
    cplx, cfg, var = cg.INSTANTIATIONS[inst]
    bm, bn = cg.tile_shape(cplx, cfg)
    rng = np.random.default_rng([cg.SEEDS[0], 3, int(cplx), cfg])
    worst, count = 0.0, 0
    with cg.variant(var):
        for m, n, lay_a, lay_b in [(65, 33, 'kfast', 'outerfast'), (193, 129, 'outerfast', 'kfast'), (300, 70, 'padded', 'padded'),
                                   (128, 64, 'kfast', 'general'), (17, 1, 'kfast', 'outerfast')]:
            c, t0, ident = _identity_case(cplx, cfg, rng, bm, bn, m, n, lay_a, lay_b)
            T = -(-m // bm)
            words = np.full(T + 3, 7, np.int32)
            words[[i + 2 for i in ident]] = 0
            outs = []
            for w in (words, np.full(T + 3, 7, np.int32)):
                w_dev = dev.to_device(w)
                tasks = c.tasks.copy()
                tasks[t0, 7] = w_dev.data_ptr()
                outs.append(cg.run_case(c, task_pad=tasks))
                del w_dev
            worst = max(worst, cg.check_case(c, outs[0]), cg.check_case(c, outs[1]))
            assert np.array_equal(kref.bits(outs[0]), kref.bits(outs[1])), c.label
            c_off, _, _, ldc = c.tasks[t0, :4]
            lk = c.links[c.tasks[t0, 4]]
            for i in ident:
                for r in range(i * bm, min(m, (i + 1) * bm)):
                    want = c.B[lk[1] + r * lk[5] + np.arange(n) * lk[6]]
                    assert np.array_equal(kref.bits(outs[0][c_off + r * ldc:c_off + r * ldc + n]), kref.bits(want)), (c.label, r)
            count += 1
    assert worst <= 1.0
    _report("tpa_gemm_chain/identity_rows", inst, count, worst)


# ---- row strides beyond 2^31 elements: the complex and cfg 1 siblings of test_kernels_gpu.py::test_gemm_row_stride_beyond_2_31_elements ----

@pytest.mark.gpu
@pytest.mark.parametrize("inst", ['chain_64x32x2x1_complex_cfg1', 'chain_128x64x4x2_complex_cfg0', 'chain2_64x64x2x2_real_cfg1_variant'])
def test_gemm_row_stride_beyond_2_31_elements(inst):
    """Rows 2^29 elements apart (row 4 starts 2^31 elements into the operand): complex data on both tile configurations, and real
    data on the round-6 loop at cfg 1.  Same free-memory guard as the real test."""
    import torch
    from tenpy_amd import _lib
    _lib.require_gpu()
    cplx, cfg, var = cg.INSTANTIATIONS[inst]
    free, _ = torch.cuda.mem_get_info()
    if free < 40 * (1 << 30):
        pytest.skip("needs 22 GB (real) / 35 GB (complex) of device memory")
    m, n, k, rs = 5, 70, 100, 1 << 29
    rng = np.random.default_rng(5)
    dt = np.complex128 if cplx else np.float64
    rows = rng.standard_normal((m, k)) + (1j * rng.standard_normal((m, k)) if cplx else 0)
    Bh = rng.standard_normal((k, n)) + (1j * rng.standard_normal((k, n)) if cplx else 0)
    A = torch.empty((m - 1) * rs + k, dtype=dev.tdtype(dt), device='cuda')
    rows_d = torch.from_numpy(rows.astype(dt)).cuda()
    for i in range(m):
        A[i * rs:i * rs + k] = rows_d[i]
    c = cg.Case()
    c.cplx, c.cfg, c.label = cplx, cfg, inst
    c.tasks = np.array([[0, m, n, n + 3, 0, 1, 0, 0]], np.int64)
    c.links = np.array([[0, 0, k, rs, 1, n, 1, 2 if cplx else 0]], np.int64)
    c.tiles = cg.tile_table(c.tasks.tolist(), *cg.tile_shape(cplx, cfg), rng)
    c.C0 = np.full(m * (n + 3), np.nan, dtype=dt)
    c.C0[(np.arange(m)[:, None] * (n + 3) + n + np.arange(3)[None, :]).reshape(-1)] = 1.5
    d = [dev.to_device(x) for x in (c.tasks, c.links, c.tiles, Bh.reshape(-1).astype(dt), c.C0)]
    with cg.variant(var):
        dev.check(dev.lib().tpa_gemm_chain(int(cplx), cfg, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(c.tiles), A.data_ptr(),
                                           d[3].data_ptr(), d[4].data_ptr(), dev.stream()), "gemm_chain")
        C = dev.to_host(d[4])
    del A
    # the reference on the compact operand: the same rows with row stride k
    c.links[0, 3] = k
    c.A, c.B = rows.reshape(-1).astype(dt), Bh.reshape(-1).astype(dt)
    worst = cg.check_case(c, C)
    assert worst <= 1.0
    _report("tpa_gemm_chain/row_stride_2^31", inst, 1, worst)
