"""``MpoZipupPlan`` / ``device_zipup_step`` (the matrix of an interior step of the zip-up MPO application: one GEMM over chi and the MPO
step, cell-dense or entry by entry) against what the reference's ``MPO.apply_zipup`` handed to ``svd_theta`` inside its own pass
(tests/golden/mpo_apply.pkl, record ``percall``; generator tests/golden/make_golden_mpo_apply.py), on the emulation and on the GPU.

Bounds: ``M`` element-wise within 1e-13 max|M| of the stored dense ``M`` (the level of the other per-call fixtures: an element is a
sum of at most chi D d <= 16 * 4 * 3 products, gamma_192 = 2e-14 times the magnitude sum); all singular values of ``M`` within
1e-12 sigma_max, the project's SVD tolerance.  The routes (``TPA_MPO_CELL`` = 0, 2 and the rule) sum the same chains
of fused multiply-adds: their results compare ``==``."""
import os
import pickle

import numpy as np
import pytest

from mpo_cell_fixtures import blocked_array, cbackend  # noqa: F401
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks.mpo import mpo_from_dense

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mpo_apply.pkl'), 'rb') as _f:
    CALLS = pickle.load(_f)['percall']
IDS = ['%s-i%d' % (c['name'], c['i']) for c in CALLS]


def _operands(c):
    chinfo = ChargeInfo([int(m) for m in c['chinfo_mod']])
    return tuple(blocked_array(c[k], chinfo, c[k]['data'].dtype) for k in ('VH_prev', 'B', 'W'))


def _step(monkeypatch, c, mode):
    if mode is None:
        monkeypatch.delenv('TPA_MPO_CELL', raising=False)
    else:
        monkeypatch.setenv('TPA_MPO_CELL', str(mode))
    mps_common.reset_zipup_stats()
    M = mps_common.device_zipup_step(*_operands(c))
    assert M is not None, "the device route declined: %r" % (mps_common.zipup_stats['why'],)
    return M, dict(mps_common.zipup_stats)


def test_fixture_is_what_the_generator_promises():
    assert {c['name'] for c in CALLS} == {'xxz', 'spin1', 'tfi'}
    by = {n: [c for c in CALLS if c['name'] == n] for n in ('xxz', 'spin1', 'tfi')}
    assert all(len(v) >= 2 for v in by.values())
    assert all(np.iscomplexobj(c['W']['data']) for c in by['xxz']) and not any(np.iscomplexobj(c['W']['data']) for c in by['spin1'])
    assert all(len(c['chinfo_mod']) == 0 for c in by['tfi']) and all(len(c['chinfo_mod']) == 1 for c in by['xxz'] + by['spin1'])
    # spin-1: the MPO bond legs carry a charge block wider than 1; TFI: every virtual leg is one block
    assert all(max(np.diff(c['W']['slices'][a])) > 1 for c in by['spin1'] for a in (0, 1))
    assert all(len(c[k]['slices'][a]) == 2 for c in by['tfi'] for k, a in (('VH_prev', 0), ('VH_prev', 2), ('B', 0), ('B', 2)))
    for c in CALLS:
        assert c['M'].shape == (c['VH_prev']['data'].shape[0], c['B']['data'].shape[1], c['W']['data'].shape[1], c['B']['data'].shape[2])
        assert 0 < len(c['S_all']) <= min(c['M'].shape[0] * c['M'].shape[1], c['M'].shape[2] * c['M'].shape[3])      # (block-wise SVD)


def test_fixture_plans_have_real_cells(cbackend):
    """The legs are rebuilt block for block: the spin-1 and TFI calls have cells of more than one row whose rows are shared by more than
    one column item in either direction (n_rows, pre, post > 1 in one job); the rows of a spin-1 cell share source rows (nnz > n_src)."""
    seen = set()
    for c in CALLS:
        VH_prev, B, W = _operands(c)
        plan = mps_common.MpoZipupPlan.get(npc.tensordot(VH_prev, B, axes=['vR', 'vL']), W)
        j = plan.jobs_host
        assert plan.ordered
        if c['name'] == 'xxz':
            continue
        assert int(np.max(j[:, 2])) > 1 and int(np.max(j[:, 3])) > 1
        if c['name'] == 'spin1':       # (the two rows of a TFI cell read different sources: sigma_x and 1 do not overlap)
            assert bool(np.any(plan.cell_nnz > plan.cell_n_src))
        if np.any((j[:, 2] > 1) & (j[:, 1] > 1) & (j[:, 3] > 1)):
            seen.add(c['name'])
        if c['name'] == 'tfi':
            assert len(j) == 2 and np.all(j[:, 1] * j[:, 3] == c['M'].shape[0] * c['M'].shape[3]), "no charge: one dense cell per MPO bond block"
    assert seen == {'spin1', 'tfi'}


@pytest.mark.parametrize("n", range(len(CALLS)), ids=IDS)
def test_step_against_the_reference(cbackend, monkeypatch, n):
    """Every per-call fixture under TPA_MPO_CELL = 0, 1, 2 and the default: M, its singular values, its labels and pipes; the cell route
    is counted under 2; all settings give equal results."""
    c = CALLS[n]
    want = c['M']
    res = {}
    for mode in (0, 1, 2, None):
        M, st = _step(monkeypatch, c, mode)
        assert st['device_steps'] == 1 and st['declined'] == 0
        assert st['cell_launches'] + st['entry_launches'] in (1, 2)
        if mode == 0:
            assert st['cell_launches'] == 0 and st['entry_launches'] == 1
        if mode == 2:
            assert st['cell_launches'] == 1, "TPA_MPO_CELL=2 sends every cell with a source to the cell-dense launch"
        assert M.get_leg_labels() == ['(vL.p)', '(wR.vR)']
        VH_prev, B, W = _operands(c)
        ref = npc.tensordot(npc.tensordot(VH_prev, B, axes=['vR', 'vL']), W, axes=(['wR', 'p'], ['wL', 'p*']))
        ref = ref.combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1])
        for a in (0, 1):      # the pipes combine_legs builds: the reference's split_legs works on U and VH
            M.legs[a].test_equal(ref.legs[a])
        dense = M.split_legs().transpose(['vL', 'p', 'wR', 'vR']).to_ndarray()
        assert dense.shape == want.shape and M.dtype == np.result_type(c['B']['data'].dtype, c['W']['data'].dtype)
        err = float(np.abs(dense - want).max())
        S_all = np.sort(np.asarray(npc.svd(M, compute_uv=False)))[::-1]
        assert len(S_all) == len(c['S_all'])
        d_S = float(np.abs(S_all - c['S_all']).max())
        print("ZIPUP_GOLDEN %s mode=%s M %s max err %.3g (bound %.3g), singular values max err %.3g (bound %.3g), launches cell=%d entry=%d"
              % (IDS[n], mode, dense.shape, err, 1e-13 * np.abs(want).max(), d_S, 1e-12 * c['S_all'][0],
                 st['cell_launches'], st['entry_launches']))
        assert err <= 1e-13 * np.abs(want).max()
        assert d_S <= 1e-12 * c['S_all'][0]
        res[mode] = dense
    assert np.array_equal(res[0], res[2]), "the cell-dense route and the entry route differ"
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[None])


def _leg(chinfo, q, widths, qconj):
    """A leg with one charge block of ``widths[k]`` indices per entry of ``q`` (neither sorted nor bunched)."""
    return LegCharge.from_qind(chinfo, np.concatenate([[0], np.cumsum(widths)]), np.asarray(q).reshape(-1, 1), qconj=qconj)


def _wide_case(cplx, D=84, side=False):
    """A synthetic Sz-conserving site with one block of ``D`` bond indices of charge 0: an MPO tensor built by ``mpo_from_dense`` from a
    seeded generator, dense on that block up to 20 % zeros (a cell of the fused matrix then has 1 x D rows); ``side``: two more bond
    indices of charge +2 and -2, coupled to the block through S+ and S- (cells of one row next to the wide ones).  Random VH_prev and B
    on virtual legs with blocks of 1 to 4 indices (pre, post > 1)."""
    rng = np.random.default_rng([11, int(cplx), D, int(side)])
    chinfo = ChargeInfo([1])
    p = LegCharge.from_qflat(chinfo, [[1], [-1]], qconj=+1)
    Dt = D + 2 * side
    Wd = np.zeros((Dt, Dt, 2, 2), dtype=np.complex128 if cplx else np.float64)
    Wd[:D, :D, 0, 0] = rng.standard_normal((D, D))
    Wd[:D, :D, 1, 1] = rng.standard_normal((D, D))
    if cplx:
        Wd[:D, :D, 0, 0] += 1j * rng.standard_normal((D, D))
    Wd[rng.random(Wd.shape) < 0.2] = 0
    Wd[0, 0, 0, 0] = Wd[D - 1, D - 1, 0, 0] = 1.
    if side:
        Wd[:D, D, 0, 1], Wd[D, :D, 1, 0] = rng.standard_normal(D), rng.standard_normal(D)
        Wd[:D, D + 1, 1, 0], Wd[D + 1, :D, 0, 1] = rng.standard_normal(D), rng.standard_normal(D)
    W = mpo_from_dense([Wd], [p], chinfo, dtype=Wd.dtype, IdR=D - 1).get_W(0)
    _, W = W.sort_legcharge(sort=False, bunch=[True, True, False, False])       # one block of D indices on either bond leg
    wL = W.get_leg('wL')
    assert wL.block_number == 1 + 2 * side and int(wL.get_block_sizes()[0]) == D
    vL = _leg(chinfo, [0, 2, 2, -2, 0], [2, 3, 1, 2, 2], +1)
    vM = _leg(chinfo, [0, 2, 0, -2, 0, 2], [3, 1, 2, 2, 1, 4], +1)
    vR = _leg(chinfo, [q + s for q in (0, 2, -2) for s in (1, -1)], [2, 3, 1, 4, 2, 3], -1)

    def rand(legs, labels):
        A = npc.Array.from_func(rng.standard_normal, legs, dtype=np.float64, labels=labels)
        return A.astype(np.complex128) if cplx else A
    return rand([vL, wL.conj(), vM.conj()], ['vL', 'wR', 'vR']), rand([vM, p, vR], ['vL', 'p', 'vR']), W


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_cell_wider_than_32_rows(cbackend, monkeypatch, cplx):
    """Cells of 84 rows: split into jobs of 32, 32 and 20 rows over one source list; against the generic contraction, and equal to
    the entry route."""
    VH_prev, B, W = _wide_case(cplx)
    ref = npc.tensordot(npc.tensordot(VH_prev, B, axes=['vR', 'vL']), W, axes=(['wR', 'p'], ['wL', 'p*']))
    ref = ref.combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1]).to_ndarray()
    res = {}
    for mode in (0, 2):
        monkeypatch.setenv('TPA_MPO_CELL', str(mode))
        mps_common.reset_zipup_stats()
        M = mps_common.device_zipup_step(VH_prev, B, W)
        assert M is not None and mps_common.zipup_stats['cell_launches'] == (1 if mode == 2 else 0)
        res[mode] = M.to_ndarray()
        # 84 sources of magnitude <= 5 each times a GEMM over 6: far below 1e-12 max|M|
        assert np.abs(res[mode] - ref).max() <= 1e-12 * np.abs(ref).max()
    plan = mps_common.MpoZipupPlan.get(npc.tensordot(VH_prev, B, axes=['vR', 'vL']), W)
    assert plan.ordered and int(np.max(plan.jobs_host[:, 2])) > 32
    assert len(plan.cell_jobs_host) > len(plan.jobs_host) and int(np.max(plan.cell_jobs_host[:, 2])) == 32
    split = plan.cell_jobs_host[plan.piece_job == int(np.argmax(plan.jobs_host[:, 2]))]
    assert len(split) >= 2 and len(set(split[:, 6])) == 1 and len(set(split[:, 8])) == len(split)      # one source list, own coefficients
    assert np.array_equal(res[0], res[2])


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
def test_rule_splits_one_step_into_both_launches(cbackend, monkeypatch, cplx):
    """TPA_MPO_CELL=1 on a site with cells of 12 rows over 12 or 13 shared sources (the rule sends them to the cell-dense launch) next
    to cells of one row and cells without a source (they stay with the entry launch, from a table of their own): two launches into
    one arena, counted, the result ``==`` to the entry route alone and to the forced cell route, and right."""
    VH_prev, B, W = _wide_case(cplx, D=12, side=True)
    T1 = npc.tensordot(VH_prev, B, axes=['vR', 'vL'])
    ref = npc.tensordot(T1, W, axes=(['wR', 'p'], ['wL', 'p*'])).combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1]).to_ndarray()
    plan = mps_common.MpoZipupPlan.get(T1, W)
    rule = plan._cell_rule(plan.cell_n_src, plan.jobs_host[:, 2], plan.cell_nnz)
    assert 0 < int(rule.sum()) < len(rule) and np.all(plan.jobs_host[rule, 2] == 12) and np.all(plan.jobs_host[~rule, 2] == 1)
    assert bool(np.any(plan.cell_n_src[~rule] == 0)) and bool(np.any(plan.cell_n_src[~rule] > 0))
    r = plan.route(1)
    assert r.n_cell == int(rule.sum()) and r.n_entry == int((~rule).sum()) and r.max_rows == 12
    res = {}
    for mode in (0, 1, 2):
        monkeypatch.setenv('TPA_MPO_CELL', str(mode))
        mps_common.reset_zipup_stats()
        M = mps_common.device_zipup_step(VH_prev, B, W)
        st = mps_common.zipup_stats
        assert M is not None and st['device_steps'] == 1
        # mode 2 leaves the cells without a source to the entry launch, which writes their zeros
        assert (st['cell_launches'], st['entry_launches']) == {0: (0, 1), 1: (1, 1), 2: (1, 1)}[mode]
        res[mode] = M.to_ndarray()
        # at most 13 sources of magnitude <= 5 each times a GEMM over 13: far below 1e-12 max|M|
        assert np.abs(res[mode] - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])


def test_declines(cbackend, monkeypatch):
    """``explicit_plus_hc``, an infinite chain, the switch and a forced job limit (``MAX_JOBS`` of the new class only): counted with their
    reasons, ``None`` returned; the plan of the subspace expansion keeps its limit."""
    c = CALLS[1]
    monkeypatch.setenv('TPA_MPO_CELL', '2')
    mps_common.reset_zipup_stats()
    assert mps_common.device_zipup_step(*_operands(c), explicit_plus_hc=True) is None
    assert mps_common.device_zipup_step(*_operands(c), finite=False) is None
    assert mps_common.device_zipup_step(None, None, None, finite=False) is None       # (decided before the operands are looked at)
    monkeypatch.setenv('TPA_ZIPUP_DEVICE', '0')
    assert mps_common.device_zipup_step(*_operands(c)) is None
    monkeypatch.delenv('TPA_ZIPUP_DEVICE')
    monkeypatch.setattr(mps_common.MpoZipupPlan, 'MAX_JOBS', 1)
    assert mps_common.MpoExpandPlan.MAX_JOBS == 60000
    npc.clear_device_caches()
    assert mps_common.device_zipup_step(*_operands(c)) is None
    st = mps_common.zipup_stats
    assert st['why'] == {'explicit_plus_hc': 1, 'not finite': 2, 'switched off': 1, 'too many jobs': 1} and st['declined'] == 5 and st['device_steps'] == 0
    monkeypatch.setattr(mps_common.MpoZipupPlan, 'MAX_JOBS', 60000)
    npc.clear_device_caches()
    assert mps_common.device_zipup_step(*_operands(c)) is not None
