"""What the three plans of the MPO step share through ``mps_common._MpoStepPlan`` -- the cached constructor with its ``id()`` keys --
and the one builder of the plan chain of the factored effective Hamiltonians, ``mps_common._factored_plans``.  Host logic only: every
test runs on the numpy emulation.  Inputs: the XXZ chain with L = 6 (``MpoApplyPlan``), the Hubbard ladder with an N-only physical leg
at chi <= 16 (``MpoBlockApplyPlan``) and ``xxz_sorted`` of ``mpo_entry_fixtures`` (``MpoEntryApplyPlan``); X is ``LP . theta`` of a
one-site vector on a bulk site.  The emulation is installed by a fixture of this file: the ``mock`` parameter of the ``backend``
fixture installs ``mock_device`` alone, which has neither ``tpa_mpo_apply_batch`` nor ``tpa_mpo_entry_apply_batch``, and without them
``_mpo_plan_class`` routes no MPO to the block and entry plans."""
import numpy as np
import pytest

import mock_mpo_entry
from mpo_apply_fixtures import ladder_engine
from mpo_entry_fixtures import model_state, sorted_mpo
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import np_conserved as npc

OUT = ('vR*', 'p0', 'wR', 'vR')
CLASSES = ['MpoApplyPlan', 'MpoBlockApplyPlan', 'MpoEntryApplyPlan']


@pytest.fixture
def emulation(monkeypatch):
    npc.clear_device_caches()
    mock_mpo_entry.install(monkeypatch)
    yield
    npc.clear_device_caches()


def _xxz(L, Jz):
    from tenpy_amd.models.spin_chains import xxz_chain_mpo
    return xxz_chain_mpo(L, 1., Jz, 0.1)


def _inputs(name):
    """``(cls, X, W, W_other)``: the plan class, ``X = LP . theta`` on a bulk site, the MPO tensor of that site and the tensor of the same
    model with other couplings (same block structure)."""
    from tenpy_amd.models.hubbard import hubbard_ladder_mpo
    if name == 'MpoApplyPlan':
        from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
        from tenpy_amd.models.spin_chains import spin_half_leg
        from tenpy_amd.networks.mps import MPS
        psi = MPS.from_product_state([spin_half_leg('Sz')[1]] * 6, [1, 0] * 3)
        eng = TwoSiteDMRGEngine(psi, _xxz(6, 0.7), {'trunc_params': {'chi_max': 8, 'svd_min': 1.e-10}, 'lanczos_params': {}})
        eng.sweep()
        env, other = eng.env, _xxz(6, 0.3)
    elif name == 'MpoBlockApplyPlan':
        eng = ladder_engine(2, False, ('N',), chi=16, sweeps=1)
        psi, env, other = eng.psi, eng.env, hubbard_ladder_mpo(2, 1., 2., 0., conserve=('N',))
    else:
        _, psi, env = model_state('mock', 'xxz_sorted')
        other = sorted_mpo(_xxz(psi.L, 0.3))
    i0 = psi.L // 2
    op = mps_common.OneSiteH(env, i0)
    assert op.factored
    X = npc.tensordot(op._LPf, op.combine_theta(psi.get_theta(i0, n=1)), axes=['vR', 'vL'])      # vR*, wR, p0, vR
    W_other = other.get_W(i0).replace_labels(['p', 'p*'], ['p0', 'p0*'])
    cls = getattr(mps_common, name)
    assert mps_common._mpo_plan_class(op.W0) is mps_common._mpo_plan_class(W_other) is cls
    assert not np.array_equal(op.W0.to_ndarray(), W_other.to_ndarray()) and op.W0.to_ndarray().shape == W_other.to_ndarray().shape
    return cls, X, op.W0, W_other


def _get(cls, X, W):
    return cls.get(X, W, *mps_common._STEP_LR, OUT)


def _tables(plan):
    return [getattr(plan, k) for k in ('jobs_host', 'terms_host', 'coeff_host', 'rows_host') if hasattr(plan, k)]


@pytest.mark.parametrize("name", CLASSES)
def test_get_is_cached_per_class(emulation, name):
    """(a) equal arguments: the same object; after ``clear_device_caches()``: a new one with the same tables.  Every class has a cache of
    its own, and the step functions of the operators reach the same entry."""
    cls, X, W, _ = _inputs(name)
    assert issubclass(cls, mps_common._MpoStepPlan) and '_cache' in vars(cls)
    plan = _get(cls, X, W)
    assert type(plan) is cls and not plan.empty
    assert _get(cls, X, W) is plan
    assert mps_common._mpo_step_lr(X, W, out_labels=OUT) is plan
    assert [c for c in CLASSES if plan in getattr(mps_common, c)._cache.values()] == [name]
    npc.clear_device_caches()
    assert len(cls._cache) == 0
    again = _get(cls, X, W)
    assert again is not plan and type(again) is cls
    assert all(np.array_equal(a, b) for a, b in zip(_tables(again), _tables(plan))) and len(_tables(plan)) >= 2
    assert np.array_equal(again.qdata, plan.qdata) and np.array_equal(again.offsets, plan.offsets) and again.total == plan.total


@pytest.mark.parametrize("name", CLASSES)
def test_stale_plan_under_a_reused_id_is_rebuilt(emulation, name):
    """(b) the cache key holds the ``id()`` of the MPO's host table.  A plan whose table has died can meet a new table with the old id
    under its key: ``get`` must compare the tables themselves and rebuild, or it would apply the OLD couplings."""
    cls, X, W, W_other = _inputs(name)
    want = cls(X, W_other, *mps_common._STEP_LR, OUT)                   # never cached
    old = _get(cls, X, W)
    assert any(not np.array_equal(a, b) for a, b in zip(_tables(old), _tables(want))), "the couplings must show in the tables"
    old_id = id(cls._table(W))
    assert old._tables_alive[0] is cls._table(W), "a cached plan keeps its table alive"
    for attr in ('_tpa_entries', '_tpa_blocks', '_tpa_coo', '_tpa_origin'):         # drop the MPO tensor's cached tables
        W.__dict__.pop(attr, None)
    del W
    table = cls._table(W_other)
    got = _get(cls, X, W_other)
    key = [k for k, v in cls._cache.items() if v is got]
    assert len(key) == 1
    # A cached plan keeps its table alive, so while `old` is cached CPython cannot hand its table's id to a new one: in practice this
    # branch is always taken, and it alone is what the test covers -- the old plan is put where a reused id would have found it.
    if id(table) != old_id:
        cls._cache[key[0]] = old
        got = _get(cls, X, W_other)
    assert got is not old and cls._cache[key[0]] is got and got._tables_alive[0] is table
    assert all(np.array_equal(a, b) for a, b in zip(_tables(got), _tables(want)))
    assert _get(cls, X, W_other) is got


def _zeroed(W):
    """``W`` with every stored block set to zero and none of the host tables that ``W`` had cached: they are read again."""
    Z = W.copy(deep=True)
    Z._arena.zero_()
    for attr in [a for a in vars(Z) if a.startswith('_tpa_')]:
        del Z.__dict__[attr]
    _, blocks = mps_common._mpo_blocks(Z)
    assert len(blocks) == W.stored_blocks > 0 and not any(np.any(b) for b in blocks)
    return Z


@pytest.mark.parametrize("sites", [1, 2])
def test_block_plan_without_a_surviving_key(emulation, sites):
    """``MpoBlockApplyPlan`` drops terms whose matrix is exactly zero.  With an MPO tensor of zeros (two sites: W1, so that every joined
    Kronecker product is zero) no key survives: the plan is empty, has the bookkeeping of Y, and ``apply`` gives an Array without blocks."""
    eng = ladder_engine(2, False, ('N',), chi=16, sweeps=1)
    i0 = eng.psi.L // 2 - 1
    fac = mps_common.TwoSiteH(None, i0, tensors=(eng.env.get_LP(i0), eng.env.get_RP(i0 + 1), eng.H.get_W(i0), eng.H.get_W(i0 + 1)),
                              factored=True)
    assert fac.factored and mps_common._mpo_plan_class(fac.W0, fac.W1) is mps_common.MpoBlockApplyPlan
    if sites == 1:
        theta = eng.psi.get_theta(i0, n=1).transpose(['vL', 'p0', 'vR'])
        args, out = (_zeroed(fac.W0),) + mps_common._STEP_LR + (OUT,), OUT
        kwargs = {}
    else:
        theta = fac.combine_theta(eng.psi.get_theta(i0, n=2))
        out = ('vR*', 'p0', 'p1', 'wR', 'vR')
        args, kwargs = (fac.W0,) + mps_common._STEP_LR + (out,), dict(W2=_zeroed(fac.W1), x_p2='p1', p2_out='p1', p2_in='p1*')
    X = npc.tensordot(fac._LPf, theta, axes=['vR', 'vL'])
    assert X.stored_blocks > 0
    full = mps_common.MpoBlockApplyPlan(X, fac.W0, *args[1:], **(dict(kwargs, W2=fac.W1) if kwargs else {}))
    assert not full.empty, "with the MPO's own tensors the step is not empty"
    for plan in (mps_common.MpoBlockApplyPlan(X, *args, **kwargs), mps_common.MpoBlockApplyPlan.get(X, *args, **kwargs)):
        assert plan.empty is True
        assert plan.labels == list(out) and plan.dtype == full.dtype and np.array_equal(plan.qtotal, full.qtotal)
        assert [l.ind_len for l in plan.legs] == [l.ind_len for l in full.legs]
        for launch in (True, False):
            Y = plan.apply(X, launch=launch)
            assert Y.stored_blocks == 0 and list(Y.get_leg_labels()) == list(out) and Y.dtype == full.dtype
    assert mps_common.MpoBlockApplyPlan.get(X, *args, **kwargs) is plan


def test_factored_plans_one_dict_and_hand_over(emulation):
    """(c) ``matvec`` and ``matvec_program`` of one ``TwoSiteH`` share one dict of plans; plans handed over from an earlier visit of the
    bond (``dmrg.py``: ``eff_H._fplans = cache[i0]``) are rebuilt when an environment has another block structure."""
    eng = ladder_engine(2, False, ('N', '2*Sz'), chi=16, sweeps=1)
    i0 = eng.psi.L // 2 - 1
    LP, RP, W0, W1 = eng.env.get_LP(i0), eng.env.get_RP(i0 + 1), eng.H.get_W(i0), eng.H.get_W(i0 + 1)
    eff = mps_common.TwoSiteH(None, i0, tensors=(LP, RP, W0, W1), factored=True)
    assert eff.factored
    theta = eff.combine_theta(eng.psi.get_theta(i0, n=2))
    y = eff.matvec(theta)
    fp = eff._fplans
    assert sorted(fp) == ['a01', 'dtype', 'key', 'lkey', 'p1', 'p2', 'rkey'] and eff.flops_per_matvec > 0
    eff.matvec_program(theta)
    assert eff._fplans is fp
    assert np.array_equal(eff.matvec(theta)._arena.cpu().numpy(), y._arena.cpu().numpy()) and eff._fplans is fp
    hit = mps_common._factored_plans(eff._LPf, eff._RPf, theta, eff.W0, eff.W1, old=fp)
    assert hit[0] is fp and hit[1] is None and hit[2] is None
    other = mps_common.TwoSiteH(None, i0, tensors=(LP, RP, W0, W1), factored=True)
    other.matvec_program(theta)             # the program first: the same keys, no launch while building
    assert sorted(other._fplans) == sorted(fp) and other._fplans is not fp and other.flops_per_matvec == eff.flops_per_matvec
    assert np.array_equal(other.matvec(theta)._arena.cpu().numpy(), y._arena.cpu().numpy())
    # hand-over to an operator whose LP lacks a block
    LP2 = npc.Array(LP.legs, LP.dtype, LP.qtotal, LP.get_leg_labels())
    LP2._set_blocks(LP._qdata[:-1], zero=True, qdata_sorted=LP._qdata_sorted)
    new = mps_common.TwoSiteH(None, i0, tensors=(LP2, RP, W0, W1), factored=True)
    assert new._LPf._struct_key() != eff._LPf._struct_key()
    new._fplans = fp
    y2 = new.matvec(theta)
    assert new._fplans is not fp and new._fplans['lkey'] == new._LPf._struct_key() != fp['lkey'] and new._fplans['rkey'] == fp['rkey']
    fresh = mps_common.TwoSiteH(None, i0, tensors=(LP2, RP, W0, W1), factored=True).matvec(theta)
    assert np.array_equal(y2._qdata, fresh._qdata) and np.array_equal(y2._arena.cpu().numpy(), fresh._arena.cpu().numpy())
    # and on the operator itself: the environment exchanged under plans that were made for the old one
    eff._LPf = new._LPf
    y3 = eff.matvec(theta)
    assert eff._fplans is not fp and eff._fplans['lkey'] == new._LPf._struct_key()
    assert np.array_equal(y3._arena.cpu().numpy(), fresh._arena.cpu().numpy())
