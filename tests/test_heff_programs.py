"""The launch programs of the effective Hamiltonians (``matvec_program`` of ``TwoSiteH``, ``OneSiteH``, ``ZeroSiteH``, ``PlusHcH`` and
``ShardedTwoSiteH``) against a recorded snapshot, ``tests/golden/heff_programs.json`` (written by ``tests/golden/make_golden_programs.py``
from :func:`build`): the rows in their order with their slot numbers, the sizes of the buffers, the counters of the plans and of the
operator.  Host tables only, on the emulated device.

Device addresses differ from run to run, so columns 2, 3, 4 and 10 of a row hold, in place of every non-zero address, the rank of its
first appearance within the program (zero stays zero): which rows share a table is kept.  :func:`_anchor` ties the ranks of some
cases to the tables of the plans.  Chains of L <= 10 at chi <= 32."""
import json
import os
import tempfile

import numpy as np
import pytest

from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'heff_programs.json')
SPLIT = (4, 1 << 30, 2, 1 << 30)        # every plan split (tests/test_split_k.py), also the short chains of step 1


def _encode(prog):
    ops = np.array(prog[0], dtype=np.int64)
    ranks = {}
    for row in ops:
        for c in (2, 3, 4, 10):
            if row[c]:
                row[c] = ranks.setdefault(int(row[c]), len(ranks) + 1)
    return dict(ops=ops.tolist(), bufs=[[int(t.numel()), str(t.dtype)] for t in prog[1]],
                plans=[[int(p.flops), int(p.bytes_min)] for p in prog[2]], collective=len(prog) > 3)


def _record(op, theta):
    """What is kept of ``op.matvec_program(theta)``; without a program: the structure filed for ``native_input`` and the program of
    the padded vector."""
    before = dict(kb.stats)
    prog = op.matvec_program(theta)
    rec = dict(program=None if prog is None else _encode(prog))
    if prog is None:
        holder = getattr(op, 'doubled', op)
        out = holder.__dict__.get('_program_out')
        rec['program_out'] = None if out is None else [np.asarray(out[1]).tolist(), np.asarray(out[2]).tolist(), int(out[3])]
        got = op.native_input(theta)
        rec['padded'] = None if got is None else _encode(got[1])
        rec['padded_numel'] = None if got is None else int(got[0]._arena.numel())
    counts = [getattr(op, 'flops_per_matvec', None), getattr(op, 'bytes_per_matvec', None)]
    rec['counts'] = [None if c is None else int(c) for c in counts]
    rec['skip'] = [kb.stats['n_skip_taken'] - before['n_skip_taken'], kb.stats['n_skip_declined'] - before['n_skip_declined']]
    return rec, prog


def _anchor(op, prog, step_key='a01', skipped=False):
    """The decoded ranks belong to the right tables: the first GEMM runs the tasks of ``p1``, the last one the tiles of ``p2`` (split-K:
    of their parts), and the MPO step of a full program is the row its plan writes."""
    fp, ops = op._fplans, prog[0]
    p1, p2 = fp['p1'], fp['p2']
    assert ops[0, 2] == (p1 if p1.sk is None else p1.sk).tasks_dev.data_ptr()
    last = [r for r in ops if r[0] in (0, 7)][-1]
    assert last[4] == (p2 if p2.sk is None else p2.sk).tiles_dev.data_ptr()
    if p2.sk is None:
        assert ops[-1, 4] == p2.tiles_dev.data_ptr()
    if not skipped:
        step = [r for r in ops if r[0] in (5, 6) or (r[0] == 1 and r[1] == 0)]
        assert len(step) == 1 and step[0].tolist() == fp[step_key].program_op(2, int(step[0][8]))


def _split_everything(mp):
    mp.setattr(npc, 'GEMM_SPLIT_K', SPLIT)
    mp.setattr(npc, 'GEMM_K_TILE', 2)           # (cuts snap to whole k-tiles: 16 would swallow the short chains of step 1)
    npc._plan_cache.clear()


def _xxz_engine(name, i0):
    from test_matvec_unit_program import _engine
    return _engine(name, i0)


def _two_site(mp, name, i0, skip, factored=True, split=False):
    import mock_device_ex
    mock_device_ex.install(mp)
    mp.setattr(mps_common, 'MATVEC_SKIP', False)
    eng = _xxz_engine(name, i0)
    mp.setattr(mps_common, 'MATVEC_SKIP', skip)
    if split:
        _split_everything(mp)
    op = mps_common.TwoSiteH(eng.env, i0, factored=factored)
    assert op.factored == factored
    theta = op.combine_theta(eng.psi.get_theta(i0, n=2))
    rec, _ = _record(op, theta)
    prog = op.native_input(theta)[1]            # (of theta, or of theta with zero blocks where H creates blocks: recorded as `padded`)
    if split:
        plans = (op._fplans['p1'], op._fplans['p2']) if factored else prog[2]
        assert all(p.sk is not None for p in plans), "the plans were not split"
    if factored:
        _anchor(op, prog, skipped=7 in prog[0][:, 0])
    return rec


def _blocks(mp):
    import mock_mpo_entry
    from mpo_apply_fixtures import bond_tensors, ladder_engine
    mock_mpo_entry.install(mp)
    eng = ladder_engine(2, False)
    i0 = eng.psi.L // 2 - 1
    op = mps_common.TwoSiteH(None, i0, tensors=bond_tensors(eng, i0), factored=True)
    got = op.native_input(op.combine_theta(eng.psi.get_theta(i0, n=2)))
    rec, prog = _record(op, got[0])
    assert prog is got[1] and 5 in prog[0][:, 0]
    _anchor(op, prog)
    return rec


def _entries(mp):
    import mock_mpo_entry
    from mpo_entry_fixtures import bond_tensors, model_state
    mock_mpo_entry.install(mp)
    H, psi, env = model_state('mock', 'xxz_sorted')
    i0 = psi.L // 2 - 1
    op = mps_common.TwoSiteH(None, i0, tensors=bond_tensors(H, env, i0), factored=True)
    got = op.native_input(op.combine_theta(psi.get_theta(i0, n=2)))
    rec, prog = _record(op, got[0])
    assert prog is got[1] and 6 in prog[0][:, 0]
    _anchor(op, prog)
    return rec


def _one_site_complex(mp):
    import mock_mpo_entry
    from tdvp_fixtures import build_operator, operator_record
    mock_mpo_entry.install(mp)
    op, theta = build_operator(operator_record('xxz_Sz', 'one'))
    rec, prog = _record(op, theta)
    assert theta.dtype == np.complex128 and prog is not None
    _anchor(op, prog, 'a0')
    return rec


def _local(mp, n, split=False):
    import mock_device_ex
    from plus_hc_fixtures import bond_matrix
    mock_device_ex.install(mp)
    eng = _xxz_engine('field', 4)
    if split:
        _split_everything(mp)
    if n == 1:
        op = mps_common.OneSiteH(eng.env, 4)
        theta = op.combine_theta(eng.psi.get_theta(4, n=1))
    else:
        op = mps_common.ZeroSiteH(eng.env, 5)
        theta = bond_matrix(eng.psi, 5, op.LP.dtype)
    assert op.factored
    rec, prog = _record(op, op.native_input(theta)[0])      # (theta, or theta with zero blocks where H creates blocks)
    assert not split or all(p.sk is not None for p in prog[2]), "the plans were not split"
    if n == 1:
        _anchor(op, prog, 'a0')
    else:                       # no MPO step: the second GEMM reads the result of the first
        assert op._fplans['a0'] is None and [int(r[6]) for r in prog[0] if r[0] == 0] == [0, 2]
    return rec


def _plus_hc(mp):
    import mock_mpo_entry
    from plus_hc_fixtures import model_state, nonsquare_bond, operator_and_vector
    mock_mpo_entry.install(mp)
    H, psi, env = model_state('mock', 'xxz')
    plain, theta = operator_and_vector(psi, env, nonsquare_bond(psi, env), 2)
    op = plain.plus_hc()
    assert isinstance(op, mps_common.PlusHcH)
    rec, prog = _record(op, theta)
    assert prog is not None and op.doubled.matvec_program(theta) is prog
    return rec


def _product_engine():
    from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
    from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
    from tenpy_amd.networks.mps import MPS
    _, p = spin_half_leg('Sz')
    psi = MPS.from_product_state([p] * 10, [1, 0] * 5)
    return TwoSiteDMRGEngine(psi, xxz_chain_mpo(10, 1., 1., 0.), {'trunc_params': {'chi_max': 32, 'svd_min': 1.e-12}, 'lanczos_params': {}})


def _product_state(mp):
    import mock_device_ex
    mock_device_ex.install(mp)
    mp.setattr(mps_common, 'MATVEC_SKIP', True)
    eng = _product_engine()
    op = mps_common.TwoSiteH(eng.env, 0, factored=True)
    rec, prog = _record(op, op.combine_theta(eng.psi.get_theta(0, n=2)))
    assert prog is None and rec['program_out'] is not None and rec['padded'] is not None, "H creates blocks: the padded vector has the program"
    return rec


def _sharded(mp, factored, closed=True):
    import torch.distributed as dist
    if not dist.is_available() or not dist.is_gloo_available():
        pytest.skip("torch.distributed with the gloo backend is not available in this process")
    import mock_device
    from tenpy_amd.algorithms.sharded import ShardedTwoSiteH
    mock_device.install(mp)
    mp.setenv('TPA_SHARD_FORCE', '1')
    mp.setattr(mps_common, 'MATVEC_SKIP', False)
    mp.setattr(mps_common, 'FACTORED_MIN_SECTOR', 0)
    eng = _xxz_engine('field', 4) if closed else _product_engine()      # (a product state: H creates blocks)
    mp.setattr(mps_common, 'FACTORED_MATVEC', factored)
    with tempfile.TemporaryDirectory() as tmp:
        dist.init_process_group('gloo', init_method='file://' + os.path.join(tmp, 'store'), rank=0, world_size=1)
        try:
            op = ShardedTwoSiteH(eng.env, 4)
            assert op.factored == factored and op.world == 1
            theta = op.combine_theta(eng.psi.get_theta(4, n=2))
            rec, prog = _record(op, op.native_input(theta)[0] if closed else theta)
        finally:
            dist.destroy_process_group()
    if closed:                  # (one rank: the pack copy, the collective, nothing to unpack)
        kinds = [int(k) for k in prog[0][:, 0]]
        assert kinds.count(2) == 1 and kinds.count(3) == 1 and len(prog) == 4 and (1 in kinds) == factored
    else:
        assert prog is None and rec['program_out'] is not None
    return rec


CASES = {
    'fused_xxz': lambda mp: _two_site(mp, 'field', 4, False, factored=False),
    'factored_heis': lambda mp: _two_site(mp, 'heis', 4, False),
    'factored_blocks': _blocks,
    'factored_entries': _entries,
    'skip_heis': lambda mp: _two_site(mp, 'heis', 4, True),
    'skip_long': lambda mp: _two_site(mp, 'long', 4, True),
    'skip_heis_first_bond': lambda mp: _two_site(mp, 'heis', 0, True),
    'skip_heis_second_bond': lambda mp: _two_site(mp, 'heis', 1, True),
    'skip_long_last_bond': lambda mp: _two_site(mp, 'long', 8, True),
    'factored_heis_split': lambda mp: _two_site(mp, 'heis', 4, False, split=True),
    'skip_heis_split': lambda mp: _two_site(mp, 'heis', 4, True, split=True),
    'skip_long_split': lambda mp: _two_site(mp, 'long', 4, True, split=True),
    'fused_xxz_split': lambda mp: _two_site(mp, 'field', 4, False, factored=False, split=True),
    'one_site_complex': _one_site_complex,
    'one_site_real': lambda mp: _local(mp, 1),
    'one_site_real_split': lambda mp: _local(mp, 1, split=True),
    'zero_site': lambda mp: _local(mp, 0),
    'plus_hc': _plus_hc,
    'product_state': _product_state,
    'sharded_factored': lambda mp: _sharded(mp, True),
    'sharded_fused': lambda mp: _sharded(mp, False),
    'sharded_open': lambda mp: _sharded(mp, True, closed=False),
}


def build(name, mp):
    """The record of one case, in the form ``json`` gives it back."""
    npc.clear_device_caches()
    try:
        return json.loads(json.dumps(CASES[name](mp)))
    finally:
        npc.clear_device_caches()


@pytest.mark.parametrize("name", list(CASES))
def test_program_is_the_recorded_one(monkeypatch, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = build(name, monkeypatch)
    for key in sorted(set(want) | set(got)):
        assert got.get(key) == want.get(key), "%s: %s differs from the recorded program" % (name, key)
