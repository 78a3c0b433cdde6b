"""Host side of the batched sampling route (``tenpy_amd/networks/sample.py``) on the numpy emulation: the seg and group tables of
``SamplePlan`` for a hand-built X, the plan cache, the launch counts of a walk (they do not depend on the number of samples), the split
of a batch into several walks by the memory budget, and the counted decline reasons."""
import numpy as np
import pytest

from sample_fixtures import build_psi, golden, sbackend  # noqa: F401
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks import sample

pytestmark = pytest.mark.parametrize("sbackend", ["mock"], indirect=True)


def hand_built_x(seed=0):
    """X ['s', 'p', 'vR'] with three sectors of the stack leg (2, 1 and 3 rows; charges 0, 1, 2), a two-state site (charges 0, 1) and
    a 'vR' leg with the sectors 0, 1, 2, 3 of the widths 2, 3, 2, 1: six blocks, q_s + q_p = q_vR."""
    ch = ChargeInfo([1])
    s = LegCharge.from_qind(ch, [0, 2, 3, 6], [[0], [1], [2]], qconj=1)
    p = LegCharge.from_qind(ch, [0, 1, 2], [[0], [1]], qconj=1)
    v = LegCharge.from_qind(ch, [0, 2, 5, 7, 8], [[0], [1], [2], [3]], qconj=-1)
    rng = np.random.default_rng(seed)
    dense = np.zeros((6, 2, 8))
    for qs in range(3):
        for qp in range(2):
            qv = qs + qp
            dense[s.slices[qs]:s.slices[qs + 1], qp, v.slices[qv]:v.slices[qv + 1]] = rng.standard_normal((s.slices[qs + 1] - s.slices[qs], v.slices[qv + 1] - v.slices[qv]))
    return npc.Array.from_ndarray(dense, [s, p, v], labels=['s', 'p', 'vR']), dense


def test_tables_of_a_hand_built_x(sbackend):
    X, dense = hand_built_x()
    assert X.stored_blocks == 6
    plan = sample.SamplePlan(X)
    assert (plan.n_segs, plan.n_groups, plan.dim, plan.n_rows) == (6, 3, 2, 6)
    assert plan.groups_host.tolist() == [[0, 2, 0, 2], [2, 2, 2, 1], [4, 2, 3, 3]]
    #                            d  post sigma0                      (x_ld = d post: the blocks are contiguous)
    assert plan.segs_host[:, 1:].tolist() == [[2, 1, 2, 0, 0, 0, 0], [3, 1, 3, 1, 0, 0, 0], [3, 1, 3, 0, 0, 0, 0], [2, 1, 2, 1, 0, 0, 0],
                                              [2, 1, 2, 0, 0, 0, 0], [1, 1, 1, 1, 0, 0, 0]]
    assert plan.seg_q.tolist() == [0, 1, 1, 2, 2, 3] and plan.seg_of.tolist() == [[0, 1], [2, 3], [4, 5]]
    assert plan.row_group.tolist() == [0, 0, 1, 2, 2, 2]
    arena = dev.to_host(X._arena)
    rows, vs = [0, 2, 3, 6], [0, 2, 5, 7, 8]
    for k, (x_off, x_ld, d, post, sigma0) in enumerate(plan.segs_host[:, :5].tolist()):          # every seg points at its block
        g, qv = k // 2, plan.seg_q[k]
        want = dense[rows[g]:rows[g + 1], sigma0, vs[qv]:vs[qv + 1]]
        assert np.array_equal(arena[x_off:x_off + want.size].reshape(want.shape), want)
    spans = sorted((x_off, x_off + [2, 2, 1, 1, 3, 3][k] * x_ld) for k, (x_off, x_ld) in enumerate(plan.segs_host[:, :2].tolist()))
    assert spans[0][0] == 0 and spans[-1][1] == 24 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # (back to back)
    assert plan.bytes == 8 * 24
    assert np.array_equal(dev.to_host(plan.segs_dev), plan.segs_host) and np.array_equal(dev.to_host(plan.groups_dev), plan.groups_host)
    # the launch on these tables: rows 0, 1 can give 0 or 1, u = 0 takes the first outcome with p > 0
    out = dev.empty(24, np.float64)
    plan.launch(X, dev.to_device(np.zeros(6)), out)
    host = dev.to_host(out).reshape(6, 4)
    p = np.sum(dense.reshape(6, 2, 8)**2, axis=2)
    assert host[:, 0].tolist() == [0] * 6 and np.allclose(host[:, 1], np.sqrt(p[:, 0]), rtol=1e-15) and np.allclose(host[:, 2], p.sum(1), rtol=1e-15)
    with pytest.raises(ValueError):
        sample.SamplePlan(X.transpose(['p', 's', 'vR']))


def test_cache_hit_on_equal_structure(sbackend):
    X, _ = hand_built_x(0)
    Y, _ = hand_built_x(1)
    plan = sample.SamplePlan.get(X)
    assert sample.SamplePlan.get(Y) is plan and len(sample.SamplePlan._cache) == 1
    assert sample.SamplePlan.get(Y.astype(np.complex128)) is not plan
    sample.clear_caches()
    assert len(sample.SamplePlan._cache) == 0


def _xxz():
    rec = [r for r in golden() if r['name'] == 'xxz'][0]
    return rec, build_psi(rec)


@pytest.mark.parametrize("n", [3, 17])
def test_launch_counts_do_not_depend_on_n(sbackend, n):
    """A whole chain of L sites: L tensordots, L select launches, L gather launches (the last one leaves the phases) and L + 1
    device-to-host copies (the phases); a part of the chain: one gather launch and one copy less."""
    import mock_sample
    rec, psi = _xxz()
    L = psi.L
    c0 = dict(mock_sample.calls)
    psi.sample_measurements(rng=np.random.default_rng(1), n_samples=n)
    st = sample.sample_stats
    assert (st['walks'], st['tensordots'], st['select_launches'], st['gather_launches'], st['d2h'], st['uploads']) == (1, L, L, L, L + 1, L + 1)
    assert mock_sample.calls['tpa_sample_select_batch'] - c0['tpa_sample_select_batch'] == L
    assert mock_sample.calls['tpa_sample_gather_batch'] - c0['tpa_sample_gather_batch'] == L
    sample.reset_stats()
    psi.sample_measurements(0, 4, rng=np.random.default_rng(1), n_samples=n)
    assert (st['walks'], st['tensordots'], st['select_launches'], st['gather_launches'], st['d2h']) == (1, 5, 5, 4, 5)
    sample.reset_stats()
    psi.sample_measurements(ops=[rec['ops']['Sz']], rng=np.random.default_rng(1), n_samples=n)
    assert (st['tensordots'], st['select_launches'], st['gather_launches']) == (2 * L, L, L)          # (one rotation per site)
    assert st['device'] == 1 and st['generic'] == 0


def test_budget_split_gives_the_same_samples(sbackend, monkeypatch):
    """A budget for 5 samples per walk: a batch of 12 takes three walks and returns the outcomes of the one-walk batch; the weights
    agree to the rounding of the GEMM, whose summation order may depend on the number of rows."""
    rec, psi = _xxz()
    sig, wts = psi.sample_measurements(rng=np.random.default_rng(7), n_samples=12)
    assert sample.sample_stats['walks'] == 1
    monkeypatch.setattr(sample, '_budget', lambda: 5 * sample._sample_bytes(psi, 0, psi.L - 1))
    sample.reset_stats()
    sig2, wts2 = psi.sample_measurements(rng=np.random.default_rng(7), n_samples=12)
    assert sample.sample_stats['walks'] == 3 and sample.sample_stats['select_launches'] == 3 * psi.L
    assert np.array_equal(sig, sig2) and np.allclose(wts, wts2, rtol=16 * psi.L * 2.**-53, atol=0)


def test_every_decline_reason_is_counted(sbackend, monkeypatch):
    from tenpy_amd.networks.mps import MPS
    rec, psi = _xxz()
    rng = np.random.default_rng(3)

    def reason(expect, *args, **kw):
        sample.reset_stats()
        psi_ = kw.pop('psi', psi)
        assert sample.decline_reason(psi_, *args, n_samples=kw.get('n_samples')) == expect
        res = psi_.sample_measurements(*args, rng=rng, **kw)
        assert sample.sample_stats['why'] == {expect: 1} and sample.sample_stats['generic'] == 1 and sample.sample_stats['device'] == 0
        assert sample.sample_stats['select_launches'] == 0
        return res

    sig, w = reason('first_site', 3, 5, n_samples=2)
    assert sig.shape == (2, 3) and w.shape == (2,)
    monkeypatch.setattr(sample, 'SINGLE', False)
    s1, w1 = reason('single_sample')
    assert isinstance(s1, list) and len(s1) == psi.L and np.ndim(w1) == 0
    monkeypatch.setattr(sample, 'SAMPLE', False)
    reason('switched_off', n_samples=2)
    monkeypatch.setattr(sample, 'SAMPLE', True)
    monkeypatch.setattr(sample, 'SAMPLE_MAX_DIM', 1)
    reason('site_dim', n_samples=2)
    monkeypatch.setattr(sample, 'SAMPLE_MAX_DIM', 64)

    class Sub(MPS):
        pass
    sub = Sub(psi.p_legs, list(psi._B), list(psi._S))
    sub.form = list(psi.form)
    reason('not_plain_finite', n_samples=2, psi=sub)
    inf = psi.copy()
    inf.bc = 'infinite'
    assert sample.decline_reason(inf, n_samples=2) == 'not_plain_finite'
    two = psi.copy()
    two._p_label = ['p0', 'p1']
    sample.reset_stats()
    assert sample.decline_reason(two, n_samples=2) == 'p_label'
    with pytest.raises(NotImplementedError):
        two.sample_measurements(rng=rng, n_samples=2)
    assert sample.sample_stats['why'] == {'p_label': 1}
    mock = dev.lib()
    monkeypatch.delattr(mock, 'tpa_sample_gather_batch')
    reason('no_kernel', n_samples=2)
