"""Host logic of ``rho.SiteRhoPlan`` on the numpy emulation: the job table of a hand-built two-sector structure entry by entry, the
cache, and the guard on the number of jobs."""
import numpy as np
import pytest

from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks import rho


@pytest.fixture
def mock(monkeypatch):
    import mock_rho
    from mpo_cell_fixtures import _forget
    _forget()
    rho.clear_caches()
    mock_rho.install(monkeypatch)
    rho.reset_stats()
    yield mock_rho
    _forget()
    rho.clear_caches()


def structure(q_stack=0, n_stack=3):
    """B ['vL', 'p', 'vR']: vL sectors q = 0 (2 states), 1 (3); p sectors q = 0 (1 state), 1 (2 states); vR sectors q = 1 (4), 2 (5).
    X ['vR*', 's', 'p', 'vR'] on the same legs with the total charge ``q_stack``."""
    ci = ChargeInfo([1])
    vL = LegCharge.from_qind(ci, [0, 2, 5], [[0], [1]], qconj=+1)
    p = LegCharge.from_qind(ci, [0, 1, 3], [[0], [1]], qconj=+1)
    vR = LegCharge.from_qind(ci, [0, 4, 9], [[1], [2]], qconj=-1)
    s = LegCharge.from_trivial(n_stack, ci, 1)
    rng = np.random.default_rng(3)
    B = npc.Array.from_func(rng.standard_normal, [vL, p, vR], labels=['vL', 'p', 'vR'], shape_kw='size')
    X = npc.Array.from_func(rng.standard_normal, [vL, s, p, vR], qtotal=[q_stack], labels=['vR*', 's', 'p', 'vR'], shape_kw='size')
    return B, X


def test_job_table_entry_by_entry(mock):
    """Charge rule q_vL + q_p - q_vR = 0 for B: blocks (0, 1, 1), (1, 0, 1), (1, 1, 2).  X with the same total charge has the same
    blocks: three jobs on the diagonal tiles.  X with total charge -1 (q_vL + q_p - q_vR = -1) has the blocks (0, 0, 1), (0, 1, 2),
    (1, 0, 2): (0, 0, 1) meets B's (0, 1, 1) -- the tile of (p' sector 1, p sector 0) at row 1, column 0 --, (1, 0, 2) meets B's
    (1, 1, 2), and (0, 1, 2) has no partner among the blocks of B: no job."""
    B, X = structure()
    plan = rho.SiteRhoPlan.get(B, X)
    assert plan.d == 3 and plan.out_size == 9 and plan.max_d == 2 and plan.n_stack == 3
    bq = B._qdata.tolist()
    assert sorted(bq) == [[0, 1, 0], [1, 0, 0], [1, 1, 1]]           # (qindices)
    ext = {'vL': [2, 3], 'p': [1, 2], 'vR': [4, 5]}
    want = []
    for nx, (qa, _, qp, qc) in enumerate(X._qdata.tolist()):
        nb = bq.index([qa, qp, qc])
        pre, d, post = ext['vL'][qa], ext['p'][qp], ext['vR'][qc]
        first = [0, 1][qp]
        want.append([int(B._offsets[nb]), d * post, d, int(X._offsets[nx]), 3 * d * post, d * post, d, pre, post, first * 3 + first, 3, 0])
    assert plan.jobs_host.tolist() == want and plan.n_jobs == 3 and plan.max_cols == 3 * 5
    out = rho.dev.zeros(2 * 3 * 9, np.float64)
    plan.launch(B, X, out.data_ptr())
    got = rho.dev.to_host(out).reshape(3, 3, 3, 2)
    dense = np.einsum('aoc,aspc->sop', B.to_ndarray().conj(), X.to_ndarray())
    assert np.max(np.abs(got[..., 0] - dense)) < 1e-13 and np.all(got[..., 1] == 0)
    assert np.all(got[:, 0, 1:] == 0) and np.all(got[:, 1:, 0] == 0)

    B, X = structure(q_stack=-1)
    plan = rho.SiteRhoPlan.get(B, X)
    xq = X._qdata.tolist()
    assert sorted(xq) == [[0, 0, 0, 0], [0, 0, 1, 1], [1, 0, 0, 1]]
    want = []
    for nx, (qa, _, qp, qc) in enumerate(xq):
        if qp == 1:
            continue
        nb = bq.index([qa, 1, qc])
        pre, post = ext['vL'][qa], ext['vR'][qc]
        want.append([int(B._offsets[nb]), 2 * post, 2, int(X._offsets[nx]), 3 * post, post, 1, pre, post, 1 * 3 + 0, 3, 0])
    assert plan.jobs_host.tolist() == want
    plan.launch(B, X, out.data_ptr())
    got = rho.dev.to_host(out).reshape(3, 3, 3, 2)
    dense = np.einsum('aoc,aspc->sop', B.to_ndarray().conj(), X.to_ndarray())
    assert np.max(np.abs(got[..., 0] - dense)) < 1e-13 and np.any(got[:, 1:, 0, 0] != 0)
    assert np.all(got[:, 0] == 0) and np.all(got[:, :, 1:] == 0)         # (both jobs write the one tile; the rest: exact zeros)


def test_cache_hit_on_the_second_call(mock):
    B, X = structure()
    plan = rho.SiteRhoPlan.get(B, X)
    B2, X2 = structure()
    assert rho.SiteRhoPlan.get(B2, X2) is plan and len(rho.SiteRhoPlan._cache) == 1
    assert rho.SiteRhoPlan.get(*structure(q_stack=-1)) is not plan
    assert rho.SiteRhoPlan.get(*structure(n_stack=4)) is not plan and len(rho.SiteRhoPlan._cache) == 3


def test_job_guard(mock, monkeypatch):
    """More jobs than one launch takes (60000; here the guard is lowered to 2 for a structure of three jobs)."""
    assert rho.SiteRhoPlan.MAX_JOBS == 60000
    monkeypatch.setattr(rho.SiteRhoPlan, 'MAX_JOBS', 2)
    with pytest.raises(ValueError, match="3 jobs for one launch"):
        rho.SiteRhoPlan(*structure())


def test_wide_sector_is_refused(mock):
    ci = ChargeInfo()
    vL, p, vR = LegCharge.from_trivial(2, ci), LegCharge.from_trivial(5, ci), LegCharge.from_trivial(2, ci, -1)
    B = npc.Array.from_func(np.ones, [vL, p, vR], labels=['vL', 'p', 'vR'])
    with pytest.raises(ValueError, match="wider than 4"):
        rho.SiteRhoPlan(B, B)
