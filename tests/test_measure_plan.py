"""Host logic of the device measurement route (``tenpy_amd/networks/measure.py``) on the numpy emulation: the job tables of
``SiteInnerPlan`` for a charged operator, a neutral operator and the charge-free case, the counters of a full stacked walk at L = 8, and
every decline reason once, each returning what the row-by-row statements return."""
import numpy as np
import pytest

from measure_fixtures import build_psi, golden
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks import measure
from tenpy_amd.networks.mps import MPS


@pytest.fixture
def mock(monkeypatch):
    import mock_measure
    from mpo_cell_fixtures import _forget
    _forget()
    measure.clear_caches()
    mock_measure.install(monkeypatch)
    monkeypatch.setattr(measure, 'MEASURE', True)
    measure.reset_stats()
    yield mock_measure
    _forget()
    measure.clear_caches()


def rec_of(name):
    return [r for r in golden() if r['name'] == name][0]


def dense_value(B, X, op):
    """sum conj(B[a, p', c]) op[p', p] X[a, s, p, c] per stack slot, from the dense tensors."""
    return np.einsum('aoc,op,aspc->s', B.to_ndarray().conj(), op, X.to_ndarray())


def stack_and_X(psi, r, ops, n):
    """A stack of ``n`` start matrices (site r - 1) and its product with B_r."""
    stack = None
    for s in range(n):
        C = measure._start_matrix(psi, ops[s % len(ops)], r - 1)
        stack = measure._push(stack, C, s)
    B = psi.get_B(r, 'B')
    return B, npc.tensordot(stack, B, axes=['vR', 'vL'])


@pytest.mark.parametrize("name,op1,op2", [('xxz', 'Sp', 'Sm'), ('xxz', 'Sz', 'Sz'), ('tfi', 'Sx', 'Sx')],
                         ids=['charged', 'neutral', 'charge_free'])
def test_job_tables(mock, name, op1, op2):
    """One job per pair of blocks of B and X with equal virtual sectors and a nonzero sector block of the operator; the stack index
    sits between the row and the physical index; the emulated launch gives the dense contraction."""
    rec = rec_of(name)
    psi = build_psi(rec)
    r = 4
    A = measure.as_site_op(rec['ops'][op1], psi.p_legs[r - 1])
    B, X = stack_and_X(psi, r, [A], 5)
    assert list(X.get_leg_labels()) == ['vR*', 's', 'p', 'vR'] and X.get_leg('s').ind_len >= 5
    O = rec['ops'][op2]
    plan = measure.SiteInnerPlan.get(B, X, [O])
    assert plan is measure.SiteInnerPlan.get(B, X, [O]) and plan.n_out == 1
    S = X.get_leg('s').ind_len
    psl = np.asarray(B.get_leg('p').slices)
    want = set()
    for nx, (qa, _, qp, qc) in enumerate(X._qdata.tolist()):
        for nb, (ba, bp, bc) in enumerate(B._qdata.tolist()):
            if (ba, bc) == (qa, qc) and np.any(O[psl[bp]:psl[bp + 1], psl[qp]:psl[qp + 1]] != 0):
                want.add((int(B._offsets[nb]), int(X._offsets[nx])))
    jobs = plan.jobs_host
    assert {(int(j[0]), int(j[3])) for j in jobs} == want and len(jobs) == len(want) > 0
    xs = X._block_shapes()
    for j in jobs:
        nx = int(np.nonzero(X._offsets == j[3])[0][0])
        pre, _, d_x, post = xs[nx]
        assert (j[7], j[6], j[8]) == (pre, d_x, post) and j[5] == d_x * post and j[4] == S * d_x * post and j[1] == j[2] * post and j[10] == 0
    if name == 'tfi':
        assert len(jobs) == 1 and jobs[0][2] == jobs[0][6] == 2       # no charges: one block pair, the whole operator
    elif op2 == 'Sm':
        assert np.all(jobs[:, 2] == 1) and np.all(jobs[:, 6] == 1) and plan.coeff_host.tolist() == [1.]       # the one entry of Sm
    out = measure.dev.zeros(2 * S, np.float64)
    plan.launch(B, X, out.data_ptr())
    got = measure.dev.to_host(out).reshape(S, 2)
    assert np.max(np.abs(got[:, 0] + 1j * got[:, 1] - dense_value(B, X, O))) < 1e-13
    assert np.any(np.abs(got[:5]) > 1e-3) and np.all(got[5:] == 0)


def test_complex_operator_on_a_real_state(mock):
    """A complex operator on real tensors takes two output columns (real and imaginary part of the operator)."""
    rec = rec_of('tfi')
    psi = build_psi(rec)
    O = rec['ops']['Sx'] + 0.5j * rec['ops']['Sz']
    got = psi.expectation_value([O, rec['ops']['Sz']])
    assert np.max(np.abs(got[0] - (rec['expval']['Sx'] + 0.5j * rec['expval']['Sz']))) < 1e-12
    assert np.max(np.abs(got[1] - rec['expval']['Sz'])) < 1e-12


def test_counters_of_a_full_walk(mock, monkeypatch):
    """sites1 = sites2 = all 8 sites, hermitian: one walk; one kernel launch per closing site with a started row (sites 1 .. 7), two
    tensordots per transfer step (sites 1 .. 6; the last site only closes), one device-to-host copy, at most 25 % of the transfer
    flops on empty stack slots; the emulated entry point is called exactly as often as the route counts."""
    rec = rec_of('xxz')
    psi = build_psi(rec)
    n_td = [0]
    real_td = npc.tensordot

    def counted(*a, **kw):
        n_td[0] += 1
        return real_td(*a, **kw)
    monkeypatch.setattr(npc, 'tensordot', counted)
    mock.calls['tpa_site_inner_batch'] = 0
    hosts = {}
    ops = [measure.as_site_op(rec['ops'][n], psi.p_legs[0], hosts) for n in ('Sp', 'Sm')]
    up = measure.corr_up(psi, [ops[0]], [ops[1]], list(range(8)), list(range(8)), None, True, True, hosts=hosts)
    st = measure.measure_stats
    assert st['walks'] == 1 and st['device'] == 1 and st['generic'] == 0 and st['d2h'] == 1 and st['op_reads'] == 0
    assert st['kernel_launches'] == 7 == mock.calls['tpa_site_inner_batch']
    assert st['transfer_steps'] == 6 and st['transfer_tensordots'] == 12 and st['closing_tensordots'] == 1
    assert st['start_tensordots'] == 14 and st['opstr_tensordots'] == 0
    assert st['slot_copies'] == 6 and st['slot_adds'] == 0          # (rows 1 .. 6 join by a copy into their slot; row 0 is the stack)
    assert n_td[0] == st['transfer_tensordots'] + st['closing_tensordots'] + st['start_tensordots']
    assert st['filled'] == sum(range(1, 8)) and st['capacity'] - st['filled'] <= 0.25 * st['capacity']
    want = [c for c in rec['corr'] if c['op1'] == 'Sp' and c['sites1'] is None and not c['hermitian']][0]['result']
    iu = np.triu_indices(8, 1)
    assert np.max(np.abs(up[iu] - want[iu])) < 1e-12 and np.all(up[np.tril_indices(8)] == 0)


def test_capacity_grows_in_steps():
    filled = np.arange(1, 200)
    cap = np.array([measure._capacity(int(n)) for n in filled])
    assert np.all(cap >= filled) and np.all(cap - filled <= 0.25 * cap) and cap[0] == 1
    # a stack that regrows only when it is full changes its capacity every fifth start for large n
    grow, c = 0, 0
    for n in filled:
        if n > c:
            c, grow = measure._capacity(int(n)), grow + 1
    assert grow < 0.6 * len(filled)


def test_memory_budget_splits_the_walk(mock, monkeypatch):
    """A budget of three rows: sites1 = all sites goes in three walks with the same values."""
    rec = rec_of('xxz')
    psi = build_psi(rec)
    ops = [measure.as_site_op(rec['ops'][n], psi.p_legs[0]) for n in ('Sz', 'Sz')]
    one = measure.corr_up(psi, [ops[0]], [ops[1]], list(range(8)), list(range(8)), None, True, True)
    assert measure.measure_stats['walks'] == 1
    monkeypatch.setattr(measure, '_budget', lambda: 3 * measure._row_bytes(psi, 0, 7))
    measure.reset_stats()
    three = measure.corr_up(psi, [ops[0]], [ops[1]], list(range(8)), list(range(8)), None, True, True)
    assert measure.measure_stats['walks'] == 3 and measure.measure_stats['d2h'] == 3
    assert np.max(np.abs(one - three)) < 1e-13


def _generic(psi, ops1, ops2, **kw):
    return measure.corr_up(psi, ops1, ops2, list(range(psi.L)), list(range(psi.L)), None, True, True, why='reference', **kw)


def test_every_decline_reason_once(mock, monkeypatch):
    rec = rec_of('xxz')
    psi = build_psi(rec)
    leg = psi.p_legs[0]
    Sz, Sp, Sm = (measure.as_site_op(rec['ops'][n], leg) for n in ('Sz', 'Sp', 'Sm'))
    sites = list(range(8))
    want = _generic(psi, [Sp], [Sm])
    seen = []

    def declined(reason, psi_, ops1, ops2, want_, **kw):
        measure.reset_stats()
        got = measure.corr_up(psi_, ops1, ops2, list(range(psi_.L)), list(range(psi_.L)), None, True, True, **kw)
        st = measure.measure_stats
        assert st['why'] == {reason: 1} and st['generic'] == 1 and st['device'] == 0 and st['kernel_launches'] == 0, (reason, st)
        assert np.max(np.abs(got - want_)) < 1e-13
        seen.append(reason)

    inf = psi.copy()
    inf.bc = 'infinite'
    declined('infinite', inf, [Sp], [Sm], want)
    other = psi.copy()
    declined('bra_ne_ket', psi, [Sp], [Sm], want, bra=other)
    mixed = [Sp, Sz]        # the charge of the entries differs: no common total charge for the stack
    declined('op_charges', psi, mixed, [Sm], _generic(psi, mixed, [Sm]))
    declined('op_charges', psi, [Sp], [Sm, Sz], _generic(psi, [Sp], [Sm, Sz]))
    lab = psi.copy()
    lab._p_label = ['p0']
    declined('p_label', lab, [Sp], [Sm], want)
    # a physical sector of 17 states (no charges): a product state of three sites
    chinfo = ChargeInfo()
    wide = LegCharge.from_trivial(17, chinfo)
    prod = MPS.from_product_state([wide] * 3, [3, 0, 16])
    rng = np.random.default_rng(5)
    A, Bm = rng.standard_normal((17, 17)), rng.standard_normal((17, 17))
    a, b = measure.as_site_op(A, wide), measure.as_site_op(Bm, wide)
    occ = [3, 0, 16]
    dense = np.array([[A[occ[i], occ[i]] * Bm[occ[j], occ[j]] if j > i else 0. for j in range(3)] for i in range(3)])
    declined('wide_sector', prod, [a], [b], dense)
    monkeypatch.setattr(measure, 'MEASURE', False)
    declined('switched_off', psi, [Sp], [Sm], want)
    assert sorted(set(seen)) == ['bra_ne_ket', 'infinite', 'op_charges', 'p_label', 'switched_off', 'wide_sector']
    # and the public call of the stand-alone class on a chain the route declines
    measure.reset_stats()
    C = inf.correlation_function(rec['ops']['Sp'], rec['ops']['Sm'])
    ref = [c for c in rec['corr'] if c['op1'] == 'Sp' and c['sites1'] is None and not c['hermitian']][0]['result']
    assert np.max(np.abs(C - ref)) < 1e-12 and measure.measure_stats['why'] == {'switched_off': 3}      # (two triangles and the diagonal)


def test_derived_operators_are_measured_as_they_are(mock):
    """Operators given as device Arrays are read in every call: after ``A`` has been measured, ``2 A``, ``A.conj()``, a transposed
    copy and ``A`` scaled in place are measured as what they are now, in the list form of ``expectation_value`` and in
    ``correlation_function`` (nothing about an operator is remembered on the Array or across calls)."""
    rec = rec_of('xxz_tebd')
    psi = build_psi(rec)
    leg = psi.p_legs[0]
    Sz, Sp = rec['ops']['Sz'], rec['ops']['Sp']
    A = measure.as_site_op(Sz, leg)
    P = measure.as_site_op((1. + 0.5j) * Sp, leg)
    base = psi.expectation_value([A])[0]
    assert np.max(np.abs(base - rec['expval']['Sz'])) < 1e-12 and np.max(np.abs(base)) > 0.05
    assert measure.measure_stats['op_reads'] == 1 and not any(k.startswith('_tpa') for k in vars(A))
    twice, neg, summed = psi.expectation_value([2. * A, -A, A + A])
    assert np.max(np.abs(twice - 2 * base)) < 1e-12 and np.max(np.abs(neg + base)) < 1e-12 and np.max(np.abs(summed - 2 * base)) < 1e-12
    cSz = psi.correlation_function(A, A)
    assert np.max(np.abs(psi.correlation_function(A, 2. * A) - 2 * cSz)) < 1e-12
    assert np.max(np.abs(psi.correlation_function(3. * A, A) - 3 * cSz)) < 1e-12
    want = psi.correlation_function((1. + 0.5j) * Sp, ((1. + 0.5j) * Sp).conj().T)          # dense operators
    assert np.max(np.abs(want)) > 0.05
    got = psi.correlation_function(P, P.conj().itranspose(['p', 'p*']))        # 'p*', 'p' after conj: P^dagger
    assert np.max(np.abs(got - want)) < 1e-12
    assert np.max(np.abs(psi.correlation_function(P, P.conj().transpose(['p', 'p*'])) - want)) < 1e-12
    A.iscale_prefactor(4.)          # in place, on the object that was measured before
    assert np.max(np.abs(psi.expectation_value([A])[0] - 4 * base)) < 1e-12
    assert np.max(np.abs(psi.correlation_function(A, A) - 16 * cSz)) < 1e-12
    assert measure.measure_stats['generic'] == 0 and measure.measure_stats['device'] > 0


def test_list_form_declines_to_the_generic_statements(mock, monkeypatch):
    """``expectation_value`` with a list: a physical sector of 17 states, and the route switched off, go to the statements of the
    one-operator form with a counted reason and the same values."""
    wide = LegCharge.from_trivial(17, ChargeInfo())
    occ = [3, 0, 16]
    prod = MPS.from_product_state([wide] * 3, occ)
    rng = np.random.default_rng(6)
    A, Bm = rng.standard_normal((17, 17)), rng.standard_normal((17, 17))
    got = prod.expectation_value([A, Bm])
    assert measure.measure_stats['why'] == {'wide_sector': 1} and measure.measure_stats['kernel_launches'] == 0
    assert np.allclose(got[0], [A[o, o] for o in occ], atol=1e-14) and np.allclose(got[1], [Bm[o, o] for o in occ], atol=1e-14)
    assert np.allclose(got[0], prod.expectation_value(A), atol=1e-14)
    C = prod.correlation_function(A, Bm)        # (the diagonal goes the same way)
    assert np.allclose(np.diag(C), [(A @ Bm)[o, o] for o in occ], atol=1e-13)
    rec = rec_of('xxz')
    psi = build_psi(rec)
    monkeypatch.setattr(measure, 'MEASURE', False)
    measure.reset_stats()
    got = psi.expectation_value([rec['ops']['Sz']], sites=[5, 2])
    assert measure.measure_stats['why'] == {'switched_off': 1} and measure.measure_stats['kernel_launches'] == 0
    assert np.max(np.abs(got[0] - rec['expval']['Sz'][[5, 2]])) < 1e-12
