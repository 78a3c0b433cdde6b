"""The stacked walk of ``tenpy_amd/networks/rho.py`` on the recorded states of ``tests/golden/mutinf.pkl``, on the numpy emulation
(``mock``) and on the MI355X (``gpu``): the slot count (d (d + 1) / 2 per row), the ring (a stack never holds more than ``max_range``
rows, and the values equal those of the full walk), the split into several walks under a small memory budget (bit-equal results),
the launch and copy counters, and the declined calls (``TPA_MUTINF=0``, a physical sector of five states)."""
import numpy as np
import pytest

from measure_fixtures import LaunchCounter
from rho_fixtures import rbackend, state  # noqa: F401
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks import measure
from tenpy_amd.networks import rho as rho_mod
from tenpy_amd.networks.mps import MPS


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ['xxz', 'spin1', 'hubbard'])
def test_slots_launches_and_copies(rbackend, monkeypatch, name):
    """``slots == d (d + 1) / 2 * rows < slots_full``; one launch per closing site and stack, counted as often as the entry point is
    called; one device-to-host copy per walk."""
    rec, psi = state(name, rbackend)
    L, d = psi.L, rec['rho1'][0].shape[0]
    counter = LaunchCounter(monkeypatch, 'tpa_site_rho_batch')
    coords, rhos = rho_mod.device_two_site_rho(psi)
    st = rho_mod.rho_stats
    rows = L - 1
    assert st['slots'] == d * (d + 1) // 2 * rows and st['slots_full'] == d * d * rows and st['slots'] < st['slots_full']
    assert st['walks'] == 1 and st['d2h'] == st['walks'] and st['kernel_launches'] == counter.n > 0
    n_stacks = len(rho_mod._row_slots(psi.p_legs[0]))
    assert counter.n <= n_stacks * (L - 1) and st['transfer_steps'] <= n_stacks * (L - 2)
    assert st['start_tensordots'] == 2 * st['slots']
    if rbackend == 'mock':
        import mock_rho
        n0, k0 = mock_rho.calls['tpa_site_rho_batch'], st['kernel_launches']
        rho_mod.device_two_site_rho(psi, 2)
        assert mock_rho.calls['tpa_site_rho_batch'] - n0 == st['kernel_launches'] - k0 > 0


@pytest.mark.parametrize("name", ['xxz', 'xxz_tebd', 'hubbard'])
def test_ring_keeps_max_range_rows(rbackend, monkeypatch, name):
    """``max_range=3`` on L = 8 (6 for Hubbard): every stack leg holds three rows or fewer, and the values equal those of
    ``max_range=None`` on the shared pairs to the golden tolerance (the ring changes which rows share a GEMM, nothing else)."""
    rec, psi = state(name, rbackend)
    caps = []
    real_launch = rho_mod.SiteRhoPlan.launch

    def launch(self, B, X, out_ptr, n_stack=None):
        caps.append((self.n_stack, len(rho_mod._row_slots(B.get_leg('p')).get(tuple(int(q) for q in X.qtotal), ()))))
        return real_launch(self, B, X, out_ptr, n_stack)
    monkeypatch.setattr(rho_mod.SiteRhoPlan, 'launch', launch)
    c3, r3 = rho_mod.device_two_site_rho(psi, 3)
    assert rho_mod.rho_stats['ring_rows'] == 3 and rho_mod.rho_stats['walks'] == 1
    assert caps and all(width > 0 and n_stack <= 3 * width for n_stack, width in caps)
    call, rall = rho_mod.device_two_site_rho(psi)
    full = {tuple(p): r for p, r in zip(call.tolist(), rall)}
    assert c3.tolist() == [[i, j] for i in range(psi.L) for j in range(i + 1, min(i + 4, psi.L))]
    for p, r in zip(c3.tolist(), r3):
        assert np.max(np.abs(r - full[tuple(p)])) <= 1e-12
        assert np.max(np.abs(r - rec['rho2'][tuple(p)])) <= 1e-12


@pytest.mark.parametrize("name", ['xxz', 'xxz_tebd', 'tfi', 'hubbard'])
def test_nearest_neighbour_pairs_restart_the_stacks(rbackend, name):
    """``max_range=1``: every open row leaves at every site, so no stack is carried over a site -- the row that starts at site r
    begins new stacks on the bond right of r (the old ones stand on the bond left of it, with other legs).  One row per stack, the
    pairs (i, i + 1) in order, values equal to the recorded ones and to those of the full walk; the public calls take the route."""
    rec, psi = state(name, rbackend)
    L = psi.L
    c1, r1 = rho_mod.device_two_site_rho(psi, 1)
    st = rho_mod.rho_stats
    assert c1.tolist() == [[i, i + 1] for i in range(L - 1)]
    assert st['ring_rows'] == 1 and st['walks'] == 1 and st['d2h'] == 1 and st['transfer_steps'] == 0
    _, rall = rho_mod.device_two_site_rho(psi)
    full = {(i, j): r for (i, j), r in zip([(i, j) for i in range(L) for j in range(i + 1, L)], rall)}
    for (i, j), r in zip(c1.tolist(), r1):
        assert r.shape == rec['rho2'][(i, j)].shape
        assert np.max(np.abs(r - rec['rho2'][(i, j)])) <= 1e-12 and np.max(np.abs(r - full[(i, j)])) <= 1e-12
    rho_mod.reset_stats()
    coords, mi = psi.mutinf_two_site(max_range=1)
    c2, r2 = psi.two_site_rho(1)
    assert rho_mod.rho_stats['generic'] == 0 and rho_mod.rho_stats['device'] == 2
    assert np.array_equal(coords, c1) and np.array_equal(c2, c1) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(r1, r2))
    cg, mg = rho_mod.mutinf_generic(psi, 1)
    assert np.array_equal(cg, c1) and np.max(np.abs(mi - mg)) < 1e-11


@pytest.mark.parametrize("name", ['xxz', 'xxz_tebd'])
def test_small_budget_splits_the_walk(rbackend, monkeypatch, name):
    """``TPA_MEASURE_STACK_GB`` so small that one walk holds two rows: several walks, one copy each, results bit-equal to those of
    the one walk.  The closing kernel sums a slot in an order that depends on neither its position nor the number of slots; the
    products with B_j have fewer stack columns in the split walks, so bit-equality also asks the GEMM for a summation order that does
    not depend on the number of columns.  The device GEMM is under test here.  The emulation's GEMM is the host BLAS, whose complex
    kernels choose their order by the shape: for the complex state on the emulation the walks must agree to 8 u instead -- entries are
    at most 1 and the two orders differ by rounding only.  (Seen there: ten of the 28 pairs differ, all in the two entries
    rho[0, 1, 1, 0] and rho[1, 0, 0, 1] that come from the slot (a, b) = (1, 0) of the charged stack, by 5e-20 to 6.9e-18, the
    largest at the pair (1, 3); the neutral stack's entries and every pair of the real state are bit-equal.)"""
    rec, psi = state(name, rbackend)
    _, one = rho_mod.device_two_site_rho(psi)
    assert rho_mod.rho_stats['walks'] == 1
    per_row = measure._row_bytes(psi, 0, psi.L - 1) * 3             # (three slots per row: d = 2)
    monkeypatch.setenv('TPA_MEASURE_STACK_GB', repr(2.5 * per_row / (1 << 30)))
    monkeypatch.delitem(dev._budget_cache, 'TPA_MEASURE_STACK_GB', raising=False)
    rho_mod.reset_stats()
    try:
        _, split = rho_mod.device_two_site_rho(psi)
    finally:
        dev._budget_cache.pop('TPA_MEASURE_STACK_GB', None)
    st = rho_mod.rho_stats
    assert st['walks'] == 4 and st['d2h'] == st['walks'] and st['ring_rows'] == 2
    for a, b in zip(one, split):
        if rbackend == 'mock' and psi.dtype.kind == 'c':
            assert np.max(np.abs(a - b)) <= 8 * 2.**-53
        else:
            assert np.array_equal(bits(a), bits(b))


def test_switched_off_runs_the_generic_statements(rbackend, monkeypatch):
    rec, psi = state('xxz', rbackend)
    coords, mi = psi.mutinf_two_site(max_range=3)
    monkeypatch.setattr(rho_mod, 'MUTINF', False)
    rho_mod.reset_stats()
    c2, m2 = psi.mutinf_two_site(max_range=3)
    st = rho_mod.rho_stats
    assert st['why'] == {'switched_off': 1} and st['generic'] == 1 and st['device'] == 0 and st['kernel_launches'] == 0
    assert np.array_equal(coords, c2) and np.max(np.abs(mi - m2)) < 1e-11
    assert np.max(np.abs(m2 - rec['mutinf'][(3, 1)][1])) < 1e-11
    _, rg = psi.two_site_rho(2)
    assert st['why'] == {'switched_off': 2} and all(np.max(np.abs(r - rec['rho2'][(i, j)])) < 1e-12
                                                     for (i, j), r in zip([(i, j) for i in range(8) for j in range(i + 1, min(i + 3, 8))], rg))


def test_wide_sector_runs_the_generic_statements(rbackend):
    """A physical sector of five states (no charges): declined with the counted reason; a product state has I = 0 everywhere and a
    pure one-site density matrix."""
    wide = LegCharge.from_trivial(5, ChargeInfo())
    psi = MPS.from_product_state([wide] * 4, [3, 0, 4, 1])
    coords, mi = psi.mutinf_two_site()
    st = rho_mod.rho_stats
    assert st['why'] == {'wide_sector': 1} and st['generic'] == 1 and st['kernel_launches'] == 0
    assert coords.tolist() == [[i, j] for i in range(4) for j in range(i + 1, 4)] and np.max(np.abs(mi)) < 1e-13
    rho1 = psi.one_site_rho()
    assert st['why'] == {'wide_sector': 2} and all(abs(r[o, o] - 1.) < 1e-14 for r, o in zip(rho1, [3, 0, 4, 1]))
    infinite = state('xxz', rbackend)[1].copy()
    infinite.bc = 'infinite'
    assert rho_mod.decline_reason(infinite) == 'infinite'
    lab = state('xxz', rbackend)[1].copy()
    lab._p_label = ['p0']
    assert rho_mod.decline_reason(lab) == 'p_label'
