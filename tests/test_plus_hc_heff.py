"""``H + h.c.`` on the device: for MPOs built with ``explicit_plus_hc=True`` the effective Hamiltonians ``H_eff + H_eff^dagger`` as ONE
operator on the direct sum along the MPO bond (``mps_common.PlusHcH``, ``plus_hc()`` of ``TwoSiteH`` / ``OneSiteH`` / ``ZeroSiteH``).

Cases (``plus_hc_fixtures``), all on L = 8 chains after two warm-up sweeps at chi <= 24: XXZ with Sz (real, scalar MPO blocks), Hubbard
with (N, 2Sz) and a Peierls phase (complex ``W`` that is not Hermitian), Hubbard with N only (``MpoBlockApplyPlan``, real and complex),
and the XXZ and Hubbard MPOs with sorted and bunched bond legs (wide ``w`` blocks, ``MpoEntryApplyPlan``, environments stored in an
order that the factored form has to copy from).  Tolerance of the operator comparisons: ``1e-13 * max(1, max |entry|)``, the bound of
``tests/test_heff.py`` for the factored form; of the Lanczos comparisons: ``1e-12 * max(1, |E0|)`` (``tests/test_lanczos_native.py``);
of DMRG energies: ``1e-10`` relative (``tests/test_dmrg_golden.py``).  Every test runs on the numpy emulation and, marked ``gpu``, on
the device.  None of them passes without ``plus_hc``."""
import numpy as np
import pytest

from plus_hc_fixtures import (CASES, dense_plus_hc, ebackend, exact_ground_energy, initial_state, make_mpo, model_state,  # noqa: F401
                              nonsquare_bond, operator_and_vector)
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.sparse import OrthogonalNpcLinearOperator, SumNpcLinearOperator
from tenpy_amd.networks.mpo import MPOEnvironment

PLAN = {'xxz': mps_common.MpoApplyPlan, 'hubbard': mps_common.MpoApplyPlan, 'hubbardN_real': mps_common.MpoBlockApplyPlan,
        'hubbardN': mps_common.MpoBlockApplyPlan, 'xxz_sorted': mps_common.MpoEntryApplyPlan,
        'hubbard_sorted': mps_common.MpoEntryApplyPlan}


def _close(got, want, what):
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("%s: max err %.3g, max |entry| %.3g" % (what, err, scale))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * max(1., scale), err_msg=what)       # (tests/test_heff.py)


def _site(i0, n):
    return i0 + 1 if n == 0 else i0         # the zero-site operator sits on the bond between the two sites


def _Ws(op):
    return [W for W in (getattr(op, 'W0', None), getattr(op, 'W1', None)) if W is not None]


@pytest.mark.parametrize("name", CASES)
def test_inputs(ebackend, name):
    """What the cases rest on: the MPO is half of H (complex cases: not Hermitian), its doubled tensor takes the plan class of the
    plain one, the tested bond has a non-square block of LP, and the doubled tensors are what their definition says."""
    H, psi, env = model_state(ebackend, name)
    assert H.explicit_plus_hc is True
    i0 = nonsquare_bond(psi, env)
    W = H.get_W(i0)
    Wd = mps_common._plus_hc_W(W)
    assert Wd is mps_common._plus_hc_W(W), "built once per MPO tensor"
    assert mps_common._mpo_plan_class(W) is mps_common._mpo_plan_class(Wd) is PLAN[name]
    if name in ('hubbard', 'hubbardN', 'hubbard_sorted'):
        assert H.dtype == np.complex128
        full = make_mpo(name, False)[0].get_W(i0)
        assert full.get_leg('wL').ind_len > W.get_leg('wL').ind_len
    D, Dd = W.to_ndarray(), Wd.to_ndarray()
    a, b = D.shape[:2]
    assert np.array_equal(Dd[:a, :b], D) and np.array_equal(Dd[a:, b:], D.conj().transpose(0, 1, 3, 2))
    assert not Dd[:a, b:].any() and not Dd[a:, :b].any()
    for left, A in ((True, env.get_LP(i0)), (False, env.get_RP(i0 + 1))):
        w, order = ('wR', ['vR*', 'wR', 'vR']) if left else ('wL', ['wL', 'vL', 'vL*'])
        dense = A.transpose(order).to_ndarray()
        ax = order.index(w)
        other = [k for k in range(3) if k != ax]
        want_adj = np.swapaxes(dense.conj(), *other)
        adj = mps_common._adjoint_env(A, left)
        assert list(adj.get_leg_labels()) == list(A.get_leg_labels())
        assert np.array_equal(adj.transpose(order).to_ndarray(), want_adj)
        cache = {}
        both = mps_common._plus_hc_env(A, left, cache, 3)
        assert list(both.get_leg_labels()) == order and mps_common._plus_hc_env(A, left, cache, 3) is both
        assert np.array_equal(both.to_ndarray(), np.concatenate([dense, want_adj], axis=ax))
        both.test_sanity()


@pytest.mark.parametrize("n", [2, 1, 0])
@pytest.mark.parametrize("name", CASES)
def test_operator_parity(ebackend, name, n):
    """``plus_hc().matvec(theta)`` against the dense contraction ``H theta + H^dagger theta`` of the plain tensors on the host and
    against ``SumNpcLinearOperator`` over the generic route; everything else is answered from the plain operator."""
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    op, theta = operator_and_vector(psi, env, _site(i0, n), n)
    sh = op.LP._block_shapes()
    assert np.any(sh[:, op.LP.get_leg_index('vR*')] != sh[:, op.LP.get_leg_index('vR')]) or n == 0
    assert op.factored is True
    both = op.plus_hc()
    assert isinstance(both, mps_common.PlusHcH), "plus_hc declined"
    got = both.matvec(theta)
    assert list(got.get_leg_labels()) == list(theta.get_leg_labels())
    want = dense_plus_hc(op.LP, _Ws(op), op.RP, theta)
    _close(got.to_ndarray(), want, "%s, %d sites: doubled operator vs dense H + H^dagger" % (name, n))
    generic = SumNpcLinearOperator(op, op.adjoint()).matvec(theta)
    _close(generic.to_ndarray(), want, "%s, %d sites: generic sum vs dense" % (name, n))
    _close(got.to_ndarray(), generic.to_ndarray(), "%s, %d sites: doubled operator vs generic sum" % (name, n))
    if name in ('hubbard', 'hubbardN', 'hubbard_sorted'):          # the halves differ: H_eff alone is not Hermitian here
        assert np.abs(op.matvec(theta).to_ndarray() * 2 - want).max() > 1e-3 * np.abs(want).max()
    assert both.adjoint() is both and both.LP is op.LP and both.RP is op.RP and both.i0 == op.i0 and both.length == n
    assert both.acts_on == op.acts_on and both.combine == op.combine and both.move_right == op.move_right
    if n == 2:
        assert both.W0 is op.W0 and both.W1 is op.W1 and both.pipeL is op.pipeL and both.pipeR is op.pipeR
        assert both.LHeff is op.LHeff and both.RHeff is op.RHeff
        m = op.to_matrix()
        assert np.array_equal(both.to_matrix(), m + m.conj().T)
    else:
        m = op.to_matrix().to_ndarray()
        np.testing.assert_allclose(both.to_matrix().to_ndarray(), m + m.conj().T, rtol=0, atol=1e-15 * np.abs(m).max())


@pytest.mark.parametrize("name", ['xxz', 'hubbard'])
def test_fused_mode(ebackend, name):
    """The doubled operator of a plain operator in the ``LHeff . theta . RHeff`` form (the default below ``FACTORED_MIN_SECTOR``)."""
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    op = mps_common.TwoSiteH(env, i0, factored=False)
    both = op.plus_hc()
    assert isinstance(both, mps_common.PlusHcH) and both.doubled.factored is False
    theta = op.combine_theta(psi.get_theta(i0, n=2))
    assert theta.rank == 2
    fac, th4 = operator_and_vector(psi, env, i0, 2)
    want = fac.prepare_svd(npc.Array.from_ndarray(dense_plus_hc(fac.LP, _Ws(fac), fac.RP, th4), th4.legs, labels=th4.get_leg_labels()))
    _close(both.matvec(theta).to_ndarray(), want.to_ndarray(), name + ": fused doubled operator vs dense")
    got = both.native_input(theta)
    assert got is not None and len(got[1][0]) == len(op.native_input(theta)[1][0]) == 2


@pytest.mark.parametrize("n", [2, 1, 0])
@pytest.mark.parametrize("name", CASES)
def test_one_program_three_launches(ebackend, name, n):
    """The doubled operator offers a launch program with exactly as many ops as the plain operator's for the same theta (GEMM, MPO
    pass, GEMM -- two GEMMs without a site), on the vector as it is: after the warm-up sweeps the block structure is closed under H."""
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    op, theta = operator_and_vector(psi, env, _site(i0, n), n)
    both = op.plus_hc()
    plain, doubled = op.native_input(theta), both.native_input(theta)
    assert plain is not None and doubled is not None
    # Nothing of H + H^dagger is skipped: the program runs on theta itself where its block structure is closed under the operator (XXZ,
    # two sites), and else on theta embedded with zero blocks in the structure of the result (`native_input`; measured on the emulation:
    # after two sweeps at chi <= 24 the truncated Hubbard vectors of the middle bonds lack 2 - 24 of the blocks that H + H^dagger
    # reaches, and H + H^dagger fills more of them than the half H alone) -- the same vector either way.
    assert np.array_equal(doubled[0].to_ndarray(), theta.to_ndarray())
    if name.startswith('xxz') and n == 2:
        assert plain[0] is theta and doubled[0] is theta
    ops_p, ops_d = plain[1][0], doubled[1][0]
    assert len(ops_d) == len(ops_p) == (3 if n else 2)
    assert [int(k) for k in ops_d[:, 0]] == [int(k) for k in ops_p[:, 0]]
    assert both.matvec_program(doubled[0]) is doubled[1]
    both.matvec(theta)
    if n == 2:
        assert both.flops_per_matvec == both.doubled.flops_per_matvec > op.flops_per_matvec
        assert both.bytes_per_matvec == both.doubled.bytes_per_matvec > op.bytes_per_matvec


def _lanczos_both_routes(monkeypatch, make, theta):
    """(E0, N) of the native run on the doubled operator and of the step-by-step loop on the routing without it (``PLUS_HC`` off)."""
    res = {}
    for on in (True, False):
        monkeypatch.setattr(mps_common, 'PLUS_HC', on)
        monkeypatch.setattr(kb, 'NATIVE', on)
        eff = make()
        lz = kb.LanczosGroundState(eff, theta, {'N_min': 4, 'N_max': 12})
        if on:
            assert lz._native_program() is not None
        E, v, N = lz.run()
        res[on] = (E, N, v)
    (E1, N1, v1), (E0, N0, v0) = res[True], res[False]
    print("native doubled: E0 = %.15g, N = %d; step by step: E0 = %.15g, N = %d" % (E1, N1, E0, N0))
    assert N1 == N0
    assert abs(E1 - E0) <= 1e-12 * max(1., abs(E0))        # (tests/test_lanczos_native.py)
    return v1


@pytest.mark.parametrize("name", CASES)
def test_native_lanczos(ebackend, monkeypatch, name):
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    from tenpy_amd.algorithms.dmrg import _plus_hc
    theta = operator_and_vector(psi, env, i0, 2)[1]
    made = []

    def make():
        made.append(_plus_hc(mps_common.TwoSiteH(env, i0, factored=True)))
        return made[-1]
    _lanczos_both_routes(monkeypatch, make, theta)
    assert isinstance(made[0], mps_common.PlusHcH) and isinstance(made[1], SumNpcLinearOperator)


@pytest.mark.parametrize("name", ['xxz', 'hubbard', 'hubbardN', 'hubbard_sorted'])
def test_native_lanczos_orthogonal(ebackend, monkeypatch, name):
    """The same with an ``OrthogonalNpcLinearOperator`` around the operator, one vector to stay orthogonal to."""
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    from tenpy_amd.algorithms.dmrg import _plus_hc
    op, theta = operator_and_vector(psi, env, i0, 2)
    ortho = op.plus_hc().matvec(theta)                     # a vector with the block structure of theta
    before = kb.stats['n_native_ortho']
    _lanczos_both_routes(monkeypatch, lambda: OrthogonalNpcLinearOperator(_plus_hc(mps_common.TwoSiteH(env, i0, factored=True)), [ortho]),
                             theta)
    assert kb.stats['n_native_ortho'] > before


@pytest.mark.parametrize("name", ['xxz', 'hubbard', 'hubbardN'])
def test_half_mpo_equals_full_mpo(ebackend, name):
    """Two ways to build the same model: ``H_half theta + H_half^dagger theta`` equals ``H_full theta``."""
    H, psi, env = model_state(ebackend, name)
    i0 = nonsquare_bond(psi, env)
    env_full = MPOEnvironment(psi, make_mpo(name, False)[0])
    for n in (2, 1, 0):
        op, theta = operator_and_vector(psi, env, _site(i0, n), n)
        full, _ = operator_and_vector(psi, env_full, _site(i0, n), n)
        _close(op.plus_hc().matvec(theta).to_ndarray(), full.matvec(theta).to_ndarray(), "%s, %d sites: half MPO + h.c. vs full MPO" % (name, n))


@pytest.mark.parametrize("name,n", [('xxz', 8), ('hubbard', 4)])
def test_dmrg_reaches_exact_energy(ebackend, name, n):
    """Stand-alone DMRG at chi = 16 on the half MPO and on the full MPO of the same model against an exact diagonalisation that is
    numpy alone.  XXZ: L = 8; the Peierls ladder: 2 x 2 sites, the size at which chi = 16 holds the exact state."""
    from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
    exact = exact_ground_energy(name, n)
    for plus_hc in (True, False):
        H, p = make_mpo(name, plus_hc, n)
        psi = initial_state(name, p, n)
        eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 16, 'svd_min': 1.e-10}, 'lanczos_params': {}})
        for _ in range(4):
            eng.sweep()
        E = eng.sweep_stats['E'][-1]
        print("%s, explicit_plus_hc=%s: E = %.14f, exact %.14f; <H> = %.14f" % (name, plus_hc, E, exact, np.real(eng.env.full_contraction(n // 2 - 1))))
        assert abs(E - exact) <= 1e-10 * abs(exact)          # (tests/test_dmrg_golden.py)
        assert abs(eng.env.full_contraction(n // 2 - 1) - exact) <= 1e-10 * abs(exact)


# ---- declines: the old route, the same numbers ----------------------------------------------------------------------------------------
def test_declines(ebackend, monkeypatch):
    H, psi, env = model_state(ebackend, 'hubbard')
    i0 = nonsquare_bond(psi, env)
    op, theta = operator_and_vector(psi, env, i0, 2)
    want = op.plus_hc().matvec(theta).to_ndarray()
    from tenpy_amd.algorithms.dmrg import _plus_hc
    from tenpy_amd.algorithms.sharded import ShardedTwoSiteH

    class OtherBra:                         # an environment <bra| H |ket> of two different states
        def __init__(self, env):
            self.H, self.ket, self.bra = env.H, env.ket, object()
    op._env = OtherBra(env)
    assert op.plus_hc() is None
    route = _plus_hc(op)
    assert isinstance(route, SumNpcLinearOperator) and route.native_input(theta) is None
    _close(route.matvec(theta).to_ndarray(), want, "bra is not ket: the sum of the operator and its generic adjoint")
    op._env = env
    assert ShardedTwoSiteH.plus_hc(op) is None, "a sharded operator keeps today's route"
    monkeypatch.setattr(mps_common, 'PLUS_HC', False)
    assert op.plus_hc() is None
    for n in (1, 0):
        o, th = operator_and_vector(psi, env, _site(i0, n), n)
        assert o.plus_hc() is None
        monkeypatch.setattr(mps_common, 'PLUS_HC', True)
        w = o.plus_hc().matvec(th).to_ndarray()
        monkeypatch.setattr(mps_common, 'PLUS_HC', False)
        _close(_plus_hc(o).matvec(th).to_ndarray(), w, "switch off, %d sites" % n)
    _close(_plus_hc(op).matvec(theta).to_ndarray(), want, "switch off, two sites")
    charged = mps_common.TwoSiteH(None, i0, tensors=(op.LP, op.RP, H.get_W(i0), H.get_W(i0 + 1)), factored=True)
    monkeypatch.setattr(mps_common, 'PLUS_HC', True)
    assert charged.plus_hc() is not None
    real_env = op.RP.astype(np.complex128) if op.RP.dtype != np.complex128 else None
    assert real_env is None             # (complex case: both environments complex)
    Hx, psix, envx = model_state(ebackend, 'xxz')
    ox = mps_common.TwoSiteH(None, 3, tensors=(envx.get_LP(3), envx.get_RP(4).astype(np.complex128), Hx.get_W(3), Hx.get_W(4)), factored=True)
    assert ox.plus_hc() is None, "mixed dtypes"


def test_switch_off_same_sweep_energies(ebackend, monkeypatch):
    """``TPA_PLUS_HC=0`` (``mps_common.PLUS_HC``): two sweeps of the stand-alone driver on the old route give the same energies."""
    from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
    E = {}
    for on in (True, False):
        monkeypatch.setattr(mps_common, 'PLUS_HC', on)
        H, p = make_mpo('hubbard', True, 6)
        eng = TwoSiteDMRGEngine(initial_state('hubbard', p, 6), H, {'trunc_params': {'chi_max': 16, 'svd_min': 1.e-10}, 'lanczos_params': {}})
        for _ in range(2):
            eng.sweep()
        E[on] = list(eng.update_stats['E_total'])
    assert np.abs(np.array(E[True]) - np.array(E[False])).max() <= 1e-10 * abs(E[False][-1])
