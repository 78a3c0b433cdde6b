"""The launch program of the factored two-site matvec without the work nobody reads (``TwoSiteH._skip_program``) against
today's program (``TPA_MATVEC_UNIT=0`` = ``mps_common.MATVEC_SKIP`` off) and against a numpy Lanczos run over the oracle's
``LHeff . theta . RHeff``: on the GPU, and on the emulation of ``mock_device_ex`` (the planner without a GPU).

Tolerances: energies 1e-12, vectors 1e-13 of their largest entry, up to a common sign; on the GPU also bit-equality with
today's program.  Chains of L = 10 at chi <= 32."""
import numpy as np
import pytest

from tenpy_amd.algorithms import mps_common
from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
from tenpy_amd.networks.mpo import mpo_from_dense
from tenpy_amd.networks.mps import MPS

L = 10
N_STEPS = 8
E_TOL, V_TOL = 1e-12, 1e-13


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def ubackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_device_ex
        mock_device_ex.install(monkeypatch)
    else:
        _lib.require_gpu()
    monkeypatch.setattr(mps_common, 'MATVEC_SKIP', True)
    yield request.param
    npc.clear_device_caches()


def long_range_mpo(J3=0.4):
    """The XXZ chain with an extra ``J3 Sz_i Sz_{i+3}``: over two sites the channel of the waiting ``Sz`` moves on without reaching
    ``IdR``, so a block of T3 outside ``IdR`` comes from a block of T1 outside ``IdL``."""
    chinfo, p = spin_half_leg('Sz')
    Sp = np.array([[0., 0.], [1., 0.]])
    Sm, Sz, Id = Sp.T.copy(), np.diag([-0.5, 0.5]), np.eye(2)
    D = 7
    W = np.zeros((D, D, 2, 2))
    W[0, 0] = W[6, 6] = W[3, 4] = W[4, 5] = Id
    W[0, 1], W[0, 2], W[0, 3] = Sp, Sm, Sz
    W[1, 6], W[2, 6], W[3, 6], W[5, 6] = 0.5 * Sm, 0.5 * Sp, Sz, J3 * Sz
    Ws = [W[0:1] if i == 0 else (W[:, D - 1:D] if i == L - 1 else W) for i in range(L)]
    H = mpo_from_dense(Ws, [p] * L, chinfo)
    H.IdL, H.IdR = 0, -1
    return H


def _engine(name, i0):
    """Two sweeps of the stand-alone driver at chi <= 32 (on the route under test), then the right-moving updates of the bonds left of
    ``i0``: the MPS in canonical form around bond ``i0`` with the environments the driver itself hands to that bond.  A new engine
    for every test: its arrays belong to the backend the test installed."""
    H = {'heis': lambda: xxz_chain_mpo(L, 1., 1., 0.), 'field': lambda: xxz_chain_mpo(L, 1., 0.8, 0.3), 'long': long_range_mpo}[name]()
    _, p = spin_half_leg('Sz')
    psi = MPS.from_product_state([p] * L, [1, 0] * (L // 2))
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 32, 'svd_min': 1.e-12}, 'lanczos_params': {}})
    eng.sweep()
    eng.sweep()
    for i in range(i0):
        eng.update_bond(i, move_right=True)
    return eng


def _start(H, eng, i0):
    theta = H.combine_theta(eng.psi.get_theta(i0, n=2))
    rng = np.random.default_rng(100 + i0)
    noise = theta.copy(deep=True)
    noise._arena = dev.to_device(rng.standard_normal(theta._arena.numel()))
    st = theta * (1. / npc.norm(theta)) + noise * (0.5 / npc.norm(noise))
    return st * (1. / npc.norm(st))


def _run(monkeypatch, eng, i0, skip):
    """One forced ``N_STEPS``-step native run on bond ``i0`` -> (E, dense vector [(vL.p0), (p1.vR)], operator, program)."""
    monkeypatch.setattr(mps_common, 'MATVEC_SKIP', skip)
    H = mps_common.TwoSiteH(eng.env, i0, factored=True)
    assert H.factored
    st = _start(H, eng, i0)
    lz = kb.LanczosGroundState(H, st, {'N_min': N_STEPS, 'N_max': N_STEPS})
    prog = lz._native_program()
    assert prog is not None
    E, v, N = lz.run()
    assert N == min(N_STEPS, st._arena.numel())
    return E, H.prepare_svd(v).to_ndarray(), H, prog


def _oracle_lanczos(eng, i0):
    """The same run in numpy over the oracle's matvec."""
    from oracle import npc_oracle as orc

    def to_oracle(arr):
        legs = [orc.OLeg(l.slices, l.charges, l.qconj, arr.chinfo.mod) for l in arr.legs]
        return orc.OTensor(legs, arr.qtotal, arr._qdata, arr._data)
    fus = mps_common.TwoSiteH(eng.env, i0, factored=False)
    fac = mps_common.TwoSiteH(eng.env, i0, factored=True)
    st = fac.prepare_svd(_start(fac, eng, i0))
    Lh, Rh = to_oracle(fus.LHeff), to_oracle(fus.RHeff)

    x0 = st.to_ndarray()
    n_steps = min(N_STEPS, st._arena.numel())
    V, al, be = [x0 / np.linalg.norm(x0)], [], []

    def apply(dense):
        t = npc.Array.from_ndarray(dense, st.legs, labels=st.get_leg_labels(), qtotal=st.qtotal)
        return orc.matvec_two_site(Lh, Rh, to_oracle(t)).to_dense()
    for k in range(n_steps):
        w = apply(V[k])
        al.append(float(np.sum(w * V[k])))
        w = w - al[k] * V[k] - (be[k - 1] * V[k - 1] if k else 0.)
        be.append(float(np.linalg.norm(w)))
        V.append(w / be[k])
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    ev, evec = np.linalg.eigh(T)
    psi = sum(c * v for c, v in zip(evec[:, 0], V))
    return ev[0], psi / np.linalg.norm(psi)


def _same_vector(a, b):
    s = 1. if np.sum(a * b) >= 0 else -1.
    worst = float(np.max(np.abs(a - s * b)))
    print("max |dv| = %.3g (bound %.3g)" % (worst, V_TOL * np.max(np.abs(b))))
    return worst <= V_TOL * np.max(np.abs(b))


@pytest.mark.parametrize("name", ['heis', 'field', 'long'])
@pytest.mark.parametrize("i0", [1, L // 2 - 1, L - 3])
def test_program_against_today_and_oracle(ubackend, monkeypatch, name, i0):
    """Unread blocks of T1 dropped, single-term blocks of T3 read from T1 by scaled links: against today's program and against the
    oracle.  On the device the energy and every entry of the vector are today's bit for bit (the emulation multiplies with numpy,
    whose summation order follows the memory layout of an operand: the tolerances of the module there)."""
    eng = _engine(name, i0)
    before = dict(kb.stats)
    E1, v1, H1, prog1 = _run(monkeypatch, eng, i0, True)
    assert kb.stats['n_skip_taken'] - before['n_skip_taken'] == 1 and kb.stats['n_skip_declined'] == before['n_skip_declined'], kb.skip_declined
    E0, v0, H0, prog0 = _run(monkeypatch, eng, i0, False)
    assert kb.stats['n_skip_taken'] - before['n_skip_taken'] == 1
    kinds1, kinds0 = [int(k) for k in prog1[0][:, 0]], [int(k) for k in prog0[0][:, 0]]
    assert kinds1.count(7) == 1 and 7 not in kinds0 and len(kinds1) <= len(kinds0)
    print("E skip %.15f, today %.15f, diff %.3g" % (E1, E0, E1 - E0))
    if ubackend == 'gpu':
        assert E1 == E0 and np.array_equal(v1, v0)
    assert abs(E1 - E0) <= E_TOL and _same_vector(v1, v0)
    Eo, vo = _oracle_lanczos(eng, i0)
    assert abs(E1 - Eo) <= E_TOL and abs(E0 - Eo) <= E_TOL
    assert _same_vector(v1, vo) and _same_vector(v0, vo)
    # step 1 runs the tiles of the blocks of T1 that are read (the S+ / S- blocks that no term reads are not computed), on the kernel
    # the full launch runs on; the timers count the launches that are made
    p1, p2 = H1._fplans['p1'], H1._fplans['p2']
    full = p1.n_tiles if p1.sk is None else p1.sk.n_tiles
    assert kinds1[0] == 0 and prog1[0][0, 5] < full
    kernel = dev.lib().tpa_gemm_kernel_id
    assert kernel(0, p1.cfg, int(prog1[0][0, 5])) == kernel(0, p1.cfg, full)
    assert sum(p.flops for p in prog1[2]) < sum(p.flops for p in prog0[2]) and prog1[2][1] is p2
    assert H1.flops_per_matvec == sum(p.flops for p in prog1[2]) < H0.flops_per_matvec
    # step 2 keeps the tile table of p2 and mixes scaled links on T1 with plain links on the blocks of T3 that are written
    row = prog1[0][kinds1.index(7)]
    assert row[4] == (p2.tiles_dev if p2.sk is None else p2.sk.tiles_dev).data_ptr() and row[9] == 2
    links = dev.to_host(mps_common._skip_table_cache[(id(p1), id(H1._fplans['a01']), id(p2))][3]['c_links'])
    assert np.any((links[:, 7] >> 16) != 0) and np.any((links[:, 7] >> 16) == 0)
    assert kinds1.count(1) >= 1, "the blocks of T3 with several terms are written by the MPO step"


def test_product_state_has_no_program_either_way(ubackend, monkeypatch):
    _, p = spin_half_leg('Sz')
    H = xxz_chain_mpo(L, 1., 1., 0.)
    psi = MPS.from_product_state([p] * L, [1, 0] * (L // 2))
    eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 32, 'svd_min': 1.e-12}, 'lanczos_params': {}})
    for skip in (True, False):
        monkeypatch.setattr(mps_common, 'MATVEC_SKIP', skip)
        op = mps_common.TwoSiteH(eng.env, L // 2 - 1, factored=True)
        theta = op.combine_theta(psi.get_theta(L // 2 - 1, n=2))
        before = dict(kb.stats)
        assert op.matvec_program(theta) is None
        assert kb.stats['n_skip_taken'] == before['n_skip_taken']


def test_explicit_tensors_keep_todays_program(ubackend, monkeypatch):
    """Operators built from explicit tensors (tests, replayed bonds, the doubled operator of ``PlusHcH``): declined, counted."""
    eng = _engine('heis', L // 2 - 1)
    i0 = L // 2 - 1
    op = mps_common.TwoSiteH(None, i0, tensors=(eng.env.get_LP(i0), eng.env.get_RP(i0 + 1), eng.H.get_W(i0), eng.H.get_W(i0 + 1)), factored=True)
    before = kb.skip_declined.get('operator', 0)
    got = op.native_input(_start(op, eng, i0))
    assert got is not None and 7 not in [int(k) for k in got[1][0][:, 0]]
    assert kb.skip_declined.get('operator', 0) > before


def test_block_mpo_keeps_its_program(ubackend, monkeypatch):
    """The Hubbard ladder with an N-only leg (``MpoBlockApplyPlan``): declined with the counter set, the kind-5 program as before."""
    from mpo_apply_fixtures import ladder_engine
    if ubackend == 'mock':      # the emulation that has tpa_mpo_apply_batch, with the entry point this route asks for on top
        import mock_device_ex
        import mock_mpo_apply
        npc.clear_device_caches()
        mock = mock_mpo_apply.install(monkeypatch)
        mock.tpa_gemm_chain_ex = mock_device_ex.MockLibEx().tpa_gemm_chain_ex
    assert dev.lib_provides('tpa_mpo_apply_batch') and dev.lib_provides('tpa_gemm_chain_ex')
    eng = ladder_engine(2, False)
    i0 = eng.psi.L // 2 - 1
    op = mps_common.TwoSiteH(eng.env, i0, factored=True)
    theta = op.combine_theta(eng.psi.get_theta(i0, n=2))
    before = dict(kb.stats)
    got = op.native_input(theta)
    assert got is not None
    kinds = [int(k) for k in got[1][0][:, 0]]
    assert 5 in kinds and 7 not in kinds
    assert kb.stats['n_skip_declined'] > before['n_skip_declined'] and kb.skip_declined.get('mpo_plan', 0) > 0
