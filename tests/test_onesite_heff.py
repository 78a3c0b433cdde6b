"""Device ``OneSiteH`` / ``ZeroSiteH`` (factored form: grouped GEMM, block-wise MPO application, grouped GEMM) against the
reference's operators on the environments of a TDVP-evolved state (``tests/golden/tdvp.pkl``, records ``operators``).

Tolerance: ``1e-13 * max|entry|``, the project's block-data tolerance."""
import numpy as np
import pytest

from helpers import load_array
from tdvp_fixtures import build_operator, operator_record, zbackend  # noqa: F401
from tenpy_amd import _lib
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc

MODELS = ['tfi_parity', 'xxz_Sz']
OPS = ['one', 'zero']


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("model", MODELS)
def test_matvec_matches_reference(zbackend, model, op):
    rec = operator_record(model, op)
    H, theta = build_operator(rec)
    assert H.length == {'one': 1, 'zero': 0}[op] and H.acts_on == rec['theta']['labels']
    assert H.N == int(np.prod(rec['theta']['dense'].shape))
    want = rec['matvec']['dense']
    for _ in range(2):              # the second call replays the cached plans
        got = H.matvec(theta)
        assert got.get_leg_labels() == rec['matvec']['labels'] and got.dtype == np.complex128
        err = np.abs(got.to_ndarray() - want).max()
        print(model, op, "max err %.3g, max |entry| %.3g" % (err, np.abs(want).max()))
        assert err <= 1e-13 * np.abs(want).max()
    # a vector with its legs in another order comes back in that order
    perm = list(reversed(H.acts_on))
    got = H.matvec(theta.transpose(perm))
    assert got.get_leg_labels() == perm
    assert np.abs(got.transpose(H.acts_on).to_ndarray() - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("model", MODELS)
def test_to_matrix_times_vector(zbackend, model, op):
    rec = operator_record(model, op)
    H, theta = build_operator(rec)
    M = H.to_matrix()
    vec = theta.combine_legs(H.acts_on, pipes=M.get_leg(0))
    got = npc.tensordot(M, vec, axes=1).to_ndarray()
    want = H.matvec(theta).combine_legs(H.acts_on, pipes=M.get_leg(0)).to_ndarray()
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("model", MODELS)
def test_program_replayed_by_the_native_loop(zbackend, model, op):
    """``matvec_program`` exists for the (all complex) records; one step of ``tpa_lanczos_run`` on it gives
    ``v_1 = (H v_0 - alpha v_0) / beta``, i.e. ``H v_0 = beta v_1 + alpha v_0`` -- the vector ``matvec`` returns."""
    rec = operator_record(model, op)
    H, theta = build_operator(rec)
    got = H.native_input(theta)
    assert got is not None, "complex vector, complex environments: a launch program must exist"
    vec, (ops, bufs, plans) = got
    n = vec._arena.numel()
    L = dev.lib()
    krylov = dev.zeros(2 * n, np.complex128)
    scal = dev.zeros(2 * 3 + 4, np.float64)
    _, scr = dev.reduction_buffers()
    seen = []
    cb = _lib.LANCZOS_CALLBACK(lambda j, alpha, bsq, user: seen.append((alpha, bsq)) or 0)
    ptrs = np.array([t.data_ptr() for t in bufs], dtype=np.int64)
    info = np.zeros(4)
    dev.check(L.tpa_lanczos_run(1, n, ops.ctypes.data, len(ops), ptrs.ctypes.data, len(ptrs), krylov.data_ptr(), vec._arena.data_ptr(),
                                1, 1e-14, 0, 0., scal.data_ptr(), scr.data_ptr(), cb, None, 0, info.ctypes.data, dev.stream()), "lanczos_run")
    assert int(info[0]) == 1 and len(seen) == 1
    alpha, beta = seen[0][0], np.sqrt(seen[0][1])
    K = dev.to_host(krylov)
    hv0 = beta * K[n:] + alpha * K[:n]
    want = H.matvec(vec)
    assert np.array_equal(want._qdata, vec._qdata), "the program's vector is closed under H"
    ref = dev.to_host(want._arena) / info[3]
    assert np.abs(hv0 - ref).max() <= 1e-13 * np.abs(ref).max()
    assert abs(info[3] - npc.norm(theta)) <= 1e-14 * info[3]


def _drop_a_block(A):
    """``A`` without its heaviest stored block (a different block structure on the same legs)."""
    dense = A.to_ndarray().copy()
    slices = [tuple(slice(leg.slices[q], leg.slices[q + 1]) for leg, q in zip(A.legs, row)) for row in A._qdata]
    dense[max(slices, key=lambda sl: np.linalg.norm(dense[sl]))] = 0.
    B = npc.Array.from_ndarray(dense, A.legs, dtype=A.dtype, qtotal=A.qtotal, labels=A.get_leg_labels(), cutoff=0.)
    assert B.stored_blocks == A.stored_blocks - 1
    return B


def _dense_matvec(LP, Ws, RP, theta):
    """numpy contraction LP . theta . W.. . RP with the legs of theta."""
    T = np.tensordot(LP.transpose(['vR*', 'wR', 'vR']).to_ndarray(), theta.to_ndarray(), ([2], [0]))       # a w p.. c
    for k, W in enumerate(Ws):            # W [wL, wR, p, p*] acts on the k-th physical leg
        Wd = W.transpose(['wL', 'wR', 'p', 'p*']).to_ndarray()
        T = np.moveaxis(np.tensordot(Wd, T, ([0, 3], [1, 2 + k])), [0, 1], [1, 2 + k])
    R = RP.transpose(['wL', 'vL', 'vL*']).to_ndarray()
    T = np.moveaxis(T, 1, -2)                                                                                  # a p.. w c
    return np.tensordot(T, R, ([-2, -1], [0, 1]))


@pytest.mark.parametrize("op", ['one', 'zero', 'two'])
@pytest.mark.parametrize("model", MODELS)
def test_stale_plans_are_not_replayed(zbackend, model, op):
    """Plans travel from one visit of a site to the next while the environments grow: an operator that is handed plans made for
    another block structure of ``LP`` (``theta`` unchanged) must notice and plan again."""
    rec = operator_record(model, op)
    H, theta = build_operator(rec)
    first = H.matvec(theta)
    assert H._fplans is not None
    LP, RP = load_array(rec['LP']), load_array(rec['RP'])
    LP2 = _drop_a_block(LP)
    Ws = [load_array(rec[k]) for k in ('W0', 'W1') if k in rec]
    if op == 'two':
        H2 = mps_common.TwoSiteH(None, rec['i0'], tensors=(LP2, RP, Ws[0], Ws[1]), factored=True)
    elif op == 'one':
        H2 = mps_common.OneSiteH.from_LP_W0_RP(LP2, Ws[0], RP)
    else:
        H2 = mps_common.ZeroSiteH.from_LP_RP(LP2, RP)
    H2._fplans = H._fplans
    got = H2.matvec(theta).to_ndarray()
    want = _dense_matvec(LP2, Ws, RP, theta)
    scale = np.abs(first.to_ndarray()).max()
    assert np.abs(want - first.to_ndarray()).max() > 1e-6 * scale, "the dropped block matters"
    assert np.abs(got - want).max() <= 1e-13 * scale


def test_generic_route_without_charges(zbackend):
    """An MPO whose blocks are not single numbers (no conserved charge) has no factored form: the reference's contractions."""
    from tenpy_amd.models.spin_chains import spin_half_leg, tfi_chain_mpo
    from tenpy_amd.networks.mpo import MPOEnvironment
    from tenpy_amd.networks.mps import MPS
    L = 6
    Hm = tfi_chain_mpo(L, 1., 1.5, None)
    _, p = spin_half_leg(None)
    psi = MPS.from_product_state([p] * L, [1] * L, dtype=np.complex128)
    env = MPOEnvironment(psi, Hm)
    H = mps_common.OneSiteH(env, 2)
    assert not H.factored and H.matvec_program(psi.get_theta(2, n=1)) is None
    theta = psi.get_theta(2, n=1)
    got = H.matvec(theta).to_ndarray()
    want = _dense_matvec(H.LP, [Hm.get_W(2)], H.RP, theta)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    with pytest.raises(NotImplementedError):
        mps_common.OneSiteH(env, 2, combine=True)
