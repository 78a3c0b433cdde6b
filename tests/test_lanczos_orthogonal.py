"""Lanczos with ``orthogonal_to`` and with ``reortho`` through the native loop (``tpa_lanczos_run_ex``: the projections of
``OrthogonalNpcLinearOperator`` as op kind 4, the re-orthogonalisation as flag bit 0; both on ``tpa_project_out``) against the
step-by-step Python loop over ``OrthogonalNpcLinearOperator.matvec`` (the unchanged route: ``kb.NATIVE`` off), against the definition
(dense ``Q^H H Q`` with numpy), the decline conditions, and the promise that a run with neither option makes the calls it always made.

The start vector of every comparison is projected on the complement of the ``ortho_vecs`` first (the Ritz vector of a start vector
with a component along them keeps part of it, on either route)."""
import numpy as np
import pytest

from ortho_fixtures import inner, obackend, random_like  # noqa: F401
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.sparse import OrthogonalNpcLinearOperator
from test_heff import _engine

OPTIONS = {'forced8': {'N_min': 8, 'N_max': 8}, 'shift': {'E_shift': -3.5, 'N_max': 12}, 'default': {}}


def _operator(eng, i0, factored, cplx=False):
    tensors = [eng.env.get_LP(i0), eng.env.get_RP(i0 + 1), eng.H.get_W(i0), eng.H.get_W(i0 + 1)]
    if cplx:
        tensors = [t.astype(np.complex128) for t in tensors]
    H = mps_common.TwoSiteH(None, i0, tensors=tuple(tensors), factored=factored)
    theta = H.combine_theta(eng.psi.get_theta(i0, n=2))
    if cplx:
        theta = theta.astype(np.complex128) * np.exp(0.3j)
    return H, theta


def _wrapped(H, ortho):
    return OrthogonalNpcLinearOperator(H, [o.copy(deep=True) for o in ortho])       # (gram_schmidt works in place)


def _start(Ho, theta, rng):
    """The start vector of ``test_lanczos_evolution_native._two_site`` -- the state plus half its norm of noise: the DMRG state itself
    is (nearly) an eigenvector, a one-dimensional Krylov space up to rounding -- projected on the complement of the ``ortho_vecs``."""
    noise = random_like(theta, rng)
    st = theta * (1. / npc.norm(theta)) + noise * (0.5 / npc.norm(noise))
    for o in Ho.ortho_vecs:
        st.iadd_prefactor_other(-inner(o, st), o)
    return st * (1. / npc.norm(st))


def _both_routes(monkeypatch, H, theta, ortho, options, seed):
    """-> {native: (E0, psi, N)}; asserts the counters and the orthogonality of the results on the way."""
    res = {}
    for native in (True, False):
        monkeypatch.setattr(kb, 'NATIVE', native)
        Ho = _wrapped(H, ortho)
        st = _start(Ho, theta, np.random.default_rng(seed))
        before = dict(kb.stats)
        res[native] = kb.LanczosGroundState(Ho, st, dict(options)).run()
        assert kb.stats['n_native_ortho'] - before['n_native_ortho'] == int(native)
        assert kb.stats['n_ortho_declined'] == before['n_ortho_declined']
        for o in Ho.ortho_vecs:
            assert abs(inner(o, res[native][1])) <= 1e-12
    return res


def _compare(res, exact_N):
    (E1, v1, N1), (E0, v0, N0) = res[True], res[False]
    if exact_N:
        assert N1 == N0
    else:
        assert abs(N1 - N0) <= 1          # the two routes round the projection differently
    assert abs(E1 - E0) <= 1e-12 * max(1., abs(E0))
    if exact_N:
        assert v1.get_leg_labels() == v0.get_leg_labels()
        assert abs(inner(v0, v1) - 1.) <= 1e-10


@pytest.mark.parametrize("model", ['xxz', 'hubbard'])
@pytest.mark.parametrize("factored", [False, True], ids=['fused', 'factored'])
@pytest.mark.parametrize("opt", ['forced8', 'shift', 'default'])
def test_native_equals_stepwise(obackend, monkeypatch, model, factored, opt):
    eng = _engine(model)
    L = eng.psi.L
    for i0 in (1, L // 2 - 1, L - 3):
        H, theta = _operator(eng, i0, factored)
        assert H.factored == factored
        for m in (1, 3):
            rng = np.random.default_rng([i0, m])
            ortho = [random_like(theta, rng) for _ in range(m)]
            _compare(_both_routes(monkeypatch, H, theta, ortho, OPTIONS[opt], seed=7 * i0 + m), exact_N=(opt != 'default'))


@pytest.mark.parametrize("factored", [False, True], ids=['fused', 'factored'])
@pytest.mark.parametrize("opt", ['forced8', 'shift', 'default'])
def test_native_equals_stepwise_complex(obackend, monkeypatch, factored, opt):
    eng = _engine('xxz')
    L = eng.psi.L
    for i0 in (1, L // 2 - 1, L - 3):
        H, theta = _operator(eng, i0, factored, cplx=True)
        assert H.factored == factored
        for m in (1, 3):
            rng = np.random.default_rng([i0, m, 1])
            ortho = [random_like(theta, rng) for _ in range(m)]
            _compare(_both_routes(monkeypatch, H, theta, ortho, OPTIONS[opt], seed=11 * i0 + m), exact_N=(opt != 'default'))


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize("m", [1, 3])
def test_against_the_definition(obackend, monkeypatch, cplx, m):
    """Independent of both routes: lowest eigenvalue of Q^H H Q, Q an orthonormal complement of the o_j, with the dense H from n
    matvecs on unit vectors (i0 = 1: n is tens of elements); Lanczos with N_max = n exhausts the space."""
    eng = _engine('xxz')
    H, theta = _operator(eng, 1, False, cplx)
    vec = H.native_input(theta)[0]
    n = vec._arena.numel()
    assert 8 <= n <= 60
    dense = np.zeros((n, n), dtype=vec.dtype)
    for i in range(n):
        e = vec.copy(deep=True)
        unit = np.zeros(n, dtype=vec.dtype)
        unit[i] = 1.
        e._arena = dev.to_device(unit)
        col = H.matvec(e)
        assert col._same_structure(vec)
        dense[:, i] = dev.to_host(col._arena)[:n]
    assert np.allclose(dense, dense.conj().T, atol=1e-12)
    rng = np.random.default_rng([3, m, int(cplx)])
    ortho = [random_like(vec, rng) for _ in range(m)]
    O = np.stack([dev.to_host(o._arena)[:n] for o in ortho], axis=1)
    Q = np.linalg.qr(O, mode='complete')[0][:, m:]
    E_def = np.linalg.eigvalsh(Q.conj().T @ dense @ Q)[0]
    monkeypatch.setattr(kb, 'NATIVE', True)
    Ho = _wrapped(H, ortho)
    before = kb.stats['n_native_ortho']
    E0, psi, N = kb.LanczosGroundState(Ho, _start(Ho, vec, rng), {'N_max': n, 'N_min': 2, 'P_tol': 1e-28}).run()
    assert kb.stats['n_native_ortho'] == before + 1
    print("PROJECTED LANCZOS vs definition: n=%d m=%d N=%d |dE|=%.3e" % (n, m, N, abs(E0 - E_def)))
    assert abs(E0 - E_def) <= 1e-10 * max(1., abs(E_def))


class _NarrowProgram:
    """An operator that offers its launch program together with a vector that lacks a block (what ``native_input`` of a device
    operator returns is the wrapped operator's business; the wrapper has to look at the structure it gets).  The program is never
    run: the wrapper declines."""

    def __init__(self, H, narrow):
        self.H, self.narrow = H, narrow

    def matvec(self, v):
        return self.H.matvec(v)

    def native_input(self, theta):
        return self.narrow, self.H.native_input(theta)[1]


def _definition_energy(Ho, st, options):
    """The step-by-step route: Lanczos over ``matvec`` as it is defined."""
    native = kb.NATIVE
    kb.NATIVE = False
    try:
        return kb.LanczosGroundState(Ho, st.copy(deep=True), dict(options)).run()
    finally:
        kb.NATIVE = native


def test_declines(obackend, monkeypatch):
    monkeypatch.setattr(kb, 'NATIVE', True)
    eng = _engine('xxz')
    i0 = eng.psi.L // 2 - 1
    opts = {'N_min': 8, 'N_max': 8}
    # (a) an ortho_vec with a block that the structure handed over lacks
    H, theta = _operator(eng, i0, False)
    vec = H.native_input(theta)[0]
    assert vec.stored_blocks > theta.stored_blocks, "this bond's theta lacks a block of H theta"
    rng = np.random.default_rng(23)
    ortho = [random_like(vec, rng)]
    Ho = _wrapped(_NarrowProgram(H, theta), ortho)
    st = _start(Ho, vec, rng)
    before = dict(kb.stats)
    E0, psi, N = kb.LanczosGroundState(Ho, st.copy(deep=True), opts).run()
    assert kb.stats['n_ortho_declined'] == before['n_ortho_declined'] + 1 and kb.stats['n_native_ortho'] == before['n_native_ortho']
    E_ref, psi_ref, N_ref = _definition_energy(Ho, st, opts)
    assert N == N_ref and abs(E0 - E_ref) <= 1e-12 * max(1., abs(E_ref)) and abs(inner(psi_ref, psi) - 1.) <= 1e-10
    # (b) a complex ortho_vec on a real operator
    ortho = [random_like(theta, rng, cplx=True)]
    Ho = _wrapped(H, ortho)
    st = random_like(theta, rng)
    before = dict(kb.stats)
    E0, psi, N = kb.LanczosGroundState(Ho, st.copy(deep=True), opts).run()
    assert kb.stats['n_ortho_declined'] == before['n_ortho_declined'] + 1 and kb.stats['n_native_ortho'] == before['n_native_ortho']
    E_ref, psi_ref, N_ref = _definition_energy(Ho, st, opts)
    assert N == N_ref and abs(E0 - E_ref) <= 1e-12 * max(1., abs(E_ref)) and abs(inner(psi_ref, psi) - 1.) <= 1e-10
    # (c) another leg order
    Hf, theta_f = _operator(eng, i0, True)
    o = random_like(theta_f, rng)
    o = o.transpose(['vR', 'p1', 'p0', 'vL'])
    Ho = _wrapped(Hf, [o])
    before = dict(kb.stats)
    assert Ho.native_input(theta_f) is None
    assert kb.stats['n_ortho_declined'] == before['n_ortho_declined'] + 1


def _gram_defect(lz, prog):
    N, n, krylov, _ = lz._native_krylov(prog)
    V = dev.to_host(krylov)[:N * n].reshape(N, n)
    return N, float(np.max(np.abs(V.conj() @ V.T - np.eye(N))))


@pytest.mark.parametrize("model,cplx", [('xxz', False), ('xxz', True), ('hubbard', False)])
@pytest.mark.parametrize("factored", [False, True], ids=['fused', 'factored'])
@pytest.mark.parametrize("opt", ['forced12', 'default'])
def test_reortho_native(obackend, monkeypatch, model, cplx, factored, opt):
    options = {'forced12': {'reortho': True, 'N_min': 12, 'N_max': 12}, 'default': {'reortho': True}}[opt]
    eng = _engine(model)
    L = eng.psi.L
    for i0 in (1, L // 2 - 1, L - 3):
        H, theta = _operator(eng, i0, factored, cplx)
        assert H.factored == factored
        st = random_like(theta, np.random.default_rng([i0, 5]))
        st = st * (1. / npc.norm(st))
        res = {}
        for native in (True, False):
            monkeypatch.setattr(kb, 'NATIVE', native)
            before = kb.stats['n_native_reortho']
            res[native] = kb.LanczosGroundState(H, st.copy(deep=True), dict(options)).run()
            assert kb.stats['n_native_reortho'] - before == int(native)
        _compare(res, exact_N=(opt != 'default'))
        monkeypatch.setattr(kb, 'NATIVE', True)
        defect = {}
        for reortho in (True, False):
            lz = kb.LanczosGroundState(H, st.copy(deep=True), dict(options, reortho=reortho))
            N, defect[reortho] = _gram_defect(lz, lz._native_program())
        print("KRYLOV GRAM %s %s i0=%d N=%d: max |V^H V - 1| = %.3e with reortho, %.3e without"
              % (model, 'complex' if cplx else 'real', i0, N, defect[True], defect[False]))
        assert defect[True] <= 1e-12


def test_reortho_evolution(obackend, monkeypatch):
    """Pins the fallback, nothing more: ``LanczosEvolution`` keeps the step-by-step route for ``reortho``
    (tests/test_lanczos_evolution_native.py::test_fallback_routes requires it), so both settings of ``kb.NATIVE`` run the same Python
    loop here -- no native run is counted, and this case cannot fail for an error of the kernel or of the native loop."""
    eng = _engine('xxz')
    H, theta = _operator(eng, eng.psi.L // 2 - 1, True, cplx=True)
    st = random_like(theta, np.random.default_rng(31))
    res = {}
    for native in (True, False):
        monkeypatch.setattr(kb, 'NATIVE', native)
        before = dict(kb.stats)
        res[native] = kb.LanczosEvolution(H, st.copy(deep=True), {'reortho': True, 'N_min': 10, 'N_max': 10}).run(-0.05j)
        assert kb.stats['n_native_reortho'] == before['n_native_reortho'] and kb.stats['n_native_evolve'] == before['n_native_evolve']
    (p1, N1), (p0, N0) = res[True], res[False]
    assert N1 == N0
    assert npc.norm(p1 - p0) <= 1e-12 * npc.norm(p0)


def test_other_wrappers_offer_no_program(obackend, monkeypatch):
    """A wrapper changes the matvec, so the wrapped operator's launch program is not its own: ``ShiftNpcLinearOperator`` around a
    device ``TwoSiteH`` takes the step-by-step route and returns E0 + shift with ``kb.NATIVE`` on."""
    from tenpy_amd.linalg.sparse import ShiftNpcLinearOperator
    monkeypatch.setattr(kb, 'NATIVE', True)
    eng = _engine('xxz')
    H, theta = _operator(eng, eng.psi.L // 2 - 1, True)
    assert kb.LanczosGroundState(H, theta, {})._native_program() is not None
    Hs = ShiftNpcLinearOperator(H, 2.5)
    assert Hs.native_input(theta) is None and kb.LanczosGroundState(Hs, theta, {})._native_program() is None
    E0 = kb.LanczosGroundState(H, theta, {}).run()[0]
    Es = kb.LanczosGroundState(Hs, theta, {}).run()[0]
    assert abs(Es - (E0 + 2.5)) <= 1e-12 * max(1., abs(E0))


def test_nested_projection_declines(obackend, monkeypatch):
    """One level of projection per program: a wrapper around a wrapper takes the step-by-step route."""
    monkeypatch.setattr(kb, 'NATIVE', True)
    eng = _engine('xxz')
    H, theta = _operator(eng, eng.psi.L // 2 - 1, True)
    rng = np.random.default_rng(41)
    inner_op = _wrapped(H, [random_like(theta, rng)])
    outer = _wrapped(inner_op, [random_like(theta, rng)])
    before = dict(kb.stats)
    assert inner_op.native_input(theta) is not None and outer.native_input(theta) is None
    assert kb.stats['n_native_ortho'] == before['n_native_ortho'] + 1


def test_unchanged_path(monkeypatch):
    """Neither option: no call of ``tpa_lanczos_run_ex`` or ``tpa_project_out`` (spies on the emulation's attributes)."""
    import mock_ortho
    npc.clear_device_caches()
    mock = mock_ortho.install(monkeypatch)
    seen = []
    for name in ('tpa_lanczos_run_ex', 'tpa_project_out'):
        real = getattr(mock, name)
        setattr(mock, name, (lambda f, nm: lambda *a: (seen.append(nm), f(*a))[1])(real, name))
    monkeypatch.setattr(kb, 'NATIVE', True)
    eng = _engine('xxz')
    H, theta = _operator(eng, eng.psi.L // 2 - 1, True)
    lz = kb.LanczosGroundState(H, theta, {})
    assert lz._native_program() is not None
    kb.LanczosGroundState(H, theta, {}).run()
    kb.LanczosEvolution(H, theta.astype(np.complex128), {}).run(-0.05j)
    assert seen == []
    Ho = _wrapped(H, [random_like(theta, np.random.default_rng(2))])
    kb.LanczosGroundState(Ho, theta, {}).run()
    assert 'tpa_lanczos_run_ex' in seen and 'tpa_project_out' in seen
    npc.clear_device_caches()
