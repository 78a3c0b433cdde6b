"""``device_mix_rho`` (tenpy_amd/algorithms/mixer.py: X by the operator's own tensors, then one ``tpa_herk_chain`` launch per source)
against dense numpy contractions of the same tensors, on the emulation and on the GPU.

Operators: factored and fused ``TwoSiteH`` on a bulk bond of the XXZ chain (real), the Hubbard ladder with a Peierls phase and sorted
MPO bond legs (complex, bond blocks wider than 1: periodic weights) and a synthetic bond whose largest pipe sector has 140 rows
(three tiles per side: strictly lower, diagonal and skipped tiles).  Tolerance 1e-13 * max|entry| (tests/test_heff_entries.py)."""
import numpy as np
import pytest

from mixer_fixtures import mbackend  # noqa: F401
from mpo_entry_fixtures import bond_tensors, model_state
from tenpy_amd.algorithms import mixer, mps_common
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import LegCharge

NAMES = ['xxz', 'xxz_sorted', 'ladder_sorted_complex']


def _dense_rho(tensors, i0, theta2, mix_L, mix_R, IdL, IdR, mix_left, mix_right):
    """numpy: rho_L[a, d] = sum X[a, w, c] mix_L[w] conj(X[d, w, c]), X = LHeff . theta (+ theta theta^dagger when IdL is None);
    rho_R[r, s] = sum X[a, w, r] mix_R[w] conj(X[a, w, s]), X = theta . RHeff; an unmixed side is theta theta^dagger / theta^T theta^*.
    LHeff / RHeff come from an operator of their own (fused mode)."""
    ref = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=False)
    th = ref.combine_theta(theta2.split_legs() if theta2.rank == 2 else theta2).to_ndarray()
    plain_L, plain_R = th @ th.conj().T, th.T @ th.conj()
    if mix_left:
        X = np.tensordot(ref.LHeff.to_ndarray(), th, ([2], [0]))                       # a w c
        rho_L = (X * mix_L[None, :, None]).reshape(len(X), -1) @ X.conj().reshape(len(X), -1).T + (plain_L if IdL is None else 0)
    else:
        rho_L = plain_L
    if mix_right:
        X = np.tensordot(th, ref.RHeff.to_ndarray(), ([1], [1]))                       # a w r
        n = X.shape[2]
        rho_R = (X * mix_R[None, :, None]).reshape(-1, n).T @ X.conj().reshape(-1, n) + (plain_R if IdR is None else 0)
    else:
        rho_R = plain_R
    return rho_L, rho_R, ref


def _close(got, want, what):
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print("%s: max err %.3g, max |entry| %.3g" % (what, err, scale))
    assert err <= 1e-13 * scale, what


def _check(rho, want, pipe, labels, what):
    assert list(rho.get_leg_labels()) == labels
    pipe.test_equal(rho.legs[0])
    pipe.conj().test_equal(rho.legs[1])
    assert np.all(rho.qtotal == 0) and np.array_equal(rho._qdata[:, 0], rho._qdata[:, 1])
    d = rho.to_ndarray()
    assert np.array_equal(d, d.conj().T), what + ": not Hermitian bit for bit"
    assert np.all(np.diagonal(d).imag == 0.0)
    _close(d, want, what)
    # block diagonal with complete blocks: everything outside the stored sector blocks of `want` is zero as well
    mask = np.zeros(d.shape, bool)
    for q in rho._qdata[:, 0]:
        mask[pipe.slices[q]:pipe.slices[q + 1], pipe.slices[q]:pipe.slices[q + 1]] = True
    assert np.all(want[~mask] == 0)


def _weights(rng, chi, IdL, IdR):
    """Random positive weights, an exact zero and a negative one among them: every entry of a wide bond block is different."""
    mix_L, mix_R = rng.uniform(0.1, 1., chi), rng.uniform(0.1, 1., chi)
    mix_L[-1], mix_R[0] = 0., 0.
    if chi > 2:
        mix_L[1] *= -1
    return mix_L, mix_R, IdL, IdR


@pytest.mark.parametrize("factored", [True, False], ids=['factored', 'fused'])
@pytest.mark.parametrize("name", NAMES)
def test_device_mix_rho(mbackend, name, factored):
    H, psi, env = model_state(mbackend, name)
    i0 = psi.L // 2 - 1
    tensors = bond_tensors(H, env, i0)
    rng = np.random.default_rng(11)
    chi = tensors[2].get_leg('wR').ind_len
    if 'sorted' in name:
        assert int(np.max(tensors[2].get_leg('wR').get_block_sizes())) > 1
    for (IdL, IdR), (ml, mr) in [((0, chi - 1), (True, True)), ((None, chi - 1), (True, False)), ((0, None), (False, True)),
                                 ((None, None), (True, True))]:
        eff = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=factored)
        assert eff.factored is factored
        theta = eff.combine_theta(psi.get_theta(i0, n=2))
        w = _weights(rng, chi, IdL, IdR)
        want_L, want_R, ref = _dense_rho(tensors, i0, theta, *w, ml, mr)
        for rep in range(2):                 # the second call replays the cached plans
            built = mixer.stats['plans_built']
            rho_L, rho_R = mixer.device_mix_rho(eff, H, theta, i0, 1.e-5, ml, mr, weights=w)
            assert (mixer.stats['plans_built'] == built) == (rep == 1)
            what = '%s %s IdL=%s IdR=%s mix=%s/%s' % (name, 'factored' if factored else 'fused', IdL, IdR, ml, mr)
            _check(rho_L, want_L, ref.pipeL, ['(vL.p0)', '(vL*.p0*)'], what + ' rho_L')
            _check(rho_R, want_R, ref.pipeR, ['(p1.vR)', '(p1*.vR*)'], what + ' rho_R')
        if factored:
            assert eff._LHeff is None and eff._RHeff is None, "the factored route must not build LHeff / RHeff"


def test_device_mix_rho_reference_weights(mbackend):
    """The weights of ``_mix_LR`` (amplitude, 1 at IdL, 0 at IdR and mirrored) when none are handed in; rho agrees with an eigenvalue
    sum: tr rho_L = sum_w mix_L[w] |X_w|^2."""
    H, psi, env = model_state(mbackend, 'xxz')
    i0 = psi.L // 2 - 1
    mix_L, mix_R, IdL, IdR = mixer.mix_weights(H, i0, 1.e-3)
    chi = len(mix_L)
    assert (IdL, IdR) == (0, chi - 1) and mix_L[0] == 1. and mix_L[-1] == 0. and mix_R[0] == 0. and mix_R[-1] == 1.
    assert np.all(mix_L[1:-1] == 1.e-3) and np.all(mix_R[1:-1] == 1.e-3)
    tensors = bond_tensors(H, env, i0)
    eff = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=True)
    theta = eff.combine_theta(psi.get_theta(i0, n=2))
    rho_L, rho_R = mixer.device_mix_rho(eff, H, theta, i0, 1.e-3, True, True)
    want_L, want_R, _ = _dense_rho(tensors, i0, theta, mix_L, mix_R, IdL, IdR, True, True)
    _close(rho_L.to_ndarray(), want_L, 'rho_L with the reference weights')
    _close(rho_R.to_ndarray(), want_R, 'rho_R with the reference weights')


def _synthetic_bond(cplx, rng):
    """Random LP, RP, theta on a bond leg with blocks of 50, 90 and 50 states around the bulk MPO tensors of the XXZ chain: the
    largest sector of (vL.p0) has 140 rows."""
    from tenpy_amd.models.spin_chains import xxz_chain_mpo
    H = xxz_chain_mpo(6, 1., 0.7, 0.1)
    W0, W1 = H.get_W(2), H.get_W(3)
    chinfo = W0.chinfo
    leg = LegCharge.from_qind(chinfo, [0, 50, 140, 190], [[-2], [0], [2]], qconj=+1)
    dt = np.complex128 if cplx else np.float64

    def rnd(shape):
        return rng.standard_normal(shape) + (1j * rng.standard_normal(shape) if cplx else 0)
    LP = npc.Array.from_func(rnd, [leg, W0.get_leg('wL').conj(), leg.conj()], dtype=dt, labels=['vR*', 'wR', 'vR'])
    RP = npc.Array.from_func(rnd, [leg, W1.get_leg('wR').conj(), leg.conj()], dtype=dt, labels=['vL', 'wL', 'vL*'])
    theta = npc.Array.from_func(rnd, [leg, W0.get_leg('p'), W1.get_leg('p'), leg.conj()], dtype=dt, labels=['vL', 'p0', 'p1', 'vR'])
    return H, (LP, RP, W0.astype(dt), W1.astype(dt)), theta


@pytest.mark.parametrize("cplx", [False, True], ids=['real', 'complex'])
@pytest.mark.parametrize("factored", [True, False], ids=['factored', 'fused'])
def test_device_mix_rho_sector_of_140_rows(mbackend, cplx, factored):
    rng = np.random.default_rng(12)
    H, tensors, theta4 = _synthetic_bond(cplx, rng)
    eff = mps_common.TwoSiteH(None, 2, tensors=tensors, factored=factored)
    assert eff.factored is factored
    assert int(np.max(eff.pipeL.get_block_sizes())) >= 130 and int(np.max(eff.pipeR.get_block_sizes())) >= 130
    theta = eff.combine_theta(theta4)
    chi = tensors[2].get_leg('wR').ind_len
    w = _weights(rng, chi, 0, chi - 1)
    rho_L, rho_R = mixer.device_mix_rho(eff, H, theta, 2, 1.e-5, True, True, weights=w)
    want_L, want_R, ref = _dense_rho(tensors, 2, theta, *w, True, True)
    _check(rho_L, want_L, ref.pipeL, ['(vL.p0)', '(vL*.p0*)'], 'synthetic rho_L')
    _check(rho_R, want_R, ref.pipeR, ['(p1.vR)', '(p1*.vR*)'], 'synthetic rho_R')


def test_device_mix_rho_declines(mbackend, monkeypatch):
    H, psi, env = model_state(mbackend, 'xxz')
    i0 = psi.L // 2 - 1
    tensors = bond_tensors(H, env, i0)
    eff = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=True)
    theta = eff.combine_theta(psi.get_theta(i0, n=2))
    args = (H, theta, i0, 1.e-5, True, True)
    assert mixer.device_mix_rho(eff, *args) is not None
    n = mixer.stats['declined']
    monkeypatch.setenv('TPA_MIXER_DEVICE', '0')
    assert mixer.device_mix_rho(eff, *args) is None
    monkeypatch.delenv('TPA_MIXER_DEVICE')
    assert mixer.device_mix_rho(eff, H, theta.astype(np.complex128), i0, 1.e-5, True, True) is None          # mixed dtypes

    class Other(mps_common.TwoSiteH):          # not the plain operator (PlusHcH, sharded operators): the generic statements
        pass
    assert mixer.device_mix_rho(Other(None, i0, tensors=tensors, factored=True), *args) is None

    class Infinite:
        finite, explicit_plus_hc = False, False
    assert mixer.device_mix_rho(eff, Infinite(), theta, i0, 1.e-5, True, True) is None
    charged = mps_common.TwoSiteH(None, i0, tensors=tensors, factored=True)
    charged.LP = charged.LP.copy()
    charged.LP.qtotal = charged.LP.qtotal + 1
    assert mixer.device_mix_rho(charged, *args) is None
    assert mixer.stats['declined'] == n + 5


@pytest.mark.parametrize("name", ['xxz', 'hubbard'])
@pytest.mark.parametrize("factored", [True, False], ids=['factored', 'fused'])
def test_device_mix_rho_explicit_plus_hc(mbackend, name, factored):
    """MPOs that hold half of H: the device route (plain operator behind ``PlusHcH``, weights of ``_mix_LR`` with one = 0.5, the factor
    2 on the weights) against the reference's statement order ``rho + rho^dagger`` issued through ``npc`` (``generic_mix_rho``)."""
    import plus_hc_fixtures as phc
    H, psi, env = phc.model_state(mbackend, name)
    assert H.explicit_plus_hc
    i0 = psi.L // 2 - 1
    op = mps_common.TwoSiteH(env, i0, factored=factored)
    assert op.factored is factored
    doubled = op.plus_hc()
    assert isinstance(doubled, mps_common.PlusHcH)
    theta = op.combine_theta(psi.get_theta(i0, n=2))
    mix_L, mix_R, IdL, IdR = mixer.mix_weights(H, i0, 1.e-3)
    assert mix_L[IdL] == 0.5 and mix_R[IdR] == 0.5
    for weights in (None, (mix_L, mix_R, None, None)):
        n = mixer.stats['device_mix_rho']
        got = mixer.device_mix_rho(doubled, H, theta, i0, 1.e-3, True, True, weights=weights)
        assert got is not None and mixer.stats['device_mix_rho'] == n + 1
        ref_op = mps_common.TwoSiteH(env, i0, factored=False)
        want = mixer.generic_mix_rho(ref_op, H, ref_op.combine_theta(psi.get_theta(i0, n=2)), i0, 1.e-3, True, True, weights=weights)
        for g, w, what in zip(got, want, ('rho_L', 'rho_R')):
            assert list(g.get_leg_labels()) == list(w.get_leg_labels())
            _close(g.to_ndarray(), w.to_ndarray(), '%s %s explicit_plus_hc %s' % (name, 'factored' if factored else 'fused', what))
    if factored:
        assert op._LHeff is None and op._RHeff is None


@pytest.mark.parametrize("form", ['factored', 'fused', 'plus_hc'])
@pytest.mark.parametrize("name", ['xxz', 'hubbard'])
def test_device_mix_rho_nonsquare_bond(mbackend, name, form):
    """A bond whose ``LP`` has a block with different extents on its two virtual legs (``plus_hc_fixtures.nonsquare_bond``): the
    slices of (vL.p0) and (p1.vR) differ in size there, so an exchange of row count and contracted length, or slice offsets taken
    from the wrong pipe, cannot cancel.  Factored and fused against the dense contraction with random weights; ``PlusHcH`` against the
    reference's statement order on the same operator."""
    import plus_hc_fixtures as phc
    H, psi, env = phc.model_state(mbackend, name)
    i0 = phc.nonsquare_bond(psi, env)
    tensors = bond_tensors(H, env, i0)
    assert len(set(tensors[0].get_leg('vR').get_block_sizes().tolist())) > 1 or tensors[0].get_leg('vR').ind_len != tensors[1].get_leg('vL').ind_len
    rng = np.random.default_rng(13)
    chi = tensors[2].get_leg('wR').ind_len
    op = mps_common.TwoSiteH(env, i0, factored=(form != 'fused'))
    assert op.factored is (form != 'fused')
    theta = op.combine_theta(psi.get_theta(i0, n=2))
    if form == 'plus_hc':
        got = mixer.device_mix_rho(op.plus_hc(), H, theta, i0, 1.e-3, True, True)
        ref_op = mps_common.TwoSiteH(env, i0, factored=False)
        want = mixer.generic_mix_rho(ref_op, H, ref_op.combine_theta(psi.get_theta(i0, n=2)), i0, 1.e-3, True, True)
        for g, w, what in zip(got, want, ('rho_L', 'rho_R')):
            _close(g.to_ndarray(), w.to_ndarray(), '%s nonsquare bond %d plus_hc %s' % (name, i0, what))
        return

    class Plain:            # the same tensors as a full MPO: the weights are handed in
        explicit_plus_hc, finite = False, True
    for IdL, IdR in ((0, chi - 1), (None, None)):
        w = _weights(rng, chi, IdL, IdR)
        rho_L, rho_R = mixer.device_mix_rho(op, Plain(), theta, i0, 1.e-5, True, True, weights=w)
        want_L, want_R, ref = _dense_rho(tensors, i0, theta, *w, True, True)
        _check(rho_L, want_L, ref.pipeL, ['(vL.p0)', '(vL*.p0*)'], '%s nonsquare bond %d %s rho_L' % (name, i0, form))
        _check(rho_R, want_R, ref.pipeR, ['(p1.vR)', '(p1*.vR*)'], '%s nonsquare bond %d %s rho_R' % (name, i0, form))


def test_device_mix_rho_declines_bra_not_ket_and_sharded(mbackend):
    """The two declines that need their own objects: an environment whose bra is not its ket, and the sharded operator class."""
    from tenpy_amd.algorithms.sharded import ShardedTwoSiteH
    H, psi, env = model_state(mbackend, 'xxz')
    i0 = psi.L // 2 - 1
    eff = mps_common.TwoSiteH(env, i0, factored=True)
    theta = eff.combine_theta(psi.get_theta(i0, n=2))
    assert mixer.device_mix_rho(eff, H, theta, i0, 1.e-5, True, True) is not None

    class OtherBra:
        def __init__(self, env):
            self.__dict__.update(env.__dict__)
            self.bra, self.ket = psi.copy(), psi
    eff._env = OtherBra(env)
    n = dict(mixer.stats['why'])
    assert mixer.device_mix_rho(eff, H, theta, i0, 1.e-5, True, True) is None
    assert mixer.stats['why'].get('bra is not ket', 0) == n.get('bra is not ket', 0) + 1
    sharded = object.__new__(ShardedTwoSiteH)              # (no process group here: the class alone decides)
    assert mixer.device_mix_rho(sharded, H, theta, i0, 1.e-5, True, True) is None
    assert mixer.stats['why'].get('operator', 0) == n.get('operator', 0) + 1
