"""``MpoExpandPlan`` / ``device_expand_1site`` (the fused matrix of the subspace expansion in one ``tpa_mpo_expand_batch`` launch from
``T1 = LP . theta``) against ``generic_expand_1site`` (the reference's statements through ``LHeff`` / ``RHeff``) on the same backend,
for an MPO of each plan class of the MPO step: scalar blocks (XXZ with Sz), small matrices on the physical index (Hubbard ladder with
N only), sorted and bunched bond legs (blocks wider than 1; real and complex) and wide physical sectors (bosons with parity).

Bound (u = 2^-53): elementwise |device - generic| <= gamma_n mag with n = d chi + chi + 2 D + 4 and
``mag = sum |LP| |W| mix |theta|`` from absolute values.  The generic route rounds D products (LP . W) and a scaling, then contracts
over d chi: its error is at most gamma_(d chi + D + 2) mag; the device route contracts over chi, then sums at most D d terms with one
host rounding each: gamma_(chi + D d + 2) mag.  D d <= D + d chi for every case here, so n covers the sum of the two."""
import numpy as np
import pytest

import mpo_apply_fixtures
import mpo_entry_fixtures
from expand_fixtures import xbackend  # noqa: F401
from tenpy_amd.algorithms import mixer, mps_common
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc

U = 2.0**-53
AMPLITUDE = 1.e-2
MODELS = ['xxz', 'xxz_sorted', 'ladder_N', 'ladder_sorted_complex', 'bosons']
_cache = {}


def gamma(n):
    return n * U / (1 - n * U)


def state(backend, name):
    """``(H, psi, env)`` of a named model after two sweeps of the stand-alone two-site driver, shared per backend."""
    if name != 'ladder_N':
        return mpo_entry_fixtures.model_state(backend, name)
    if (backend, name) not in _cache:
        eng = mpo_apply_fixtures.ladder_engine(3, conserve=('N',), chi=8)
        _cache[(backend, name)] = (eng.H, eng.psi, eng.env)
    return _cache[(backend, name)]


def operator(backend, name, i0):
    H, psi, env = state(backend, name)
    eff = mps_common.OneSiteH(env, i0)
    assert eff.factored, "the fixtures are MPOs with a factored one-site operator"
    theta = psi.get_theta(i0, n=1)
    assert list(theta.get_leg_labels()) == ['vL', 'p0', 'vR']
    return H, eff, theta


def dense_parts(eff, theta):
    LP = eff.LP.transpose(['vR*', 'wR', 'vR']).to_ndarray()
    RP = eff.RP.transpose(['wL', 'vL', 'vL*']).to_ndarray()
    W = eff.W0.transpose(['wL', 'wR', 'p0', 'p0*']).to_ndarray()
    return LP, RP, W, theta.transpose(['vL', 'p0', 'vR']).to_ndarray()


def dense_expand(eff, theta, mix, move_right, absolute=False):
    """theta_expand with split legs ([vL, p0, wR, vR] / [vL, wL, p0, vR]) from dense tensors; ``absolute``: the magnitude sums."""
    LP, RP, W, th = dense_parts(eff, theta)
    if absolute:
        LP, RP, W, th, mix = np.abs(LP), np.abs(RP), np.abs(W), np.abs(th), np.abs(mix)
    if move_right:      # LP[a', w, a] theta[a, q, b] W[w, x, p, q] mix[x] -> [a', p, x, b]
        return np.einsum('awc,cqb,wxpq,x->apxb', LP, th, W, mix, optimize=True)
    return np.einsum('aqc,wcb,xwpq,x->axpb', th, RP, W, mix, optimize=True)        # theta[a, q, c] RP[w, c, b'] W[x, w, p, q]


def split_dense(E, move_right):
    return E.split_legs().transpose(['vL', 'p0', 'wR', 'vR'] if move_right else ['vL', 'wL', 'p0', 'vR']).to_ndarray()


def n_of(eff, theta):
    d, chi = theta.get_leg('p0').ind_len, max(theta.get_leg('vL').ind_len, theta.get_leg('vR').ind_len)
    D = max(eff.W0.get_leg('wL').ind_len, eff.W0.get_leg('wR').ind_len)
    return d * chi + chi + 2 * D + 4


def same_structure(got, want):
    assert got.get_leg_labels() == want.get_leg_labels()
    for a, b in zip(got.legs, want.legs):
        a.test_equal(b)
    assert np.array_equal(got.qtotal, want.qtotal)
    g, w = got.copy(deep=False), want.copy(deep=False)
    g.isort_qdata(), w.isort_qdata()
    assert np.array_equal(g._qdata, w._qdata), "block structure"


def written_once(plan):
    """Every element of the arena is listed by exactly one (job, row, i, j) of the tables."""
    count = np.zeros(plan.total, dtype=np.int64)
    for dst_off, pre, n_rows, post, row_begin, dst_ld, _, _ in plan.jobs_host.tolist():
        row_off = plan.rows_host[row_begin:row_begin + n_rows, 2]
        idx = dst_off + np.arange(pre)[:, None, None] * dst_ld + row_off[None, :, None] + np.arange(post)[None, None, :]
        np.add.at(count, idx.reshape(-1), 1)
    assert np.all(count == 1)


@pytest.mark.parametrize("move_right", [True, False], ids=['right', 'left'])
@pytest.mark.parametrize("name", MODELS)
def test_device_against_generic(xbackend, monkeypatch, name, move_right):
    H, psi, _ = state(xbackend, name)
    sites = [1, psi.L // 2] if move_right else [psi.L // 2, psi.L - 2]
    for i0 in sites:
        H, eff, theta = operator(xbackend, name, i0)
        if xbackend == 'mock':      # an element that no job writes stays NaN
            real_empty = dev.empty
            monkeypatch.setattr(dev, 'empty', lambda n, dt: real_empty(n, dt).fill_(float('nan')))
        n_dev = mixer.stats['device_expand']
        got = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right)
        if xbackend == 'mock':
            monkeypatch.setattr(dev, 'empty', real_empty)
        assert got is not None and mixer.stats['device_expand'] == n_dev + 1
        E, Id = got
        assert not np.isnan(dev.to_host(E._arena).view(np.float64)).any(), "an element of the arena was not written"
        plan = eff._expandplans[move_right]
        written_once(plan)
        assert plan.bytes > 0 and plan.flops > 0
        want, Id_want = mixer.generic_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right)
        assert Id == Id_want and Id is not None
        same_structure(E, want)
        mix_L, mix_R, IdL, IdR = mixer.mix_weights(H, i0 if move_right else i0 - 1, np.sqrt(AMPLITUDE))
        mix = mix_L if move_right else mix_R
        mag = dense_expand(eff, theta, mix, move_right, absolute=True)
        exact = dense_expand(eff, theta, mix, move_right)
        d_got, d_want = split_dense(E, move_right), split_dense(want, move_right)
        bound = gamma(n_of(eff, theta)) * mag
        worst = float(np.max(np.abs(d_got - d_want) / np.maximum(bound, 1e-300)))
        print("%s %s i0=%d: %s blocks=%d jobs=%d rows=%d terms=%d, max |device - generic| / bound = %.3g"
              % (name, 'right' if move_right else 'left', i0, E.shape, E.stored_blocks, plan.n_jobs, len(plan.rows_host), len(plan.term_w), worst))
        assert np.all(np.abs(d_got - d_want) <= bound)
        assert np.all(np.abs(d_got - exact) <= bound)
        assert np.abs(exact).max() > 0
        # the second call replays the plan: identical bits
        again, _ = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right)
        assert eff._expandplans[move_right] is plan
        assert np.array_equal(dev.to_host(again._arena).view(np.int64), dev.to_host(E._arena).view(np.int64))


@pytest.mark.parametrize("move_right", [True, False], ids=['right', 'left'])
@pytest.mark.parametrize("name", ['xxz', 'ladder_sorted_complex'])
def test_stacked_form(xbackend, name, move_right):
    """``IdL`` (right move) / ``IdR`` (left move) = ``None``: theta itself on a trivial first index of the outgoing MPO leg, read from
    the second source, followed by the indices that survive the projection with the weight sqrt(amplitude)."""
    H, psi, _ = state(xbackend, name)
    i0 = psi.L // 2
    H, eff, theta = operator(xbackend, name, i0)
    mix_L, mix_R, IdL, IdR = mixer.mix_weights(H, i0 if move_right else i0 - 1, np.sqrt(AMPLITUDE))
    weights = (mix_L, mix_R, None, IdR) if move_right else (mix_L, mix_R, IdL, None)
    E, Id = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right, weights=weights)
    want, Id_want = mixer.generic_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right, weights=weights)
    assert Id == Id_want == 0
    plan = eff._expandplans[move_right]
    assert plan.stacked and np.count_nonzero(plan.rows_host[:, 3]) > 0
    written_once(plan)
    same_structure(E, want)
    keep = np.ones(len(mix_L), bool)
    keep[IdR if move_right else IdL] = False
    s = np.sqrt(AMPLITUDE)
    ax = 2 if move_right else 1
    th = np.expand_dims(theta.to_ndarray(), ax)
    exact = np.concatenate([th, np.compress(keep, dense_expand(eff, theta, np.full(len(keep), s), move_right), axis=ax)], axis=ax)
    mag = np.concatenate([np.abs(th), np.compress(keep, dense_expand(eff, theta, np.full(len(keep), s), move_right, absolute=True), axis=ax)], axis=ax)
    d_got, d_want = split_dense(E, move_right), split_dense(want, move_right)
    bound = gamma(n_of(eff, theta)) * mag
    assert np.all(np.abs(d_got - d_want) <= bound) and np.all(np.abs(d_got - exact) <= bound)
    sl = np.take(d_got, 0, axis=ax)
    assert np.array_equal(sl, theta.to_ndarray()), "the rows of theta are copies (one term, alpha = 1)"


def test_zero_weights_are_stored(xbackend):
    """The sector that ``mix = 0`` on ``IdR`` wipes out (right move) holds zeros, as after the reference's ``iscale_axis``: its blocks
    are stored, its rows have no terms."""
    H, psi, _ = state(xbackend, 'xxz')
    i0 = psi.L // 2
    H, eff, theta = operator(xbackend, 'xxz', i0)
    mix_L, _, IdL, IdR = mixer.mix_weights(H, i0, np.sqrt(AMPLITUDE))
    assert mix_L[IdR] == 0.
    E, _ = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, True)
    want, _ = mixer.generic_expand_1site(eff, H, theta, i0, AMPLITUDE, True)
    same_structure(E, want)
    d = split_dense(E, True)
    assert np.all(d[:, :, IdR, :] == 0)
    plan = eff._expandplans[True]
    assert np.any(plan.rows_host[:, 1] == 0) and not np.any(plan.term_w == IdR)
    full = dense_expand(eff, theta, np.ones(len(mix_L)), True, absolute=True)
    assert np.any(full[:, :, IdR, :] > 0), "the zero weight wipes out something"


def test_amplitude_change_keeps_the_plan(xbackend):
    H, psi, _ = state(xbackend, 'xxz')
    i0 = psi.L // 2
    H, eff, theta = operator(xbackend, 'xxz', i0)
    E1, _ = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, True)
    plan = eff._expandplans[True]
    E2, _ = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE / 4, True)
    assert eff._expandplans[True] is plan
    want, _ = mixer.generic_expand_1site(eff, H, theta, i0, AMPLITUDE / 4, True)
    mix = mixer.mix_weights(H, i0, np.sqrt(AMPLITUDE / 4))[0]
    bound = gamma(n_of(eff, theta)) * dense_expand(eff, theta, mix, True, absolute=True)
    assert np.all(np.abs(split_dense(E2, True) - split_dense(want, True)) <= bound)
    assert not np.array_equal(split_dense(E1, True), split_dense(E2, True))


def test_prepared_theta_keeps_its_pipe(xbackend):
    """theta prepared for the SVD (``[(vL.p0), vR]`` / ``[vL, (p0.vR)]``): its pipe is the pipe of the result."""
    H, psi, _ = state(xbackend, 'xxz_sorted')
    i0 = psi.L // 2
    H, eff, theta = operator(xbackend, 'xxz_sorted', i0)
    for move_right in (True, False):
        th2 = theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0) if move_right else theta.combine_legs(['p0', 'vR'], qconj=-1, new_axes=1)
        E, _ = mixer.device_expand_1site(eff, H, th2, i0, AMPLITUDE, move_right)
        assert E.legs[0 if move_right else 1] is th2.legs[0 if move_right else 1]
        want, _ = mixer.generic_expand_1site(eff, H, th2, i0, AMPLITUDE, move_right)
        same_structure(E, want)
        E3, _ = mixer.device_expand_1site(eff, H, theta, i0, AMPLITUDE, move_right)
        assert np.array_equal(split_dense(E, move_right), split_dense(E3, move_right))


def _declined(fn, why):
    n, w = mixer.stats['expand_declined'], mixer.stats['why'].get(why, 0)
    assert fn() is None
    assert mixer.stats['expand_declined'] == n + 1 and mixer.stats['why'].get(why, 0) == w + 1, why


def test_declines_are_counted(xbackend, monkeypatch):
    H, psi, env = state(xbackend, 'xxz')
    i0 = psi.L // 2
    H, eff, theta = operator(xbackend, 'xxz', i0)
    call = lambda e=eff, h=H, t=theta: mixer.device_expand_1site(e, h, t, i0, AMPLITUDE, True)
    assert call() is not None
    # switched off: the generic statements, no device expansion
    monkeypatch.setenv('TPA_EXPAND_DEVICE', '0')
    n = mixer.stats['device_expand']
    _declined(call, 'switched off')
    assert mixer.stats['device_expand'] == n

    class Eng:
        eff_H, trunc_params = eff, {}

        class env:
            pass
    Eng.env.H = H
    got_E, got_Id = mixer.SubspaceExpansion({'amplitude': AMPLITUDE}).expand(Eng, theta, i0, True)      # ... and the mixer issues the generic statements
    want_E, want_Id = mixer.generic_expand_1site(eff, H, theta, i0, AMPLITUDE, True)
    assert got_Id == want_Id and mixer.stats['device_expand'] == n
    same_structure(got_E, want_E)
    assert np.array_equal(split_dense(got_E, True), split_dense(want_E, True))
    monkeypatch.delenv('TPA_EXPAND_DEVICE')
    # an operator that is not a factored OneSiteH
    two = mps_common.TwoSiteH(env, i0)
    _declined(lambda: call(e=two), 'operator')
    unf = mps_common.OneSiteH(env, i0)
    unf.factored = False
    _declined(lambda: call(e=unf), 'operator')

    class Flags:
        def __init__(self, H, **kw):
            self.__dict__.update(H.__dict__)
            self.__dict__.update(kw)
            self._H = H

        def __getattr__(self, name):
            return getattr(self._H, name)
    _declined(lambda: call(h=Flags(H, explicit_plus_hc=True)), 'explicit_plus_hc')
    _declined(lambda: call(h=Flags(H, finite=False)), 'infinite')

    class Env:
        bra, ket = object(), object()
    other = mps_common.OneSiteH(env, i0)
    other._env = Env()
    _declined(lambda: call(e=other), 'bra is not ket')
    _declined(lambda: call(t=theta.astype(np.complex128)), 'mixed dtypes')
    charged = mps_common.OneSiteH(env, i0)
    charged.LP = charged.LP.copy(deep=False)
    charged.LP.qtotal = charged.LP.qtotal + 1
    _declined(lambda: call(e=charged), 'charged environment')
    empty = npc.Array(theta.legs, theta.dtype, theta.qtotal, theta.get_leg_labels())
    _declined(lambda: call(t=empty), 'empty theta')
    # more cells than one launch takes jobs: declined, not raised
    fresh = mps_common.OneSiteH(env, i0)
    monkeypatch.setattr(mps_common.MpoExpandPlan, 'MAX_JOBS', 3)
    npc.clear_device_caches()
    _declined(lambda: call(e=fresh), 'too many jobs')
    monkeypatch.setattr(mps_common.MpoExpandPlan, 'MAX_JOBS', 60000)
    assert call(e=fresh) is not None
    if xbackend == 'mock':          # an emulation that predates the entry point
        monkeypatch.delattr(dev.lib(), 'tpa_mpo_expand_batch')
        _declined(call, 'entry point')
