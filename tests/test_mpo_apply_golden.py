"""The stand-alone ``MPO.apply`` (zip-up pass on the device, then ``MPS.compress_svd``) against the reference's own ``MPO.apply`` with
``compression_method='zip_up'`` on the XXZ chain L = 8 (tests/golden/mpo_apply.pkl, records ``untruncated`` and ``truncating``;
generator tests/golden/make_golden_mpo_apply.py), on the emulation and on the GPU.  The W tensors of ``U_II`` come from the fixture.

Bounds:

* ``untruncated`` (chi_max = 16: no cut above svd_min): the normalised state vector within 1e-12 of the stored one after fixing the
  global phase, S of every bond within 1e-12 sigma_max (the project's SVD tolerance), |<psi|psi> - 1| <= 1e-12.
* ``truncating`` (chi_max = 4, m_temp = 2, 8 applications): a cut rotates the kept subspace by at most (perturbation) / gap, so state and S
  are within 10 n_cuts 1e-12 / g -- the gap rule of tests/test_1site_golden.py summed over the stored cuts, ``g`` the smallest stored gap
  between the last kept and the first dropped normalised singular value --, and so is the summed truncation error."""
import os
import pickle

import numpy as np
import pytest

from mpo_cell_fixtures import blocked_array, cbackend  # noqa: F401
from tenpy_amd.algorithms import mps_common
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks.mpo import MPO
from tenpy_amd.networks.mps import MPS

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mpo_apply.pkl'), 'rb') as _f:
    GOLD = pickle.load(_f)


def _setup():
    rec = GOLD['untruncated']['mpo']
    chinfo = ChargeInfo([int(m) for m in rec['chinfo_mod']])
    Ws = [blocked_array(w, chinfo, np.complex128) for w in rec['W']]
    p = LegCharge.from_qflat(chinfo, rec['p_leg'][0], qconj=rec['p_leg'][1])
    U = MPO([p] * len(Ws), Ws, IdL=rec['IdL'], IdR=rec['IdR'])
    psi = MPS.from_product_state([p] * len(Ws), GOLD['untruncated']['init'])
    return U, psi


def _vector(psi):
    th = psi.get_B(0, 'Th')
    for i in range(1, psi.L):
        th = npc.tensordot(th, psi.get_B(i, 'B').replace_label('p', 'p%d' % i), axes=['vR', 'vL'])
    return th.to_ndarray().reshape(-1)


def _run(rec, monkeypatch, mode):
    monkeypatch.setenv('TPA_MPO_CELL', str(mode))
    mps_common.reset_zipup_stats()
    U, psi = _setup()
    opts = dict(compression_method='zip_up', trunc_params=dict(chi_max=rec['chi_max'], svd_min=rec['svd_min']), m_temp=rec['m_temp'])
    eps = 0.
    for _ in range(rec['n_apply']):
        eps += U.apply(psi, dict(opts)).eps
    st = mps_common.zipup_stats
    assert st['device_steps'] == rec['n_apply'] * (psi.L - 2) and st['declined'] == 0, "every interior site runs on the device route"
    assert st['cell_launches'] == (st['device_steps'] if mode == 2 else 0)
    return psi, eps


def _compare(psi, rec, tol, tag):
    vec, want = _vector(psi), rec['vec']
    assert vec.shape == want.shape
    phase = np.vdot(vec, want)
    d_vec = float(np.abs(vec * (phase / abs(phase)) - want).max())
    d_S = max(float(np.abs(np.asarray(psi.get_SL(i)) - rec['S'][i - 1]).max()) if len(psi.get_SL(i)) == len(rec['S'][i - 1]) else np.inf
              for i in range(1, psi.L))
    d_norm = abs(psi.norm - rec['norm'])
    print("MPO_APPLY_GOLDEN %s: state max err %.3g, S max err %.3g, norm err %.3g (bound %.3g); chi %s"
          % (tag, d_vec, d_S, d_norm, tol, [len(psi.get_SL(i)) for i in range(1, psi.L)]))
    assert d_vec <= tol and d_S <= tol * max(s[0] for s in rec['S']) and d_norm <= tol * rec['norm']


@pytest.mark.parametrize("mode", [0, 2])
def test_untruncated(cbackend, monkeypatch, mode):
    rec = GOLD['untruncated']
    assert rec['n_cuts'] == 0 and rec['chi_max'] == 16 and rec['n_apply'] == 4
    psi, eps = _run(rec, monkeypatch, mode)
    _compare(psi, rec, 1e-12, 'untruncated mode=%d' % mode)
    assert abs(psi.norm_test() - 1.) <= 1e-12
    assert abs(eps - rec['err_eps']) <= 1e-12


@pytest.mark.parametrize("mode", [0, 2])
def test_truncating(cbackend, monkeypatch, mode):
    rec = GOLD['truncating']
    assert rec['n_cuts'] > 0 and rec['g'] >= 1e-5 and rec['chi_max'] == 4 and rec['m_temp'] == 2 and rec['n_apply'] == 8
    assert rec['g'] == float(np.min(rec['cuts'][:, 0] - rec['cuts'][:, 1]))
    tol = 10 * rec['n_cuts'] * 1e-12 / rec['g']
    psi, eps = _run(rec, monkeypatch, mode)
    _compare(psi, rec, tol, 'truncating mode=%d' % mode)
    print("MPO_APPLY_GOLDEN truncation error %.6g, stored %.6g, bound %.3g" % (eps, rec['err_eps'], tol))
    assert abs(eps - rec['err_eps']) <= tol
    assert abs(psi.norm_test() - 1.) <= 1e-12


def test_unserved_methods_are_named(cbackend):
    U, psi = _setup()
    for method in ('SVD', 'variational', 'variationalQR'):
        with pytest.raises(ValueError, match='zip_up'):
            U.apply(psi, dict(compression_method=method, trunc_params=dict(chi_max=4)))


def test_compress_svd_keeps_a_compressed_state(cbackend, monkeypatch):
    """``compress_svd`` on the state ``apply`` has already compressed: nothing changes beyond 1e-12."""
    rec = GOLD['truncating']
    monkeypatch.setenv('TPA_MPO_CELL', '2')
    U, psi = _setup()
    U.apply(psi, dict(compression_method='zip_up', trunc_params=dict(chi_max=4, svd_min=rec['svd_min']), m_temp=2))
    vec, S, norm = _vector(psi), [np.array(psi.get_SL(i)) for i in range(1, psi.L)], psi.norm
    err = psi.compress_svd(dict(chi_max=4, svd_min=rec['svd_min']))
    vec2 = _vector(psi)
    phase = np.vdot(vec2, vec)
    assert np.abs(vec2 * (phase / abs(phase)) - vec).max() <= 1e-12
    assert all(len(a) == len(psi.get_SL(i + 1)) and np.abs(a - psi.get_SL(i + 1)).max() <= 1e-12 for i, a in enumerate(S))
    assert abs(psi.norm - norm) <= 1e-12 * norm and err.eps <= 1e-12
