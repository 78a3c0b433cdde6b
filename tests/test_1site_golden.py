"""The subspace expansion against what the reference's ``SubspaceExpansion.mix_and_decompose_1site`` produced inside its own runs of
single-site DMRG (tests/golden/dmrg_1site.pkl, record ``percall``; generator tests/golden/make_golden_1site.py): the tensors of a
site are rebuilt from the dense arrays and charges of the fixture, ``device_expand_1site`` and the decomposition run on them -- on the
emulation and on the GPU.

Bounds (u = 2^-53):

* ``theta_expand``, element-wise: gamma_n ``mag`` with n = d chi + chi + 2 D + 4 (derivation: tests/test_expand_plan.py) and the stored
  magnitude sums ``mag`` = sum |LP| |W| mix |theta|.
* all singular values of ``theta_expand`` (normalised to norm 1): 1e-12 sigma_max, the project's SVD tolerance.
* where the fixture stores a gap (>= 1e-4 between the last kept and the first dropped singular value): ``err.eps`` to 1e-12, and
  ``U S VH`` within 10 x 1e-12 / gap of the stored one; ``U S VH`` is the truncated theta: normalised, it differs from the normalised
  theta by at most 2 sqrt(err.eps) (the dropped weight) plus that bound."""
import os
import pickle

import numpy as np
import pytest

from expand_fixtures import xbackend  # noqa: F401
from tenpy_amd.algorithms import mixer, mps_common
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo
from test_mixer_golden import _array

U = 2.0**-53
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dmrg_1site.pkl'), 'rb') as _f:
    CALLS = pickle.load(_f)['percall']
IDS = ['%s-i%d-%s%s' % (c['name'], c['i0'], 'right' if c['move_right'] else 'left', '-stacked' if c['stacked'] else '') for c in CALLS]


class _Neighbour:
    """The MPO tensor left of the site: only its ``wR`` leg is read (the number of weights of that bond)."""

    def __init__(self, W0):
        self.W0 = W0

    def get_leg(self, label):
        assert label == 'wR'
        return self.W0.get_leg('wL').conj()


class _H:
    """What the mixer reads of an MPO: the tensor of the site, IdL / IdR of the bond of this call, the h.c. flag."""
    finite = True
    explicit_plus_hc = False

    def __init__(self, W0, c):
        self.W0, self.c = W0, c

    def get_W(self, i):
        return self.W0 if i == self.c['i0'] else _Neighbour(self.W0)

    def get_IdL(self, i):
        return self.c['IdL']

    def get_IdR(self, i):
        return self.c['IdR']


class _Env:
    pass


class _Engine:
    pass


def test_fixture_is_what_the_generator_promises():
    assert {c['name'] for c in CALLS} == {'xxz', 'peierls_ladder'}
    for name in ('xxz', 'peierls_ladder'):
        mine = [c for c in CALLS if c['name'] == name]
        natural = [c for c in mine if not c['stacked']]
        assert len({c['i0'] for c in natural}) == 2 and len(natural) == 4 and {c['move_right'] for c in natural} == {True, False}
        assert sum(c['stacked'] for c in mine) >= 1
        assert all(c['sweep'] == 1 and c['trunc_params']['chi_max'] == 8 for c in mine)
    assert any(np.iscomplexobj(c['theta']['data']) for c in CALLS) and not all(np.iscomplexobj(c['theta']['data']) for c in CALLS)
    assert all(c['mag'].dtype == np.float32 and c['mag'].shape == c['theta_expand'].shape for c in CALLS)


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_call_against_the_reference(xbackend, c):
    cplx = any(np.iscomplexobj(c[k]['data']) for k in ('theta', 'W0', 'LP', 'RP'))
    dtype = np.complex128 if cplx else np.float64
    chinfo = ChargeInfo([int(m) for m in c['chinfo_mod']])
    LP, RP, W0, theta = (_array(c[k], chinfo, dtype) for k in ('LP', 'RP', 'W0', 'theta'))
    W0 = W0.replace_labels(['p0', 'p0*'], ['p', 'p*'])
    move_right, i0 = c['move_right'], c['i0']
    eff = mps_common.OneSiteH.from_LP_W0_RP(LP, W0, RP, i0, move_right=move_right)
    assert eff.factored
    H = _H(W0, c)
    got = mixer.device_expand_1site(eff, H, theta, i0, c['amplitude'], move_right)
    assert got is not None, "the device route declined"
    E, Id = got
    assert Id == (0 if c['stacked'] else (c['IdL'] if move_right else c['IdR']))
    labels = ['vL', 'p0', 'wR', 'vR'] if move_right else ['vL', 'wL', 'p0', 'vR']
    assert E.get_leg_labels() == (['(vL.p0)', '(wR.vR)'] if move_right else ['(vL.wL)', '(p0.vR)'])
    dense = E.split_legs().transpose(labels).to_ndarray()
    want = c['theta_expand']
    assert dense.shape == want.shape
    d, chi, D = theta.shape[1], max(theta.shape[0], theta.shape[2]), max(W0.get_leg('wL').ind_len, W0.get_leg('wR').ind_len)
    n = d * chi + chi + 2 * D + 4
    lim = n * U / (1 - n * U) * c['mag'].astype(np.float64)
    err = np.abs(dense - want)
    worst = float(np.max(err / np.maximum(lim, 1e-300)))
    print("1SITE_GOLDEN %s theta_expand %s max_err_over_bound=%.4f" % (IDS[CALLS.index(c)], dense.shape, worst))
    assert np.all(err <= lim)
    assert np.abs(want).max() > 0
    # all singular values before truncation
    S_all = np.sort(np.asarray(npc.svd(E, compute_uv=False)))[::-1]
    S_all = S_all / np.linalg.norm(S_all)
    assert len(S_all) == len(c['S_all'])
    print("1SITE_GOLDEN %s singular values max err %.3g (sigma_max %.3g)" % (IDS[CALLS.index(c)], np.abs(S_all - c['S_all']).max(), c['S_all'][0]))
    assert np.all(np.abs(S_all - c['S_all']) <= 1e-12 * c['S_all'][0])
    if 'USV' not in c:
        return
    assert c['gap'] >= 1.e-4
    eng = _Engine()
    eng.trunc_params, eng.eff_H, eng.env = dict(c['trunc_params']), eff, _Env()
    eng.env.H = H
    mix = mixer.SubspaceExpansion({'amplitude': c['amplitude']})
    th2 = theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0) if move_right else theta.combine_legs(['p0', 'vR'], qconj=-1, new_axes=1)
    Um, S, VH, terr = mix.mix_and_decompose_1site(eng, th2, i0, move_right)
    assert len(S) == c['n_keep'] and abs(terr.eps - c['err_eps']) <= 1e-12
    assert np.all(np.abs(np.sort(S)[::-1] - np.sort(c['S'])[::-1]) <= 1e-12 * np.max(c['S']) / np.linalg.norm(c['S_all'][:c['n_keep']]))
    assert Um.get_leg_labels() == (['(vL.p0)', 'vR'] if move_right else ['vL', 'vR'])
    assert VH.get_leg_labels() == (['vL', 'vR'] if move_right else ['vL', '(p0.vR)'])
    usv = npc.tensordot(Um, VH.scale_axis(S, 'vL'), axes=['vR', 'vL']).split_legs().transpose(['vL', 'p0', 'vR']).to_ndarray()
    lim_usv = 10 * 1e-12 / c['gap']
    d_usv = float(np.abs(usv - c['USV']).max())
    print("1SITE_GOLDEN %s U S VH max err %.3g, bound %.3g (gap %.3g)" % (IDS[CALLS.index(c)], d_usv, lim_usv, c['gap']))
    assert d_usv <= lim_usv
    th = theta.to_ndarray()
    diff = np.linalg.norm(usv / np.linalg.norm(usv) - th / np.linalg.norm(th))
    assert diff <= 2 * np.sqrt(terr.eps) + lim_usv, "U S VH is the truncated theta"
