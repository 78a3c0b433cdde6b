"""The density-matrix mixer against what the reference's ``DensityMatrixMixer`` produced inside its own mixer-on runs
(tests/golden/mixer.pkl, record ``percall``; generator tests/golden/make_golden_mixer.py): the tensors of a bond are rebuilt from the
dense arrays and charges of the fixture, ``device_mix_rho`` and ``svd_from_rho`` run on them -- on the emulation and on the GPU.

Bounds (EPS = 2^-52, f = 1 real / 2 complex; derived, not measured):

* ``rho``, element-wise.  The product ``X diag(s) X^dagger`` rounds like the conformance cases of ``tpa_herk_chain``:
  (f (K_rho + 2) + 1) EPS sum |s| |x| |x|  with K_rho = D d chi (the contracted wR, p1, vR).  X itself carries the rounding of the two
  contractions that form it, |dX| <= f K_X EPS |LP| |W| |theta| with K_X = chi d + D (through LHeff) or less (factored), and enters rho
  twice: 2 f K_X EPS more.  The fixture stores ``mag`` = sum |s| (|LP| |W| |theta|) (|LP| |W| |theta|)^T, which majorises both magnitude
  sums.  Both sides of the comparison (this route and the reference's numpy products) err by that much:
        |rho - golden| <= 2 (f (K_rho + 2 K_X + 2) + 1) EPS mag.
* kept eigenvalues (normalised to sum 1, as ``S_approx**2``): the ``tpa_eigh_batch`` bound of include/tenpy_amd.h,
  (6 n + 16 f' (1 + 2 sqrt n)) eps sqrt(n) |rho|_F with eps = 2^-53, f' = 4 for complex data, evaluated on the whole matrix (n its
  dimension: an upper bound of every block's), plus the Frobenius norm of the rho bound above (Weyl), both over the trace; times 2
  for the two sides.
* ``U S VH``: 10 x that eigenvalue bound / the stored relative gap between the last kept and the first dropped eigenvalue.
* ``U``, ``VH`` isometric: |U^dagger U - 1| <= 64 f' eps sqrt(n) (header)."""
import os
import pickle

import numpy as np
import pytest

from mixer_fixtures import mbackend  # noqa: F401
from tenpy_amd.algorithms import mixer, mps_common
from tenpy_amd.linalg import np_conserved as npc
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge

EPS = 2.0**-52
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mixer.pkl'), 'rb') as _f:
    GOLDEN = pickle.load(_f)
CALLS = GOLDEN['percall']
IDS = ['%s-i%d-%s' % (c['name'], c['i0'], 'right' if c['mix_left'] else 'left') for c in CALLS]


def _array(rec, chinfo, dtype):
    legs = [LegCharge.from_qflat(chinfo, q, qconj=qc) for q, qc in rec['legs']]
    return npc.Array.from_ndarray(rec['data'].astype(dtype), legs, dtype=dtype, qtotal=rec['qtotal'], labels=rec['labels'], cutoff=0.)


class _H:
    """What the mixer reads of an MPO: the tensor left of the bond, IdL / IdR of this bond, the h.c. flag."""
    finite = True

    def __init__(self, W0, c):
        self.W0, self.IdL, self.IdR, self.explicit_plus_hc = W0, c['IdL'], c['IdR'], c['explicit_plus_hc']

    def get_W(self, i):
        return self.W0


class _Engine:
    pass


def test_fixture_is_what_the_generator_promises():
    assert len(CALLS) == 12 and {c['name'] for c in CALLS} == {'xxz', 'peierls_ladder', 'xxz_plus_hc'}
    for name in ('xxz', 'peierls_ladder', 'xxz_plus_hc'):
        mine = [c for c in CALLS if c['name'] == name]
        assert len({c['i0'] for c in mine}) == 2 and {c['mix_left'] for c in mine} == {True, False}
        assert all(c['mix_left'] != c['mix_right'] and c['gap'] >= 1.e-4 and c['trunc_params']['chi_max'] <= 24 for c in mine)
    assert any(np.iscomplexobj(c['theta']['data']) for c in CALLS) and any(c['explicit_plus_hc'] for c in CALLS)


@pytest.mark.parametrize("factored", [True, False], ids=['factored', 'fused'])
@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_mixer_call_against_the_reference(mbackend, c, factored):
    cplx = np.iscomplexobj(c['theta']['data']) or np.iscomplexobj(c['W0']['data'])
    dtype = np.complex128 if cplx else np.float64
    chinfo = ChargeInfo([int(m) for m in c['chinfo_mod']])
    LP, RP, W0, W1, theta = (_array(c[k], chinfo, dtype) for k in ('LP', 'RP', 'W0', 'W1', 'theta'))
    W0, W1 = W0.replace_labels(['p0', 'p0*'], ['p', 'p*']), W1.replace_labels(['p1', 'p1*'], ['p', 'p*'])
    eff = mps_common.TwoSiteH(None, c['i0'], tensors=(LP, RP, W0, W1), factored=factored)
    if not factored:
        assert eff.factored is False
    H = _H(W0, c)
    got = mixer.device_mix_rho(eff, H, eff.combine_theta(theta), c['i0'], c['amplitude'], c['mix_left'], c['mix_right'])
    assert got is not None, "the device route declined"
    rho_L, rho_R = got
    if eff.factored:
        assert eff._LHeff is None and eff._RHeff is None
    f = 2 if cplx else 1
    chi, d, D = LP.get_leg('vR').ind_len, W0.get_leg('p').ind_len, W0.get_leg('wR').ind_len
    K_rho, K_X = D * d * RP.get_leg('vL').ind_len, max(chi, RP.get_leg('vL').ind_len) * d + D
    factor = 2 * (f * (K_rho + 2 * K_X + 2) + 1) * EPS
    worst, frob, trace = 0., {}, {}
    for side, rho, labels in (('L', rho_L, ['vL', 'p0', 'vL*', 'p0*']), ('R', rho_R, ['p1', 'vR', 'p1*', 'vR*'])):
        dense = rho.split_legs().transpose(labels).to_ndarray()
        want = c['rho_' + side]
        n = dense.shape[0] * dense.shape[1]
        lim = factor * c['mag_' + side].astype(np.float64).reshape(want.shape)
        err = np.abs(dense - want)
        assert np.all(err <= lim), "rho_%s: worst err / bound %.3g" % (side, float(np.max(err / np.maximum(lim, 1e-300))))
        worst = max(worst, float(np.max(err[lim > 0] / lim[lim > 0])))
        frob[side] = (float(np.linalg.norm(lim)), float(np.linalg.norm(want)), n)
        trace[side] = float(np.real(np.trace(want.reshape(n, n))))
    print("MIXER_GOLDEN %s rho max_err_over_bound=%.4f" % (c['name'], worst))

    def eig_bound(side):        # normalised eigenvalues: (header bound on |rho|_F + Weyl on the rho bound) / trace, both sides
        lim_f, rho_f, n = frob[side]
        fp = 4 if cplx else 1
        return 2 * ((6 * n + 16 * fp * (1 + 2 * np.sqrt(n))) * 2.0**-53 * np.sqrt(n) * rho_f + lim_f) / trace[side]
    eng = _Engine()
    eng.trunc_params, eng.eff_H = dict(c['trunc_params']), eff
    mix = mixer.DensityMatrixMixer({'amplitude': c['amplitude']})
    theta2 = eff.prepare_svd(eff.combine_theta(theta))
    U, S, VH, err, S_a = mix.svd_from_rho(eng, rho_L, rho_R, theta2, [c['qtotal_L'], None])
    assert U.shape[1] == c['n_keep_L'] and VH.shape[0] == c['n_keep_R'] and S.get_leg_labels() == ['vL', 'vR']
    tol = eig_bound('L')
    d_val = np.abs(np.sort(S_a**2)[::-1] - np.sort(c['S_approx_sq'])[::-1])
    print("MIXER_GOLDEN %s eigenvalues max err %.3g, bound %.3g; gap %.3g" % (c['name'], d_val.max(), tol, c['gap']))
    assert np.all(d_val <= tol)
    n_drop = frob['L'][2] - c['n_keep_L'] + frob['R'][2] - c['n_keep_R']
    assert abs(err.eps - c['err_eps']) <= n_drop * max(tol, eig_bound('R'))
    usv = npc.tensordot(npc.tensordot(U, S, axes=['vR', 'vL']), VH, axes=['vR', 'vL']).split_legs()
    d_usv = float(np.abs(usv.transpose(['vL', 'p0', 'p1', 'vR']).to_ndarray() - c['USV']).max())
    lim_usv = 10 * max(tol, eig_bound('R')) / c['gap']
    print("MIXER_GOLDEN %s U S VH max err %.3g, bound %.3g" % (c['name'], d_usv, lim_usv))
    assert d_usv <= lim_usv
    fp = 4 if cplx else 1
    for iso, contr, n in ((U, ['(vL*.p0*)', '(vL.p0)'], U.shape[0]), (VH, ['(p1*.vR*)', '(p1.vR)'], VH.shape[1])):
        G = npc.tensordot(iso.conj(), iso, axes=contr).to_ndarray()
        assert np.abs(G - np.eye(len(G))).max() <= 64 * fp * 2.0**-53 * np.sqrt(n)
