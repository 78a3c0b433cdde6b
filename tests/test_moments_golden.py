"""The stand-alone ``MPO.expectation_value`` and ``MPO.variance`` against what the reference returned, on the recorded cases of
``tests/golden/moments.pkl`` (``make_golden_moments.py``: scalar, block and entry plan, a chain without a charge, complex tensors, a
product state, two sites).  On the numpy emulation (``mock``) and on the MI355X (``gpu``).

Tolerance: the project's golden ``TOL = 1e-12`` times ``max(1, |value|)`` for ``<H>`` and ``<H^2>``; for ``variance(psi)`` itself
``TOL max(1, <H^2>)``, because it is the difference of two such numbers.  ``test_generic_statements_stay_inside_the_bound`` checks
that the reference's statements, recomputed on the mirror, stay inside these bounds for every case.

Fails without the feature with ``AttributeError`` (the stand-alone ``MPO`` has neither method)."""
import numpy as np
import pytest

from moments_fixtures import NAMES, case, close, mobackend  # noqa: F401
from tenpy_amd.algorithms import mps_common
from tenpy_amd.networks import moments


def check(rec, E, H2, var, tag):
    print("MOMENTS golden %s %s: dE %.3g dH2 %.3g dvar %.3g (H2 %.6g)" % (rec['name'], tag, abs(E - rec['E']), abs(H2 - rec['H2']),
                                                                         abs(var - rec['var']), abs(rec['H2'])))
    assert close(E, rec['E'], rec['E']) and close(H2, rec['H2'], rec['H2']) and close(var, rec['var'], rec['H2'])
    for v, w in ((E, rec['E']), (H2, rec['H2']), (var, rec['var'])):
        assert np.iscomplexobj(v) == np.iscomplexobj(w)


@pytest.mark.parametrize("pair", ['auto', 'product', 'two_pass'])
@pytest.mark.parametrize("name", [n for n in NAMES if n != 'tfi'])
def test_walk_matches_the_reference(mobackend, monkeypatch, name, pair):
    rec, psi, H = case(name, mobackend)
    monkeypatch.setenv('TPA_MPO_MOMENTS_PAIR', pair)
    E, H2, var = H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi)
    check(rec, E, H2, var, pair)
    st = moments.moments_stats
    assert st['device'] == 3 and st['reference'] == 0 and st['walks'] == 3 and st['d2h'] == 3
    assert st['steps_1'] == 2 * psi.L and st['steps_2'] == 2 * psi.L      # (``variance(psi)``: both row sets from one walk)
    family = {'xxz': mps_common.MpoApplyPlan, 'hubbard': mps_common.MpoBlockApplyPlan, 'xxz_sorted': mps_common.MpoEntryApplyPlan}
    if name in family:
        assert all(mps_common.MpoPairPlan.family(H.get_W(i)) is family[name] for i in range(1, H.L - 1))


def test_chain_without_a_charge(mobackend, monkeypatch):
    """Case (d): served by the entry plan with ``ENTRY_APPLY = 2``; by default there is no plan class for such an MPO and the call
    runs the reference's statements with the reason ``plan``."""
    rec, psi, H = case('tfi', mobackend)
    check(rec, H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi), 'declined')
    assert moments.moments_stats['device'] == 0 and moments.moments_stats['why'] == {'plan': 4}     # (``variance(psi)`` asks for <H> itself)
    monkeypatch.setattr(mps_common, 'ENTRY_APPLY', 2)
    moments.reset_stats()
    check(rec, H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi), 'entry')
    assert moments.moments_stats['device'] == 3 and moments.moments_stats['reference'] == 0


@pytest.mark.parametrize("name", NAMES)
def test_generic_statements_stay_inside_the_bound(mobackend, monkeypatch, name):
    """The reference's statements on the mirror (``TPA_MPO_MOMENTS=0``) against the recorded values: the bound leaves room."""
    rec, psi, H = case(name, mobackend)
    monkeypatch.setenv('TPA_MPO_MOMENTS', '0')
    check(rec, H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi), 'generic')
    assert moments.moments_stats['device'] == 0 and set(moments.moments_stats['why']) == {'switched_off'}


def test_errors_are_the_references(mobackend):
    from tenpy_amd.networks.mpo import MPO
    rec, psi, H = case('xxz', mobackend)
    _, psi2, _ = case('two_sites', mobackend)
    with pytest.raises(ValueError, match='expect same L'):
        H.variance(psi2)
    half = MPO(H.p_legs, H._W, H.IdL, H.IdR, explicit_plus_hc=True)
    with pytest.raises(NotImplementedError, match='explicit_plus_hc'):
        half.variance(psi)
    E = half.expectation_value(psi)         # declined: <H> + conj(<H>) from the environment
    assert close(E, 2 * rec['E'], 2 * rec['E']) and moments.moments_stats['why'] == {'plus_hc': 1}
