"""The walk of ``networks/moments.py`` against the reference's statements on the same device (``TPA_MPO_MOMENTS`` 1 against 0) on the
cases (a), (b), (c) and (e) of ``tests/golden/moments.pkl``, the number of MPO-step launches, and a forced ``memory`` decline."""
import pytest

from moments_fixtures import case, close, mobackend  # noqa: F401
from tenpy_amd.networks import measure, moments

CASES = ['xxz', 'hubbard', 'xxz_sorted', 'xxz_tebd']


def three(psi, H):
    return H.expectation_value(psi), H.variance(psi, 0.), H.variance(psi)


@pytest.mark.parametrize("name", CASES)
def test_route_on_against_off(mobackend, monkeypatch, name):
    rec, psi, H = case(name, mobackend)
    on = three(psi, H)
    assert moments.moments_stats['device'] == 3 and moments.moments_stats['reference'] == 0
    monkeypatch.setenv('TPA_MPO_MOMENTS', '0')
    off = three(psi, H)
    assert moments.moments_stats['device'] == 3 and set(moments.moments_stats['why']) == {'switched_off'}
    print("MOMENTS on/off %s: %r" % (name, [abs(a - b) for a, b in zip(on, off)]))
    assert close(on[0], off[0], off[0]) and close(on[1], off[1], off[1]) and close(on[2], off[2], off[1])


@pytest.mark.parametrize("name", CASES)
def test_one_mpo_step_launch_per_site_and_row_set(mobackend, monkeypatch, name):
    """With the product table every site of every row set is ONE launch of the MPO step (and two grouped GEMMs); ``variance(psi)``
    walks once with both row sets, ``variance(psi, 0.)`` with the pair rows alone."""
    rec, psi, H = case(name, mobackend)
    monkeypatch.setenv('TPA_MPO_MOMENTS_PAIR', 'product')
    H.variance(psi)
    st = moments.moments_stats
    assert st['walks'] == 1 and st['d2h'] == 1 and st['steps_1'] == st['steps_2'] == psi.L
    assert st['step_launches'] == 2 * psi.L and st['gemms'] == 4 * psi.L and st['modes'] == {'product': psi.L, 'two_pass': 0}
    moments.reset_stats()
    H.variance(psi, 0.)
    assert st['walks'] == 1 and st['steps_1'] == 0 and st['steps_2'] == st['step_launches'] == psi.L
    moments.reset_stats()
    monkeypatch.setenv('TPA_MPO_MOMENTS_PAIR', 'two_pass')
    H.variance(psi, 0.)
    assert st['steps_2'] == psi.L and st['step_launches'] == 2 * psi.L


def test_forced_memory_decline_returns_the_same_number(mobackend, monkeypatch):
    rec, psi, H = case('xxz', mobackend)
    want = H.variance(psi)
    monkeypatch.setattr(measure, '_budget', lambda: 0)
    moments.reset_stats()
    got = H.variance(psi)
    assert moments.moments_stats['device'] == 0 and moments.moments_stats['why'] == {'memory': 2}     # (the statements ask for <H> themselves)
    assert close(got, want, rec['H2']) and close(got, rec['var'], rec['H2'])
