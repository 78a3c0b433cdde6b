"""The stand-alone ``MPS.correlation_function`` / ``MPS.expectation_value`` against what the reference returned on the recorded states of
``tests/golden/measure.pkl`` (``make_golden_measure.py``): XXZ with a staggered field (Sz Sz, and the charged pair Sp Sm), spinless
fermions with the Jordan-Wigner string (Cd C), the TFI chain without a charge, and the complex XXZ state after a quench.  On the numpy
emulation (``mock``) and on the MI355X (``gpu``).  Tolerance: 1e-12 absolute, the project's golden tolerance (the values are O(1), every
one a sum of at most a few thousand products of numbers below 1 in float64)."""
import numpy as np
import pytest

from measure_fixtures import build_psi, golden, mbackend  # noqa: F401
from tenpy_amd.networks import measure

TOL = 1.e-12
NAMES = ['xxz', 'fermions', 'tfi', 'xxz_tebd']
_psi = {}


def state(name, backend):
    """The recorded state, built once per backend."""
    key = (name, backend)
    if key not in _psi:
        rec = [r for r in golden() if r['name'] == name][0]
        _psi[key] = (rec, build_psi(rec))
    return _psi[key]


def call(psi, rec, c, **over):
    kw = dict(sites1=c['sites1'], sites2=c['sites2'], str_on_first=c['str_on_first'], hermitian=c['hermitian'],
              opstr=None if c['opstr'] is None else rec['ops'][c['opstr']])
    kw.update(over)
    return psi.correlation_function(rec['ops'][c['op1']], rec['ops'][c['op2']], **kw)


@pytest.fixture
def stacked(monkeypatch):
    monkeypatch.setattr(measure, 'MEASURE', True)
    measure.reset_stats()


@pytest.mark.parametrize("name", NAMES)
def test_correlation_functions_match_the_reference(mbackend, stacked, name):
    rec, psi = state(name, mbackend)
    for c in rec['corr']:
        got = call(psi, rec, c)
        err = float(np.max(np.abs(got - c['result'])))
        print("MEASURE golden %s %s %s sites1=%s hermitian=%s str_on_first=%s: max abs err %.3g"
              % (name, c['op1'], c['op2'], c['sites1'], c['hermitian'], c['str_on_first'], err))
        assert got.shape == c['result'].shape and err <= TOL
    assert measure.measure_stats['device'] >= len(rec['corr']) and measure.measure_stats['generic'] == 0
    assert measure.measure_stats['kernel_launches'] > 0


@pytest.mark.parametrize("name", NAMES)
def test_expectation_values_match_the_reference(mbackend, stacked, name):
    """The list form (one launch per site for all operators) against the reference and against the per-operator calls."""
    rec, psi = state(name, mbackend)
    names = sorted(rec['expval'])
    n0 = measure.measure_stats['kernel_launches']
    got = psi.expectation_value([rec['ops'][n] for n in names])
    assert measure.measure_stats['kernel_launches'] - n0 == psi.L and measure.measure_stats['d2h'] == 1
    for n, g in zip(names, got):
        assert np.max(np.abs(g - rec['expval'][n])) <= TOL
        one = psi.expectation_value(rec['ops'][n])
        assert np.max(np.abs(g - one)) <= TOL
    sub = psi.expectation_value([rec['ops'][names[0]]], sites=[5, 2])
    assert np.max(np.abs(sub[0] - rec['expval'][names[0]][[5, 2]])) <= TOL


@pytest.mark.parametrize("name", ['xxz', 'fermions', 'xxz_tebd'])
def test_hermitian_is_the_conjugate_of_the_upper_triangle(mbackend, stacked, name):
    """``hermitian=True``: the lower triangle is the conjugate transpose of the upper one, bit for bit."""
    rec, psi = state(name, mbackend)
    for c in rec['corr']:
        if not c['hermitian']:
            continue
        got = np.asarray(call(psi, rec, c))
        iu = np.triu_indices(psi.L, 1)
        low, up = np.ascontiguousarray(got.T[iu]), np.ascontiguousarray(got[iu])
        if np.iscomplexobj(got):
            assert np.array_equal(low.real.view(np.uint64), up.real.view(np.uint64))
            assert np.array_equal(low.imag.view(np.uint64), (-up.imag).view(np.uint64))
        else:       # (all imaginary parts vanished: the matrix came back real)
            assert np.array_equal(low.view(np.uint64), up.view(np.uint64))


@pytest.mark.parametrize("name", NAMES)
def test_stacked_route_agrees_with_the_generic_statements(mbackend, monkeypatch, name):
    """``TPA_MEASURE=0`` (the row-by-row statements) and the stacked route agree to 1e-12; the former launches no kernel of the latter."""
    rec, psi = state(name, mbackend)
    for c in rec['corr']:
        monkeypatch.setattr(measure, 'MEASURE', True)
        a = call(psi, rec, c)
        monkeypatch.setattr(measure, 'MEASURE', False)
        measure.reset_stats()
        b = call(psi, rec, c)
        assert measure.measure_stats['kernel_launches'] == 0 and measure.measure_stats['why'] == {'switched_off': 2 if c['hermitian'] else 3}       # (the triangles and the diagonal)
        assert np.max(np.abs(a - b)) <= TOL and np.max(np.abs(b - c['result'])) <= TOL
