"""The MPO moments in the module form: the reference's ``tests/test_mpo.py::test_MPO_var`` and ``::test_MPO_expectation_value``
(unedited) under ``install(fused=True)``, where ``MPO.expectation_value_finite`` and ``MPO.variance`` are wrapped in place and finite
chains run the walk of ``tenpy_amd/networks/moments.py``.  On the emulation (``mock``) and on the MI355X (``gpu``, where the reference
travels as the archive ``oracle/_ref``); one process per run, so that the counters are those of the whole run.  The criterion is the
reference's own: 1e-13 relative against exact diagonalisation.

* ``test_MPO_var`` (a chain without a charge: served with ``TPA_MPO_ENTRY_APPLY=2``): ``<H>``, ``variance(psi, 0.)`` and
  ``variance(psi)`` come from the walk, nothing is handed back;
* with the default ``TPA_MPO_ENTRY_APPLY`` the same test passes on the reference's statements, every call counted under ``plan``;
* ``test_MPO_expectation_value`` (infinite chains): counted under ``infinite``, the reference's methods run.

All fail without the wrapper: the plugin asserts that it is installed, and the counters do not exist."""
import ast
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from test_reference_suite import WHERE, _needs, run_reference_tests  # noqa: E402

REF = build_ref.reference_root()
pytestmark = pytest.mark.skipif(REF is None or not os.path.isdir(os.path.join(REF, 'tests')), reason="reference tree not available")


def run(test, **env):
    out = run_reference_tests(['test_mpo.py', '-k', test], plugin='refsuite_moments_plugin', extra_env=env)
    assert int(re.search(r'(\d+) passed', out).group(1)) == 1 and ' failed' not in out and ' error' not in out
    line = [l for l in out.splitlines() if l.startswith('MOMENTS_STATS ')][-1]
    st = ast.literal_eval(line[len('MOMENTS_STATS '):])
    print(st)
    return st


@pytest.mark.parametrize("where", WHERE)
def test_reference_test_MPO_var_on_the_walk(where):
    _needs(where)
    st = run('test_MPO_var', TPA_MPO_MOMENTS='1', TPA_MPO_ENTRY_APPLY='2')
    assert st['moments_device'] == st['device'] == st['walks'] == 3 and st['moments_device'] >= 2
    assert st['moments_reference'] == st['reference'] == 0 and st['why'] == {}
    assert st['steps_1'] == 2 * 8 and st['steps_2'] == 2 * 8 and st['d2h'] == 3


@pytest.mark.parametrize("where", WHERE)
def test_reference_test_MPO_var_declined_without_a_plan_class(where):
    _needs(where)
    st = run('test_MPO_var', TPA_MPO_MOMENTS='1', TPA_MPO_ENTRY_APPLY='1')
    assert st['moments_device'] == 0 and st['walks'] == 0
    assert st['moments_reference'] == st['reference'] == 4 and st['why'] == {'plan': 4}     # (``variance(psi)`` asks for <H> itself)


@pytest.mark.parametrize("where", WHERE)
def test_reference_test_MPO_expectation_value_is_counted_as_infinite(where):
    _needs(where)
    st = run('test_MPO_expectation_value', TPA_MPO_MOMENTS='1')
    assert st['moments_device'] == 0 and st['walks'] == 0
    assert st['moments_reference'] == st['reference'] >= 1 and set(st['why']) == {'infinite'}
