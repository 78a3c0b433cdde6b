"""``H + h.c.`` in the module form: the reference's engines (unedited) on MPOs with ``explicit_plus_hc`` under ``install(fused=True)``,
where ``SumNpcLinearOperator(eff_H, eff_H.adjoint())`` of a device operator becomes ``eff_H.plus_hc()`` -- one device operator on the
direct sum along the MPO bond.  CPU container only (the emulation of the device entry points; the reference tree does not exist on
the GPU box).  Run the way ``tests/test_reference_tdvp_fused.py`` runs its files, in one process each so that the counters of
``module_form.stats`` are those of the whole run.

* ``test_dmrg.py::test_dmrg_explicit_plus_hc`` (spin chain with Sz, mixer on, finite and infinite, against the full MPO to 1e-13);
* the ``+hc`` / ``-hc`` cases of ``test_tdvp.py`` (TDVP against TEBD; the model has no conserved charge, which the device classes take
  with ``TPA_MPO_ENTRY_APPLY=2``).

Both fail without ``plus_hc``: the counters do not exist, and the device classes refuse such environments."""
import ast
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from test_reference_suite import run_reference_tests  # noqa: E402

REF = build_ref.reference_root()
pytestmark = pytest.mark.skipif(REF is None or not os.path.isdir(os.path.join(REF, 'tests')), reason="reference tree not available")


def _cpu_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of H + h.c.: checked on the emulation")


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith('PLUS_HC_STATS ')][-1]
    return ast.literal_eval(line[len('PLUS_HC_STATS '):])


def _check(out, device_counters):
    assert ' passed' in out and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['plus_hc_device'] > 0
    assert all(st[k] > 0 for k in device_counters), "device operators were constructed"
    # No H + h.c. bond reached the reference's classes uncounted: the ordinary sums that were constructed (`plus_hc_other`) are exactly
    # the bonds that a device class handed back at construction (`plus_hc_reference` -- the bond at the right end of a finite chain,
    # whose boundary RP is stored in a leg order that the factored form does not take, with or without h.c.), what `plus_hc` itself
    # declined is counted (`plus_hc_declined` holds both), and the doubled device operator served the bulk.
    assert st['plus_hc_other'] == st['plus_hc_reference'] <= st['plus_hc_declined']
    assert 10 * st['plus_hc_declined'] <= st['plus_hc_device']
    return st


def test_reference_dmrg_explicit_plus_hc_with_fused_callers():
    _cpu_only()
    out = run_reference_tests(['test_dmrg.py', '-k', 'test_dmrg_explicit_plus_hc'], plugin='refsuite_plus_hc_plugin')
    st = _check(out, ['device'])
    assert st['plus_hc_declined'] == st['plus_hc_reference'], "plus_hc itself declines no bond of this model"


def test_reference_tdvp_plus_hc_with_fused_callers():
    _cpu_only()
    out = run_reference_tests(['test_tdvp.py', '-k', 'test_tdvp and hc'], plugin='refsuite_plus_hc_plugin',
                              extra_env={'TPA_MPO_ENTRY_APPLY': '2'})
    assert '4 passed' in out
    # (plus_hc declines the evolutions of the first sweep from the real product state, where one environment is complex already
    # and the other still real)
    _check(out, ['device', 'device_one', 'device_zero'])


def test_switch_off_restores_the_reference_route():
    """``TPA_PLUS_HC=0``: such environments go to the reference's classes as before -- same test, no doubled operator."""
    _cpu_only()
    out = run_reference_tests(['test_dmrg.py', '-k', 'test_dmrg_explicit_plus_hc and finite'], plugin='refsuite_plus_hc_plugin',
                              extra_env={'TPA_PLUS_HC': '0'})
    assert ' passed' in out and ' failed' not in out
    st = _stats(out)
    assert st['plus_hc_device'] == 0 and st['plus_hc_reference'] == st['plus_hc_other'] > 0
