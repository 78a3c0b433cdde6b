"""Single-site DMRG in the module form: the reference's ``SingleSiteDMRGEngine`` (unedited) with ``SubspaceExpansion`` under
``install(fused=True)``, where ``mix_and_decompose_1site`` is wrapped in place and -- with a device ``OneSiteH`` -- served by
``mixer.device_expand_1site`` (one ``tpa_mpo_expand_batch`` launch).  CPU container only (the emulation of the device entry points; the
reference tree does not exist on the GPU box); one process per run so that the counters are those of the whole run.

* the reference's own ``test_dmrg.py`` cases for a finite single-site engine -- ``test_dmrg[finite-True-True-1]`` and
  ``test_dmrg_diag_method[SingleSiteDMRGEngine-ED_block]`` -- both set ``combine=True``, which the device ``OneSiteH`` hands back to the
  reference's class: they pass with the wrapper installed, every expansion counted as the reference's;
* the same cases, still unedited, with ``combine=False`` forced at the constructor of the reference's ``SingleSiteDMRGEngine`` by the
  plugin (``TPA_REFSUITE_1SITE_COMBINE=0``): the reference's own assertions pass and the expansions run on the device route, one
  ``tpa_mpo_expand_batch`` call each; the charged model (``test_dmrg_diag_method``, a spin chain with Sz) alone for the share of the
  device route.

All fail without the wrapper: the plugin asserts that it is installed, and the counters do not exist."""
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
        pytest.skip("module form of the subspace expansion: checked on the emulation")


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith('EXPAND_STATS ')][-1]
    return ast.literal_eval(line[len('EXPAND_STATS '):])


def test_reference_single_site_cases_pass_with_the_wrapper():
    _cpu_only()
    out = run_reference_tests(BOTH,
                              plugin='refsuite_expand_plugin', extra_env={'TPA_MPO_ENTRY_APPLY': '2'})
    import re
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 2 and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['expand_reference'] > 0 and st['reference_one'] > 0        # combine=True: the reference's OneSiteH and method
    assert st['expand_calls'] == st['expand_device'] == st['device_expand']


CHARGED = ['test_dmrg.py', '-k', 'test_dmrg_diag_method and SingleSiteDMRGEngine']
BOTH = ['test_dmrg.py', '-k', '(test_dmrg and finite-True-True-1 and not infinite) or (test_dmrg_diag_method and SingleSiteDMRGEngine)']


def test_reference_cases_with_combine_false_on_the_device_route():
    """The same two cases, unedited, with ``combine=False`` forced at the engine's constructor (the plugin): the reference's own
    assertions pass, the expansions run on the device route, one ``tpa_mpo_expand_batch`` call each."""
    _cpu_only()
    import re
    out = run_reference_tests(BOTH, plugin='refsuite_expand_plugin', extra_env={'TPA_MPO_ENTRY_APPLY': '2', 'TPA_REFSUITE_1SITE_COMBINE': '0'})
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 2 and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['combine_forced'] >= 2 and st['device_one'] > 0 and st['expand_device'] > 0
    assert st['expand_calls'] == st['expand_device'] == st['device_expand'], "one tpa_mpo_expand_batch call per device expansion"


def test_charged_reference_case_runs_mostly_on_the_device_route():
    _cpu_only()
    out = run_reference_tests(CHARGED, plugin='refsuite_expand_plugin', extra_env={'TPA_REFSUITE_1SITE_COMBINE': '0'})
    assert '1 passed' in out and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['expand_device'] > 0
    assert 10 * st['expand_reference'] <= st['expand_device'], "the bulk of the expansions of the charged model runs on the device route"
    assert st['expand_calls'] == st['expand_device'] == st['device_expand']
