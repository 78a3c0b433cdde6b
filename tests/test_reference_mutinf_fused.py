"""Mutual information in the module form: the reference's ``MPS.mutinf_two_site`` (unedited callers) under ``install(fused=True)``,
where it is wrapped in place and the density matrices come from the stacked walk of ``tenpy_amd/networks/rho.py``.  CPU container only
(the emulation of the device entry points; the reference tree does not exist on the GPU box); one process per run so that the counters
are those of the whole run.

* the reference's own ``test_mps.py`` passes with the wrapper -- ``test_singlet_mps`` among its tests wants the mutual information of
  singlet pairs to 14 decimals, which is why the eigenvalues are taken per charge block;
* calls served by the device route > 0, and every one of its kernel launches reached the emulated entry point;
* every call handed back to the reference's method has a counted reason;
* ``test_purification.py`` still passes: ``PurificationMPS`` keeps its own method.

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
from test_reference_suite import run_reference_tests  # noqa: E402

REF = build_ref.reference_root()
pytestmark = pytest.mark.skipif(REF is None or not os.path.isdir(os.path.join(REF, 'tests')), reason="reference tree not available")


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith('MUTINF_STATS ')][-1]
    return ast.literal_eval(line[len('MUTINF_STATS '):])


def test_reference_test_mps_on_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of the mutual-information route: checked on the emulation")
    out = run_reference_tests(['test_mps.py'], plugin='refsuite_mutinf_plugin', extra_env={'TPA_MUTINF': '1'})
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 30 and ' failed' not in out and ' error' not in out
    st = _stats(out)
    print(st)
    assert st['mutinf_device'] > 0 and st['kernel_launches'] > 0 and st['kernel_launches'] == st['site_rho_calls']
    assert st['mutinf_device'] == st['device'] and st['walks'] >= st['mutinf_device'] and st['d2h'] == st['walks']
    assert st['mutinf_reference'] == sum(st['why'].values()) == st['generic']
    assert 0 < st['slots'] < st['slots_full']


def test_reference_test_purification_keeps_its_own_method():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of the mutual-information route: checked on the emulation")
    out = run_reference_tests(['test_purification.py'], plugin='refsuite_mutinf_plugin', extra_env={'TPA_MUTINF': '1'})
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 5 and ' failed' not in out and ' error' not in out
    st = _stats(out)
    assert st['mutinf_device'] == 0 and st['kernel_launches'] == 0
