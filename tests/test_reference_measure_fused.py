"""Measurement in the module form: the reference's ``MPS.correlation_function`` / ``MPS.expectation_value`` (unedited) under
``install(fused=True)``, where both are wrapped in place and the rows of a correlation matrix come from the stacked walk of
``tenpy_amd/networks/measure.py``.  CPU container only (the emulation of the device entry points; the reference tree does not exist
on the GPU box); one process per run so that the counters are those of the whole run.

* the reference's own ``test_mps.py`` passes with the wrappers;
* calls served by the device route > 0, and every one of its kernel launches reached the emulated entry point;
* every call handed back to the reference's statements has a counted reason.

All fail without the wrappers: the plugin asserts that they are installed, and the counters do not exist."""
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
    line = [l for l in out.splitlines() if l.startswith('MEASURE_STATS ')][-1]
    return ast.literal_eval(line[len('MEASURE_STATS '):])


def test_reference_test_mps_on_the_device_route():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of the measurement route: checked on the emulation")
    out = run_reference_tests(['test_mps.py'], plugin='refsuite_measure_plugin', extra_env={'TPA_MEASURE': '1'})
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 30 and ' failed' not in out and ' error' not in out
    st = _stats(out)
    print(st)
    assert st['measure_device'] > 0 and st['kernel_launches'] > 0 and st['kernel_launches'] == st['site_inner_calls']
    assert st['measure_device'] == st['device'] and st['walks'] > 0 and st['d2h'] <= st['measure_device']
    assert st['measure_reference'] == sum(st['why'].values()) and st['generic'] == 0
    assert st['capacity'] - st['filled'] <= 0.25 * st['capacity']
