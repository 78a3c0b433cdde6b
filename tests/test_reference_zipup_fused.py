"""Applying an MPO to an MPS in the module form: the reference's ``MPO.apply`` / ``ExpMPOEvolution`` (unedited) with
``compression_method='zip_up'`` under ``install(fused=True)``, where ``MPO.apply_zipup`` is wrapped in place and the matrix of every
interior site comes from ``mps_common.device_zipup_step`` (one GEMM over chi and the MPO step).  CPU container only (the emulation of
the device entry points; the reference tree does not exist on the GPU box); one process per run so that the counters are those of the
whole run.

* the reference's own ``test_mpo.py::test_apply_mpo[zip_up]`` and the ``zip_up`` cases of ``test_time_evolution.py`` pass with the wrapper;
* device steps > 0; every device step issued the launches of exactly one MPO-step apply (one or two calls of the emulated entry points:
  the cell-dense launch and / or the entry-by-entry launch; ``TPA_MPO_CELL=2``: one cell-dense call at least per step);
* steps by the reference's statements occur only at the two boundary sites of a pass or with a counted reason.

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

CASES = ['test_mpo.py', 'test_time_evolution.py', '-k', '(test_apply_mpo and zip_up) or (test_time_evolution and zip_up)']


def _cpu_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of the zip-up application: checked on the emulation")


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith('ZIPUP_STATS ')][-1]
    return ast.literal_eval(line[len('ZIPUP_STATS '):])


@pytest.mark.parametrize("mode", ['0', '2'])
def test_reference_zip_up_cases_on_the_device_route(mode):
    _cpu_only()
    out = run_reference_tests(CASES, plugin='refsuite_zipup_plugin', extra_env={'TPA_MPO_CELL': mode, 'TPA_MPO_ENTRY_APPLY': '2'})
    assert int(re.search(r'(\d+) passed', out).group(1)) >= 3 and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['zipup_device'] > 0 and st['zipup_device'] == st['step_device_steps']
    # one MPO-step apply per device step: its launches, nothing else
    assert st['step_cell_launches'] + st['step_entry_launches'] == st['cell_calls'] + st['expand_calls']
    assert st['zipup_device'] <= st['cell_calls'] + st['expand_calls'] <= 2 * st['zipup_device']
    if mode == '0':
        assert st['cell_calls'] == 0 and st['expand_calls'] == st['zipup_device']
    else:
        assert st['cell_calls'] == st['zipup_device']
    # the reference's statements: the two boundary sites of a pass, or a counted reason
    assert st['zipup_boundary'] > 0 and st['zipup_boundary'] % 2 == 0
    assert st['step_declined'] == sum(st['step_why'].values())
    assert st['zipup_reference'] - st['zipup_boundary'] == st['step_declined'] - st['zipup_handed_back']      # (a pass handed back: one decline)
