"""The density-matrix mixer in the module form: the reference's ``TwoSiteDMRGEngine`` (unedited) with the mixer on under
``install(fused=True)``, where ``DensityMatrixMixer.mix_rho`` is wrapped in place and -- with a device ``TwoSiteH`` -- served by
``mixer.device_mix_rho`` (one ``tpa_herk_chain`` launch per side).  CPU container only (the emulation of the device entry points; the
reference tree does not exist on the GPU box); one process per run so that the counters are those of the whole run.

* ``test_dmrg.py::test_dmrg`` finite, two sites, ``DensityMatrixMixer``: ``combine=True`` (fused ``TwoSiteH``) and ``combine=False``
  (factored); the model has no conserved charge, which the device classes take with ``TPA_MPO_ENTRY_APPLY=2``.  The reference's own
  assertions (energy against exact diagonalisation) are the check of the result;
* ``test_dmrg.py::test_dmrg_mixer_cleanup`` finite (a spin chain with Sz) and ``test_dmrg_explicit_plus_hc`` finite (half of H in the
  MPO, the operator is ``PlusHcH``; the reference asserts the energy of the full MPO to 1e-13).

All fail without the wrapper: the plugin asserts that it is installed, and the counter does not exist."""
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
        pytest.skip("module form of the mixer: checked on the emulation")


def _stats(out):
    line = [l for l in out.splitlines() if l.startswith('MIXER_STATS ')][-1]
    return ast.literal_eval(line[len('MIXER_STATS '):])


def test_reference_dmrg_with_mixer_on_the_device_route():
    _cpu_only()
    out = run_reference_tests(['test_dmrg.py', '-k', 'test_dmrg and not infinite and (finite-True-DensityMatrixMixer-2 or finite-False-True-2)'],
                              plugin='refsuite_mixer_plugin', extra_env={'TPA_MPO_ENTRY_APPLY': '2'})
    assert '2 passed' in out and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['device'] > 0 and st['mixer_device'] > 0
    assert st['herk_calls'] >= 2 * st['mixer_device']          # one launch per side (and one more where IdL / IdR is None)
    assert 10 * st['mixer_reference'] <= st['mixer_device'], "the bulk of the mixer calls runs on the device route"


def test_reference_mixer_cleanup_with_charges():
    _cpu_only()
    out = run_reference_tests(['test_dmrg.py', '-k', '(test_dmrg_mixer_cleanup or test_dmrg_explicit_plus_hc) and not infinite'],
                              plugin='refsuite_mixer_plugin')
    assert '2 passed' in out and ' failed' not in out
    st = _stats(out)
    print(st)
    assert st['mixer_device'] > 0 and st['herk_calls'] >= 2 * st['mixer_device']
    assert st['plus_hc_device'] > 0, "the H + h.c. run went through the doubled device operator"
    assert st['mixer_why'] == {}, "no call that reached device_mix_rho was declined"
