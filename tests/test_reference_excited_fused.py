"""Excited states in the module form: the reference's engines (``tenpy/algorithms/dmrg.py``, ``mps_common.py``, unedited) under
``install(fused=True)``, which hands ``_wrap_ortho_eff_H`` the device ``OrthogonalNpcLinearOperator``.  CPU container only (the
emulation of the device entry points; the reference tree does not exist on the GPU box).

* the reference's own ``tests/test_dmrg.py`` (it contains the excited-state test) under the fused callers; this is also the test of
  ``module_form.DeviceTwoSiteH._device_ok`` handing infinite dipole-conserving bonds back to the reference's class:
  ``test_dmrg_dipole_conservation[2-infinite]`` of that file raised "incompatible LegCharge" in the device ``update_LP`` before;
* the reference's ``TwoSiteDMRGEngine`` with ``orthogonal_to=[psi0]`` on a small ``XXZChain``: the projected runs went through the
  native loop, and the energy of the same run under plain ``install()`` is reproduced to 1e-10."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402
from test_reference_suite import run_reference_tests  # noqa: E402

REF = build_ref.reference_root() or '/root/reference'
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'tests')), reason="reference tree not available")


def _cpu_only():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form of the excited-state search: checked on the emulation")


def test_reference_dmrg_tests_with_fused_callers():
    _cpu_only()
    out = run_reference_tests(['test_dmrg.py', '-n', '4'], plugin='refsuite_ortho_plugin')
    assert ' passed' in out and ' failed' not in out


SCRIPT = r"""
import sys, warnings
import numpy as np
fused = sys.argv[1] == 'fused'
if fused:
    import refsuite_ortho_plugin
else:
    import refsuite_plugin
warnings.simplefilter('ignore')
import tenpy.algorithms.mps_common as ref_mc
from tenpy.algorithms import dmrg
from tenpy.models.xxz_chain import XXZChain
from tenpy.networks.mps import MPS
from tenpy_amd.linalg import krylov_based as kb
from tenpy_amd.linalg import sparse as dev_sparse
assert (ref_mc.OrthogonalNpcLinearOperator is dev_sparse.OrthogonalNpcLinearOperator) == fused
L = 12
M = XXZChain(dict(L=L, Jxx=1., Jz=0.7, hz=0.2, bc_MPS='finite', sort_charge=True))
# diag_method lanczos: the engine diagonalises small bonds exactly otherwise (dmrg.py: full_diag_effH below N = 400)
pars = {'trunc_params': {'chi_max': 40, 'svd_min': 1.e-12}, 'max_sweeps': 6, 'min_sweeps': 6, 'mixer': None, 'combine': False,
        'diag_method': 'lanczos', 'lanczos_params': {'N_max': 20}}
psi0 = MPS.from_product_state(M.lat.mps_sites(), ['up', 'down'] * (L // 2), bc='finite')
E0, _ = dmrg.TwoSiteDMRGEngine(psi0, M, dict(pars)).run()
psi1 = MPS.from_product_state(M.lat.mps_sites(), ['down', 'up'] * (L // 2), bc='finite')
before = kb.stats['n_native_ortho']
E1, _ = dmrg.TwoSiteDMRGEngine(psi1, M, dict(pars), orthogonal_to=[psi0]).run()
print('NATIVE_ORTHO %d DECLINED %d' % (kb.stats['n_native_ortho'] - before, kb.stats['n_ortho_declined']))
print('OVERLAP %.3e' % abs(psi1.overlap(psi0)))
print('ENERGIES %.14f %.14f' % (E0, E1))
if fused:
    assert kb.stats['n_native_ortho'] > before
"""


def _run(mode):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([HERE, ROOT, REF, env.get('PYTHONPATH', '')])
    res = subprocess.run([sys.executable, '-c', SCRIPT, mode], env=env, capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('ENERGIES')][0]
    return [float(x) for x in line.split()[1:]], res.stdout


def test_reference_engine_reaches_the_native_loop_and_reproduces_the_energy():
    _cpu_only()
    (E0f, E1f), out = _run('fused')
    (E0p, E1p), _ = _run('plain')
    print(out)
    assert 'NATIVE_ORTHO' in out
    assert E1f > E0f + 1e-3
    assert abs(E0f - E0p) <= 1e-10 and abs(E1f - E1p) <= 1e-10
