"""A model whose site has two states in one charge sector, in the module form: the reference's ``TwoSiteDMRGEngine``
(``tenpy/algorithms/dmrg.py``, unedited, ``combine=False``) on ``FermiHubbardChain`` with only N conserved (site sectors of widths
1, 2, 1) under ``install(fused=True)`` and under plain ``install()``.  CPU container only (the emulation of the device entry points;
the reference tree does not exist on the GPU box).

* the sweep energies of the two runs agree to 1e-10;
* the fused run handles its bonds with the device form (``module_form.stats['device'] > 0``), and no BULK bond is handed back to the
  reference's class -- bulk: a bond whose LP and RP carry the standard labels with the bra leg of LP before its ket leg and the ket
  leg of RP before its bra leg (``vR*`` before ``vR``, ``vL`` before ``vL*``), which is how every environment that the engine has
  contracted stores them.  The trivial right boundary (``init_RP``: ``vL*, wL, vL``) does not, so the last bond of the chain goes
  back to the reference's class -- for MPOs of single numbers just the same (``mps_common._envs_factorable``, unchanged here)."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import build_ref  # noqa: E402

REF = build_ref.reference_root() or '/root/reference'
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, 'tests')), reason="reference tree not available")

SCRIPT = r"""
import sys, warnings
import numpy as np
fused = sys.argv[1] == 'fused'
if fused:
    import refsuite_mpo_apply_plugin
else:
    import refsuite_plugin
warnings.simplefilter('ignore')
import tenpy.algorithms.mps_common as ref_mc
from tenpy.algorithms import dmrg
from tenpy.models.hubbard import FermiHubbardChain
from tenpy.networks.mps import MPS
from tenpy_amd.algorithms import module_form
L = 6
M = FermiHubbardChain(dict(L=L, t=1., U=4., mu=0., cons_N='N', cons_Sz=None, bc_MPS='finite'))
assert [int(b) for b in M.lat.mps_sites()[0].leg.get_block_sizes()] == [1, 2, 1]
log = []
if fused:
    cls = ref_mc.TwoSiteH
    assert hasattr(cls, '_reference_class')
    orig = cls._device_ok

    def spy(env, i0, combine):
        ok = orig(env, i0, combine)
        LP, RP = env.get_LP(i0), env.get_RP(i0 + 1)
        lp, rp = list(LP.get_leg_labels()), list(RP.get_leg_labels())
        bulk = (sorted(lp) == sorted(['vR*', 'wR', 'vR']) and sorted(rp) == sorted(['wL', 'vL', 'vL*']) and
                lp.index('vR*') < lp.index('vR') and rp.index('vL') < rp.index('vL*'))
        log.append((int(i0), bool(ok), bulk))
        return ok
    cls._device_ok = staticmethod(spy)
# diag_method lanczos: the engine diagonalises small bonds exactly otherwise (dmrg.py: full_diag_effH below N = 400)
pars = {'trunc_params': {'chi_max': 32, 'svd_min': 1.e-12}, 'max_sweeps': 4, 'min_sweeps': 4, 'mixer': None, 'combine': False,
        'diag_method': 'lanczos', 'lanczos_params': {'N_max': 20}}
psi = MPS.from_product_state(M.lat.mps_sites(), ['up', 'down'] * (L // 2), bc='finite')
eng = dmrg.TwoSiteDMRGEngine(psi, M, dict(pars))
eng.run()
print('ENERGIES ' + ' '.join('%.14f' % e for e in eng.sweep_stats['E']))
print('DEVICE %d REFERENCE %d' % (module_form.stats['device'], module_form.stats['reference']))
print('BULK_HANDED_BACK %d OF %d' % (sum(1 for _, ok, bulk in log if bulk and not ok), sum(1 for _, _, bulk in log if bulk)))
"""


def _run(mode):
    env = dict(os.environ)
    env['PYTHONPATH'] = os.pathsep.join([HERE, ROOT, REF, env.get('PYTHONPATH', '')])
    res = subprocess.run([sys.executable, '-c', SCRIPT, mode], env=env, capture_output=True, text=True, timeout=1200)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith('ENERGIES')][0]
    return [float(x) for x in line.split()[1:]], res.stdout


def test_reference_engine_on_a_block_mpo_runs_the_device_form():
    import torch
    if torch.cuda.is_available():
        pytest.skip("module form on the reference tree: checked on the emulation")
    Ef, out = _run('fused')
    Ep, _ = _run('plain')
    print(out)
    assert len(Ef) == len(Ep) >= 2
    assert max(abs(a - b) for a, b in zip(Ef, Ep)) <= 1e-10
    dev_line = [ln for ln in out.splitlines() if ln.startswith('DEVICE')][0].split()
    assert int(dev_line[1]) > 0
    bulk = [ln for ln in out.splitlines() if ln.startswith('BULK_HANDED_BACK')][0].split()
    assert int(bulk[3]) > 0 and int(bulk[1]) == 0
