"""pytest plugin (``-p refsuite_ortho_plugin``): ``refsuite_plugin`` with ``install(fused=True)`` and, on the emulation, the entry
points of ``tests/mock_ortho.py`` (the fused excited-state callers reach ``tpa_lanczos_run_ex`` / ``tpa_project_out``; it installs
on top of ``mock_evolve``).  Importable as a plain module too (the script of ``tests/test_reference_excited_fused.py``).  Test
infrastructure only."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


class _Setter:
    """The part of pytest's monkeypatch that the emulations use, without undo (they stay for the session)."""
    @staticmethod
    def setattr(obj, name, value, raising=True):
        setattr(obj, name, value)


def _activate():
    import torch
    if not torch.cuda.is_available():
        import mock_ortho
        mock_ortho.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.algorithms.mps_common as ref_mc
    import tenpy_amd.linalg.sparse as dev_sparse
    assert ref_mc.OrthogonalNpcLinearOperator is dev_sparse.OrthogonalNpcLinearOperator


_activate()
