"""pytest plugin (``-p refsuite_mpo_apply_plugin``): ``refsuite_ortho_plugin`` with, on the emulation, the entry points of
``tests/mock_mpo_apply.py`` on top (the fused callers reach ``tpa_mpo_apply_batch`` and op kind 5 of the launch programs for models
whose site has several states per charge sector).  Importable as a plain module too (the script of
``tests/test_reference_blocks_fused.py``).  Test infrastructure only."""
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
        import mock_mpo_apply
        mock_mpo_apply.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"


_activate()
