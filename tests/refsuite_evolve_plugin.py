"""pytest plugin (``-p refsuite_evolve_plugin``): ``refsuite_plugin`` with ``install(fused=True)`` and, on the emulation, the entry
points of ``tests/mock_evolve.py`` (the fused TDVP callers reach ``tpa_krylov_combine_z``).  Importable as a plain module too
(the script of ``tests/test_reference_tdvp_fused.py``).  Test infrastructure only."""
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
        import mock_evolve
        mock_evolve.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.algorithms.tdvp as ref_tdvp
    import tenpy_amd.linalg.krylov_based as kb
    assert ref_tdvp.LanczosEvolution is kb.LanczosEvolution and hasattr(ref_tdvp.OneSiteH, '_reference_class')


_activate()
