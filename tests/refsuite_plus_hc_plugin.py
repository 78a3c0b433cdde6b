"""pytest plugin (``-p refsuite_plus_hc_plugin``): ``refsuite_mpo_apply_plugin`` with, on the emulation, the entry points of
``tests/mock_mpo_entry.py`` on top (with ``TPA_MPO_ENTRY_APPLY=2`` the fused callers take MPOs without a conserved charge), and the
counters of ``module_form.stats`` printed at the end of the run as one line ``PLUS_HC_STATS {...}`` (run without ``-n``: one process,
one set of counters).  Test infrastructure only (``tests/test_reference_plus_hc_fused.py``)."""
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
        import mock_mpo_entry
        mock_mpo_entry.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.algorithms.mps_common as ref_mc
    import tenpy.algorithms.tdvp as ref_tdvp
    assert hasattr(ref_mc.SumNpcLinearOperator, '_reference_class') and ref_tdvp.SumNpcLinearOperator is ref_mc.SumNpcLinearOperator


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    terminalreporter.write_line("PLUS_HC_STATS %r" % (dict(module_form.stats),))


_activate()
