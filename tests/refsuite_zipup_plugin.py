"""pytest plugin (``-p refsuite_zipup_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
points of ``tests/mock_mpo_cell.py`` on top (``tpa_mpo_cell_apply_batch``), and the counters of ``module_form.stats``,
``mps_common.zipup_stats`` and the calls of the emulated MPO-step entry points printed at the end of the run as one line
``ZIPUP_STATS {...}`` (run without workers: one process, one set of counters).  Test infrastructure only
(``tests/test_reference_zipup_fused.py``)."""
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
        import mock_mpo_cell
        mock_mpo_cell.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.networks.mpo as ref_mpo
    assert getattr(ref_mpo.MPO.apply_zipup, '_tpa_wrapped', False)


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form, mps_common
    st = {k: v for k, v in module_form.stats.items() if k.startswith('zipup')}
    st.update({'step_' + k: (dict(v) if isinstance(v, dict) else v) for k, v in mps_common.zipup_stats.items()})
    try:
        import mock_expand
        import mock_mpo_cell
        st['cell_calls'] = mock_mpo_cell.calls['tpa_mpo_cell_apply_batch']
        st['expand_calls'] = mock_expand.calls['tpa_mpo_expand_batch']
    except ImportError:
        pass
    terminalreporter.write_line("ZIPUP_STATS %r" % (st,))


_activate()
