"""pytest plugin (``-p refsuite_sample_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
points of ``tests/mock_sample.py`` on top (``tpa_sample_select_batch`` / ``tpa_sample_gather_batch``), and the counters of
``module_form.stats`` and ``sample.sample_stats`` printed at the end of the run as one line ``SAMPLE_STATS {...}`` (run without
workers: one process, one set of counters).  Test infrastructure only (``tests/test_reference_sample_fused.py``)."""
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
        import mock_sample
        mock_sample.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.networks.mps as ref_mps
    assert getattr(ref_mps.MPS.sample_measurements, '_tpa_wrapped', False)


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    from tenpy_amd.networks import sample
    st = {k: v for k, v in module_form.stats.items() if k.startswith('sample')}
    st.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in sample.sample_stats.items()})
    try:
        import mock_sample
        st['select_calls'] = mock_sample.calls['tpa_sample_select_batch']
        st['gather_calls'] = mock_sample.calls['tpa_sample_gather_batch']
    except ImportError:
        pass
    terminalreporter.write_line("SAMPLE_STATS %r" % (st,))


_activate()
