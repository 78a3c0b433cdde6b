"""pytest plugin (``-p refsuite_measure_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
point of ``tests/mock_measure.py`` on top (``tpa_site_inner_batch``), and the counters of ``module_form.stats`` and
``measure.measure_stats`` printed at the end of the run as one line ``MEASURE_STATS {...}`` (run without workers: one process, one set
of counters).  Test infrastructure only (``tests/test_reference_measure_fused.py``)."""
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
        import mock_measure
        mock_measure.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.networks.mps as ref_mps
    assert getattr(ref_mps.BaseMPSExpectationValue.correlation_function, '_tpa_wrapped', False)
    assert getattr(ref_mps.BaseMPSExpectationValue.expectation_value, '_tpa_wrapped', False)


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    from tenpy_amd.networks import measure
    st = {k: v for k, v in module_form.stats.items() if k.startswith('measure')}
    st.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in measure.measure_stats.items()})
    try:
        import mock_measure
        st['site_inner_calls'] = mock_measure.calls['tpa_site_inner_batch']
    except ImportError:
        pass
    terminalreporter.write_line("MEASURE_STATS %r" % (st,))


_activate()
