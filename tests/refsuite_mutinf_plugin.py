"""pytest plugin (``-p refsuite_mutinf_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
point of ``tests/mock_rho.py`` on top (``tpa_site_rho_batch``), and the counters of ``module_form.stats`` and ``rho.rho_stats`` printed
at the end of the run as one line ``MUTINF_STATS {...}`` (run without workers: one process, one set of counters).  Test infrastructure
only (``tests/test_reference_mutinf_fused.py``)."""
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
        import mock_rho
        mock_rho.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.networks.mps as ref_mps
    assert getattr(ref_mps.MPS.mutinf_two_site, '_tpa_wrapped', False)
    from tenpy.networks.purification_mps import PurificationMPS
    assert not getattr(PurificationMPS.mutinf_two_site, '_tpa_wrapped', False)


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    from tenpy_amd.networks import rho
    st = {k: v for k, v in module_form.stats.items() if k.startswith('mutinf')}
    st.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in rho.rho_stats.items()})
    try:
        import mock_rho
        st['site_rho_calls'] = mock_rho.calls['tpa_site_rho_batch']
    except ImportError:
        pass
    terminalreporter.write_line("MUTINF_STATS %r" % (st,))


_activate()
