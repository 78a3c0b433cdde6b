"""pytest plugin (``-p refsuite_moments_plugin``): the reference's tests under ``install(fused=True)`` -- on the emulation with every
emulated entry point (``tests/mock_sample.py`` stacks them all) -- and the counters of ``module_form.stats`` and
``moments.moments_stats`` printed at the end of the run as one line ``MOMENTS_STATS {...}`` (run without workers: one process, one set
of counters).  Test infrastructure only (``tests/test_reference_moments_fused.py``)."""
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
    import tenpy.networks.mpo as ref_mpo
    assert getattr(ref_mpo.MPO.expectation_value_finite, '_tpa_wrapped', False)
    assert getattr(ref_mpo.MPO.variance, '_tpa_wrapped', False)


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    from tenpy_amd.networks import moments
    st = {k: v for k, v in module_form.stats.items() if k.startswith('moments')}
    st.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in moments.moments_stats.items()})
    terminalreporter.write_line("MOMENTS_STATS %r" % (st,))


_activate()
