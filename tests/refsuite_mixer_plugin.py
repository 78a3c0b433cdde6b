"""pytest plugin (``-p refsuite_mixer_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
points of ``tests/mock_mixer.py`` on top (``tpa_herk_chain``), and the counters of ``module_form.stats`` and the calls of the
emulated entry point printed at the end of the run as one line ``MIXER_STATS {...}`` (run without ``-n``: one process, one set of
counters).  Test infrastructure only (``tests/test_reference_mixer_fused.py``)."""
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
        import mock_mixer
        mock_mixer.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.algorithms.mps_common as ref_mc
    from tenpy.tools.misc import find_subclass
    assert getattr(ref_mc.DensityMatrixMixer.mix_rho, '_tpa_wrapped', False)
    assert find_subclass(ref_mc.Mixer, 'DensityMatrixMixer') is ref_mc.DensityMatrixMixer


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import module_form
    st = dict(module_form.stats)
    from tenpy_amd.algorithms import mixer
    st['mixer_why'] = dict(mixer.stats['why'])
    try:
        import mock_mixer
        st['herk_calls'] = mock_mixer.calls['tpa_herk_chain']
    except ImportError:
        pass
    terminalreporter.write_line("MIXER_STATS %r" % (st,))


_activate()
