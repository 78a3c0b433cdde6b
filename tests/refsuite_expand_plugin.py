"""pytest plugin (``-p refsuite_expand_plugin``): the reference's tests under ``install(fused=True)`` with, on the emulation, the entry
points of ``tests/mock_expand.py`` on top (``tpa_mpo_expand_batch``), and the counters of ``module_form.stats`` and the calls of the
emulated entry point printed at the end of the run as one line ``EXPAND_STATS {...}`` (run without workers: one process, one set of
counters).  ``TPA_REFSUITE_1SITE_COMBINE=0``: the reference's ``SingleSiteDMRGEngine`` gets ``combine=False`` whatever the case asks for.
Test infrastructure only (``tests/test_reference_1site_fused.py``)."""
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
        import mock_expand
        mock_expand.install(_Setter)
    import tenpy_amd.install as ti
    ti.install(fused=True)
    import tenpy
    import tenpy_amd.linalg.np_conserved as mirror
    assert tenpy.linalg.np_conserved is mirror, "import hook not active"
    import tenpy.algorithms.dmrg as ref_dmrg
    import tenpy.algorithms.mps_common as ref_mc
    from tenpy.tools.misc import find_subclass
    assert getattr(ref_mc.SubspaceExpansion.mix_and_decompose_1site, '_tpa_wrapped', False)
    assert find_subclass(ref_mc.Mixer, 'SubspaceExpansion') is ref_mc.SubspaceExpansion
    assert ref_dmrg.SingleSiteDMRGEngine.EffectiveH is ref_dmrg.OneSiteH and hasattr(ref_dmrg.OneSiteH, '_reference_class')
    if os.environ.get('TPA_REFSUITE_1SITE_COMBINE') == '0':
        # every finite single-site case of the reference's test_dmrg.py sets combine=True, which the device OneSiteH hands back to the
        # reference's class: run the same cases, unedited, with the option forced to False at the engine's constructor
        ref_init = ref_dmrg.SingleSiteDMRGEngine.__init__

        def init(self, psi, model, options, **kwargs):
            options['combine'] = False
            forced['n'] += 1
            ref_init(self, psi, model, options, **kwargs)
        ref_dmrg.SingleSiteDMRGEngine.__init__ = init


forced = {'n': 0}


def pytest_terminal_summary(terminalreporter):
    from tenpy_amd.algorithms import mixer, module_form
    st = dict(module_form.stats)
    st['mixer_why'] = dict(mixer.stats['why'])
    st['device_expand'] = mixer.stats['device_expand']
    st['combine_forced'] = forced['n']
    try:
        import mock_expand
        st['expand_calls'] = mock_expand.calls['tpa_mpo_expand_batch']
    except ImportError:
        pass
    terminalreporter.write_line("EXPAND_STATS %r" % (st,))


_activate()
