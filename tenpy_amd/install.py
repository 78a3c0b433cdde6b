"""Run an UNMODIFIED TeNPy on device-resident Arrays: ``import tenpy_amd.install as ti; ti.install(); import tenpy``.

``north_star``: "keeping the tenpy.linalg.np_conserved Array API and ChargeInfo/LegCharge bookkeeping so
algorithms/dmrg.py and algorithms/tebd.py run unchanged".  TeNPy's callers only ever reach block data through the
``np_conserved`` / ``charges`` API (nothing in algorithms/ or networks/mps.py touches ``_data``), so the whole
backend swap is an *import hook*: when the interpreter is asked for ``tenpy.linalg.np_conserved`` or
``tenpy.linalg.charges`` it is handed ``tenpy_amd.linalg.np_conserved`` / ``.charges`` instead -- the API mirror whose
``Array`` keeps its blocks in one HBM arena and whose workers are the HIP kernels behind ``include/tenpy_amd.h``.
Everything else (``tenpy.algorithms``, ``tenpy.networks``, ``tenpy.models``, ``tenpy.linalg.krylov_based``,
``truncation``, ``sparse`` ...) is the reference's own code, imported from wherever TeNPy is installed and run as is.

The reference ships its own replacement hook, ``tools/optimization.py:262 use_cython``, which looks functions up in
``tenpy.linalg._npc_helper``; it is evaluated inside the two modules replaced here, so with the mirror in place it is
never consulted (``have_cython_functions`` is set to ``False``, the state the reference itself reaches with
``TENPY_NO_CYTHON=1``, optimization.py:322).  The fine-grained form of the boundary -- the 16 ``use_cython`` names for
a TeNPy that keeps its own ``np_conserved`` -- is ``tenpy_amd/_npc_helper.py``.

``install(fused=True)`` additionally rebinds, after ``import tenpy``, the callers for which the device has a
fused form: ``LanczosGroundState`` (one fused recurrence kernel per step instead of four BLAS-1 calls), ``TwoSiteH``
(cached plans; factored matvec LP . theta . W0 W1 . RP for ``combine=False``), the bond hint of the warm-started block
SVD, ``OrthogonalNpcLinearOperator`` (the projections of an excited-state search inside the native Krylov loop), and for TDVP ``LanczosEvolution`` (one native loop and one combination pass per evolution) with the device ``OneSiteH`` /
``ZeroSiteH``, the subspace expansion of ``SingleSiteDMRGEngine`` (one ``tpa_mpo_expand_batch`` launch with a device ``OneSiteH``), and ``SumNpcLinearOperator`` (``H + h.c.`` of an MPO with ``explicit_plus_hc`` as one device operator); see
:func:`use_fused_callers`.
"""
import importlib
import importlib.abc
import importlib.machinery
import sys

__all__ = ['install', 'uninstall', 'installed', 'use_fused_callers']

_SUBST = {
    'tenpy.linalg.np_conserved': 'tenpy_amd.linalg.np_conserved',
    'tenpy.linalg.charges': 'tenpy_amd.linalg.charges',
}


class _MirrorLoader(importlib.abc.Loader):
    def __init__(self, target):
        self.target = target

    def create_module(self, spec):
        mod = importlib.import_module(self.target)
        self._orig_spec = getattr(mod, '__spec__', None)
        return mod

    def exec_module(self, module):
        # the import system has overwritten __spec__ / left __name__ alone; keep the mirror's own identity
        module.__spec__ = self._orig_spec
        # the reference evaluates @use_cython while importing the two modules replaced here and asserts afterwards
        # that somebody did (linalg/__init__.py:74); record "no compiled helper", like TENPY_NO_CYTHON=1
        from tenpy.tools import optimization
        if optimization.have_cython_functions is None:
            optimization.have_cython_functions = False


class _MirrorFinder(importlib.abc.MetaPathFinder):
    def find_spec(self, fullname, path=None, target=None):
        tgt = _SUBST.get(fullname)
        if tgt is None:
            return None
        return importlib.machinery.ModuleSpec(fullname, _MirrorLoader(tgt))


_finder = None


def installed():
    return _finder is not None


def install(fused=False):
    """Register the import hook.  Must run before the first ``import tenpy`` (raises otherwise: a TeNPy that has
    already bound its own ``np_conserved`` in dozens of module namespaces cannot be re-pointed reliably)."""
    global _finder
    if _finder is None:
        for name in _SUBST:
            if name in sys.modules and sys.modules[name].__name__ != _SUBST[name]:
                raise RuntimeError("tenpy was imported before tenpy_amd.install.install(); call install() first")
        _finder = _MirrorFinder()
        sys.meta_path.insert(0, _finder)
    if fused:
        use_fused_callers()


def uninstall():
    """Remove the hook and forget every ``tenpy`` module, so that a later ``import tenpy`` is the plain CPU TeNPy."""
    global _finder
    if _finder is not None:
        sys.meta_path.remove(_finder)
        _finder = None
    for name in [n for n in sys.modules if n == 'tenpy' or n.startswith('tenpy.')]:
        del sys.modules[name]


def use_fused_callers():
    """Optional, after the hook: rebind, in the reference's modules, the callers for which the device has a fused form.
    The engines themselves (``algorithms/dmrg.py``, ``mps_common.py`` sweeps, mixers, ``tebd.py``) remain the reference's code.

    * ``LanczosGroundState`` (``linalg/krylov_based.py:645``; constructed at ``dmrg.py:740/742``) -> the fused device recurrence
      of ``tenpy_amd/linalg/krylov_based.py`` (same options, same results, one kernel per Krylov step);
    * ``TwoSiteH`` (``algorithms/mps_common.py:1245``; ``TwoSiteDMRGEngine.EffectiveH``, ``dmrg.py:865``) -> the device form of
      ``tenpy_amd/algorithms/module_form.py`` (cached plans, fused ``LHeff`` build; ``combine=False``: factored matvec), which
      hands bonds it does not cover back to the reference's class;
    * ``TwoSiteDMRGEngine.mixed_svd`` (``dmrg.py:876``) is wrapped to pass the bond index to the block SVD (warm start).
    * ``DensityMatrixMixer.mix_rho`` (``mps_common.py:1972``) is wrapped in place: with a device ``TwoSiteH`` the density matrices are
      one ``tpa_herk_chain`` launch per side (``algorithms/mixer.py``), else the reference's statements.
    * ``SubspaceExpansion.mix_and_decompose_1site`` (``mps_common.py:2133``) is wrapped in place, and ``OneSiteH`` as ``dmrg`` knows it
      and ``SingleSiteDMRGEngine.EffectiveH`` (``dmrg.py:974``) are a device ``OneSiteH`` that also takes the chain's boundary environments: with it the expanded matrix of single-site
      DMRG is one GEMM over chi and one ``tpa_mpo_expand_batch`` launch (``mixer.device_expand_1site``; ``LHeff`` / ``RHeff`` are not
      built), else -- ``combine=True``, ``explicit_plus_hc``, infinite systems, sites the device class hands back -- the reference's
      method runs (``module_form.stats['expand_device']`` / ``['expand_reference']``).
    * ``MPO.apply_zipup`` (``networks/mpo.py:1679``; ``MPO.apply`` with ``compression_method='zip_up'``, ``ExpMPOEvolution``) is wrapped in
      place: the matrix of every interior site is one GEMM over chi and the MPO step on the device (``mps_common.device_zipup_step``,
      ``tpa_mpo_cell_apply_batch`` / ``tpa_mpo_expand_batch``), the boundary sites and declined sites run the reference's statements
      (``module_form.stats['zipup_device']`` / ``['zipup_reference']``, reasons in ``mps_common.zipup_stats['why']``).
    * ``MPS.correlation_function`` and the one-site case of ``MPS.expectation_value`` (``networks/mps.py:680`` / ``:462``) are wrapped in
      place (``module_form.device_measure``): the reference's argument handling runs, the rows of a correlation matrix come from one
      stacked walk over the chain and one ``tpa_site_inner_batch`` launch per closing site (``networks/measure.py``); ``MPSEnvironment``,
      infinite chains, multi-site operators and the ``term_*`` functions keep the reference's statements
      (``module_form.stats['measure_device']`` / ``['measure_reference']``, reasons in ``measure.measure_stats['why']``; ``TPA_MEASURE=0``
      switches the route off).
    * ``MPS.sample_measurements`` (``networks/mps.py:4349``) is wrapped in place (``module_form.device_sample``) and takes the extra
      keyword ``n_samples``: a batch of samples is carried through a finite chain as one stack, per site one GEMM, one
      ``tpa_sample_select_batch`` and one ``tpa_sample_gather_batch`` launch and one host read (``networks/sample.py``); infinite and
      segment chains, subclasses and ``first_site > 0`` inside the chain run the reference's own method
      (``module_form.stats['sample_device']`` / ``['sample_reference']``, reasons in ``sample.sample_stats['why']``; ``TPA_SAMPLE=0``
      switches the route off, ``TPA_SAMPLE_SINGLE=0`` does so for single-sample calls only; defaults: ``profiles/sample.txt``).
    * ``MPS.mutinf_two_site`` (``networks/mps.py:4180``) is wrapped in place (``module_form.device_mutinf``): the two-site density
      matrices of all pairs come from one stacked walk -- per site and charge difference one GEMM pair and one ``tpa_site_rho_batch``
      launch that closes every open row with the physical index pair left open, one device-to-host copy per walk -- and the entropies
      from host eigenvalues per charge block (``networks/rho.py``); infinite and segment chains, subclasses (``PurificationMPS`` and
      ``UniformMPS`` have methods of their own and are not touched), several physical legs and physical sectors wider than 4 run the
      reference's own method (``module_form.stats['mutinf_device']`` / ``['mutinf_reference']``, reasons in
      ``rho.rho_stats['why']``; ``TPA_MUTINF=0`` switches the route off; default: ``profiles/mutinf.txt``).
    * ``MPO.expectation_value_finite`` and ``MPO.variance`` (``networks/mpo.py:1144`` / ``:1296``) are wrapped in place
      (``module_form.device_moments``): ``<H>`` and ``<H^2>`` of a finite chain come from one left-to-right walk -- per site and row
      set two grouped GEMMs and one launch of the MPO-step plan of the MPO, ``variance`` without ``exp_val`` takes both moments from
      the same walk (``networks/moments.py``); segment chains, ``explicit_plus_hc``, given environment data, MPOs without a plan class
      and MPO bonds wider than about 8 run the reference's own method (``module_form.stats['moments_device']`` / ``['moments_reference']``, reasons in
      ``moments.moments_stats['why']``; ``TPA_MPO_MOMENTS=0`` switches the route off; default: ``profiles/mpo_moments.txt``).
    * ``TEBDEngine.evolve_step`` (``tebd.py:374``; inherited by ``QRBasedTEBDEngine``) -> the bonds of a half-step decomposed in one
      batched device call (``module_form.batched_tebd_evolve_step``; the per-bond statements stay the reference's).
    * ``LanczosEvolution`` (``linalg/krylov_based.py:718``; constructed at ``tdvp.py:132 _krylov_evolve``) -> the device class: the
      whole Krylov loop as one ``tpa_lanczos_run`` call and the result as one pass over the Krylov vectors with complex coefficients (plus the normalising ``tpa_scal``), where the operator
      offers a launch program; ``OneSiteH`` / ``ZeroSiteH`` (``mps_common.py:1040`` / ``:1440``; ``tdvp.py:308`` / ``:419``) -> the
      device forms of ``module_form`` (factored matvec with cached plans), which hand what they do not cover back to the
      reference's classes; ``TwoSiteTDVPEngine.EffectiveH`` / ``SingleSiteTDVPEngine.EffectiveH`` (``tdvp.py:248`` / ``:333``) get the
      device ``TwoSiteH`` / ``OneSiteH``, so that the forward evolutions run natively too.  ``OneSiteH`` is rebound in ``mps_common``,
      ``tdvp`` and ``dmrg``, ``ZeroSiteH`` in ``mps_common`` and ``tdvp`` only: VUMPS and the plane-wave excitations keep theirs.
    * ``OrthogonalNpcLinearOperator`` (``linalg/sparse.py:220``; constructed at ``mps_common.py:540 _wrap_ortho_eff_H``, where it is
      imported by name) -> the device class of ``tenpy_amd/linalg/sparse.py`` (same constructor, same ``gram_schmidt``, same
      ``matvec``), whose ``native_input`` puts the two projections into the launch program of the operator it wraps: the engines'
      ``orthogonal_to=[...]`` runs (excited states) reach the native Krylov loop through the device ``TwoSiteH``.
    * ``SumNpcLinearOperator`` (``linalg/sparse.py:152``; constructed at ``mps_common.py:520``, ``tdvp.py:311`` and ``:423`` for MPOs with
      ``explicit_plus_hc``, where it is imported by name) -> ``module_form.device_sum_operator``: a subclass whose constructor hands
      back ``eff_H.plus_hc()`` -- ``H_eff + H_eff^dagger`` as one device operator -- for a device operator and its own adjoint, and is
      the reference's class for everything else.  Rebound in ``mps_common`` and ``tdvp`` only (VUMPS and the plane-wave excitations
      keep theirs).
    """
    import tenpy.algorithms.dmrg as ref_dmrg
    import tenpy.algorithms.mps_common as ref_mc
    import tenpy.linalg.krylov_based as ref_kb
    from .algorithms import module_form
    from .linalg import krylov_based as kb
    ref_kb.LanczosGroundState = kb.LanczosGroundState
    ref_dmrg.LanczosGroundState = kb.LanczosGroundState
    import tenpy.linalg.sparse as ref_sparse
    from .linalg import sparse as dev_sparse
    ref_sparse.OrthogonalNpcLinearOperator = ref_mc.OrthogonalNpcLinearOperator = dev_sparse.OrthogonalNpcLinearOperator
    if not hasattr(ref_mc.TwoSiteH, '_reference_class'):
        dev_cls = module_form.device_two_site_h(ref_mc.TwoSiteH)
        ref_mc.TwoSiteH = dev_cls
        ref_dmrg.TwoSiteH = dev_cls
        ref_dmrg.TwoSiteDMRGEngine.EffectiveH = dev_cls
    if not getattr(ref_dmrg.TwoSiteDMRGEngine.mixed_svd, '_tpa_wrapped', False):
        ref_dmrg.TwoSiteDMRGEngine.mixed_svd = module_form.hinted_mixed_svd(ref_dmrg.TwoSiteDMRGEngine.mixed_svd)
    if not getattr(ref_mc.DensityMatrixMixer.mix_rho, '_tpa_wrapped', False):
        ref_mc.DensityMatrixMixer.mix_rho = module_form.device_mixer_mix_rho(ref_mc.DensityMatrixMixer.mix_rho)
    if not getattr(ref_mc.SubspaceExpansion.mix_and_decompose_1site, '_tpa_wrapped', False):
        ref_mc.SubspaceExpansion.mix_and_decompose_1site = module_form.device_subspace_expansion(
            ref_mc.SubspaceExpansion.mix_and_decompose_1site, ref_mc)
    import tenpy.networks.mpo as ref_mpo
    if not getattr(ref_mpo.MPO.apply_zipup, '_tpa_wrapped', False):
        ref_mpo.MPO.apply_zipup = module_form.device_apply_zipup(ref_mpo.MPO.apply_zipup, ref_mpo)
    if not getattr(ref_mpo.MPO.variance, '_tpa_wrapped', False):
        module_form.device_moments(ref_mpo)
    import tenpy.networks.mps as ref_mps
    if not getattr(ref_mps.BaseMPSExpectationValue.correlation_function, '_tpa_wrapped', False):
        module_form.device_measure(ref_mps)
    if not getattr(ref_mps.MPS.mutinf_two_site, '_tpa_wrapped', False):
        module_form.device_mutinf(ref_mps)
    if not getattr(ref_mps.MPS.sample_measurements, '_tpa_wrapped', False):
        module_form.device_sample(ref_mps)
    import tenpy.algorithms.tebd as ref_tebd
    if not getattr(ref_tebd.TEBDEngine.evolve_step, '_tpa_wrapped', False):
        ref_tebd.TEBDEngine.evolve_step = module_form.batched_tebd_evolve_step(ref_tebd)
    import tenpy.algorithms.tdvp as ref_tdvp
    ref_kb.LanczosEvolution = kb.LanczosEvolution
    ref_tdvp.LanczosEvolution = kb.LanczosEvolution
    if not hasattr(ref_mc.OneSiteH, '_reference_class'):
        ref_mc.OneSiteH = ref_tdvp.OneSiteH = module_form.device_one_site_h(ref_mc.OneSiteH)
    if not getattr(ref_dmrg.OneSiteH, '_boundary_envs', False):      # (a class of its own: it also takes the boundary environments)
        ref_dmrg.OneSiteH = ref_dmrg.SingleSiteDMRGEngine.EffectiveH = module_form.device_one_site_h(
            getattr(ref_mc.OneSiteH, '_reference_class', ref_mc.OneSiteH), boundary_envs=True)
    # `import tenpy` has imported tdvp already: the names and class attributes bound there are re-pointed one by one
    ref_tdvp.TwoSiteH = ref_tdvp.TwoSiteTDVPEngine.EffectiveH = ref_mc.TwoSiteH
    ref_tdvp.SingleSiteTDVPEngine.EffectiveH = ref_mc.OneSiteH
    if not hasattr(ref_mc.ZeroSiteH, '_reference_class'):
        ref_mc.ZeroSiteH = ref_tdvp.ZeroSiteH = module_form.device_zero_site_h(ref_mc.ZeroSiteH)
    if not hasattr(ref_mc.SumNpcLinearOperator, '_reference_class'):
        ref_mc.SumNpcLinearOperator = ref_tdvp.SumNpcLinearOperator = module_form.device_sum_operator(ref_sparse.SumNpcLinearOperator)
