"""Device forms of the callers that TeNPy's own engines construct per bond update, for the module form of the boundary
(``tenpy_amd.install.install(fused=True)``): the engines (``tenpy/algorithms/dmrg.py:529 update_local``,
``mps_common.py:516 make_eff_H``) stay the reference's code; only what they instantiate is rebound.

* ``device_two_site_h(RefTwoSiteH)`` -> a class with the constructor and interface of the reference's ``TwoSiteH``
  (``mps_common.py:1245``: ``(env, i0, combine=False, move_right=True)``, ``matvec`` :1321, ``combine_theta`` :1374,
  ``update_LP`` / ``update_RP`` :1421-1437, ``LHeff`` / ``RHeff`` for the mixers :1887-1898) on top of
  ``tenpy_amd.algorithms.mps_common.TwoSiteH``: cached contraction plans, fused ``LHeff`` build, and -- for
  ``combine=False``, the reference's default -- the factored matvec ``LP . theta . (W0 W1) . RP`` with the MPO tensors
  applied blockwise -- linear combinations of blocks where every MPO block is a single number, small dense matrices on the
  physical index where a charge sector of the site holds several states (``mps_common.MpoBlockApplyPlan``), single entries between
  the middle rows of blocks where MPO bond legs have blocks wider than 1 -- MPOs after ``sort_legcharges`` -- or physical sectors are
  wider than ``TPA_MPO_APPLY_MAXD`` (two sites: their product) (``mps_common.MpoEntryApplyPlan``) -- instead of K = 1
  GEMMs.  Bonds the device form does not cover (sectors below ``MIN_SECTOR``, MPOs without a conserved charge unless
  ``TPA_MPO_ENTRY_APPLY=2``, the two-thread ``H + h.c.`` environments of ``dmrg_parallel``, exact diagonalisation of small bonds) get
  the reference's own class: ``__new__`` dispatches, so the engines see one ``EffectiveH``.
* ``device_one_site_h(RefOneSiteH)`` / ``device_zero_site_h(RefZeroSiteH)`` -> the same for the operators TDVP constructs after
  every two-site / one-site update (``tdvp.py:308 one_site_update``, ``:419 zero_site_update``) on top of
  ``mps_common.OneSiteH`` / ``ZeroSiteH``; ``combine=True``, MPO tensors without a blockwise form
  (``mps_common._mpo_plan_class``: as above) and non-standard labels get the reference's class.
* ``device_sum_operator(RefSum)`` -> ``SumNpcLinearOperator`` as the engines construct it for MPOs with ``explicit_plus_hc``
  (``mps_common.py:519``, ``tdvp.py:310``, ``:422``: ``SumNpcLinearOperator(eff_H, eff_H.adjoint())``).  ``adjoint()`` of the three device
  classes is a token that knows its operator (``mps_common.AdjointH``, with a step-by-step matvec of its own); given a device operator
  and that operator's own token, the constructor hands back ``eff_H.plus_hc()`` -- ``H_eff + H_eff^dagger`` as ONE device operator on
  the direct sum along the MPO bond (``mps_common.PlusHcH``: three launches per matvec, a launch program for the native Krylov loops)
  -- and an ordinary instance in every other case (``stats['plus_hc_device']`` / ``['plus_hc_declined']``).  ``TPA_PLUS_HC=0``: such
  environments go to the reference's classes as before.
* ``hinted_mixed_svd(ref_mixed_svd)`` wraps ``TwoSiteDMRGEngine.mixed_svd`` (``dmrg.py:876``) to tell the block SVD which
  bond it decomposes (``np_conserved.svd_hint``), which enables the warm start of ``linalg/_svd_warm.py``.
"""
import os
import warnings

import numpy as np

from ..linalg import np_conserved as npc
from ..linalg.charges import DipolarChargeInfo
from . import mps_common as dev_mc

__all__ = ['device_two_site_h', 'device_one_site_h', 'device_zero_site_h', 'device_sum_operator', 'hinted_mixed_svd', 'device_mixer_mix_rho',
           'device_subspace_expansion', 'device_measure', 'device_mutinf', 'device_sample', 'device_moments']

# Smallest "largest bond sector" for which the device form is used.  Round 3 measurement (module form on the MI355X, Heisenberg
# L = 100, mixer ramp): with the reference's own class below 64 -- four generic tensordots with transposed copies per matvec,
# ~20 device calls and ~1 ms of interpreter time each -- a chi <= 256 sweep took 4.4 - 4.9 s against 0.9 - 1.5 s with the
# device form everywhere, so the threshold is 1 (kept as a knob for A/B runs).
MIN_SECTOR = 1
stats = {'device': 0, 'reference': 0,      # bonds handled by the device form / handed back to the reference's class (TwoSiteH)
         'device_one': 0, 'reference_one': 0, 'device_zero': 0, 'reference_zero': 0,      # the same for OneSiteH / ZeroSiteH
         # H + h.c. (MPOs with explicit_plus_hc): operators that became one doubled device operator / that did not -- `plus_hc`
         # declined (the ordinary SumNpcLinearOperator of the device operator and its step-by-step adjoint then), or the device class
         # handed the bond to the reference's class at construction, which `plus_hc_reference` counts once more on its own;
         # `plus_hc_other`: sums of anything but a device operator and its own adjoint (the reference's class, unchanged)
         'plus_hc_device': 0, 'plus_hc_declined': 0, 'plus_hc_reference': 0, 'plus_hc_other': 0,
         # DensityMatrixMixer.mix_rho: calls served by `mixer.device_mix_rho` (one tpa_herk_chain launch per side) / by the reference's statements
         'mixer_device': 0, 'mixer_reference': 0,
         # SubspaceExpansion.mix_and_decompose_1site: expansions served by `mixer.device_expand_1site` (one tpa_mpo_expand_batch launch) / by
         # the reference's method
         'expand_device': 0, 'expand_reference': 0,
         # MPO.apply_zipup: sites whose matrix came from `mps_common.device_zipup_step` / from the reference's statements (of these:
         # the two boundary sites of every pass); whole passes handed to the reference's method with ONE counted decline
         # (`explicit_plus_hc`, not finite: it refuses them before its loop); declines by reason: `mps_common.zipup_stats['why']`, so
         # zipup_reference - zipup_boundary == declined - zipup_handed_back
         'zipup_device': 0, 'zipup_reference': 0, 'zipup_boundary': 0, 'zipup_handed_back': 0,
         # MPS.correlation_function / one-site MPS.expectation_value: calls (per triangle of a correlation matrix) whose values came
         # from `networks/measure.py` (the stacked walk, `tpa_site_inner_batch`) / from the reference's statements, the latter each
         # with a reason in `measure.measure_stats['why']`
         'measure_device': 0, 'measure_reference': 0,
         # calls of ``MPS.mutinf_two_site`` served by the stacked walk of `networks/rho.py` (`tpa_site_rho_batch`) / by the reference's
         # own method, the latter each with a reason in `rho.rho_stats['why']`
         'mutinf_device': 0, 'mutinf_reference': 0,
         # calls of ``MPS.sample_measurements`` served by the batched walk of `networks/sample.py` (`tpa_sample_select_batch` /
         # `tpa_sample_gather_batch`) / by the reference's own method, the latter each with a reason in `sample.sample_stats['why']`
         'sample_device': 0, 'sample_reference': 0,
         # calls of ``MPO.expectation_value_finite`` / ``MPO.variance`` served by the walk of `networks/moments.py` / by the reference's
         # own methods, the latter each with a reason in `moments.moments_stats['why']` (infinite MPOs in ``MPO.expectation_value`` too)
         'moments_device': 0, 'moments_reference': 0}


def device_two_site_h(Ref):
    class DeviceTwoSiteH(dev_mc.TwoSiteH):
        __doc__ = "Device form of tenpy.algorithms.mps_common.TwoSiteH (see tenpy_amd/algorithms/module_form.py)."
        length = 2
        acts_on = ['vL', 'p0', 'p1', 'vR']
        _reference_class = Ref

        def __new__(cls, env, i0, combine=False, move_right=True):
            if cls._device_ok(env, i0, combine):
                stats['device'] += 1
                return object.__new__(cls)
            stats['reference'] += 1
            _count_hc_reference(env)
            return Ref(env, i0, combine, move_right)          # not an instance of cls: __init__ below is skipped

        @staticmethod
        def _device_ok(env, i0, combine):
            try:
                if not _plain_env(env):
                    return False
                if isinstance(env.H.chinfo, DipolarChargeInfo) and not env.ket.finite:
                    # dipole charges shift from unit cell to unit cell, which update_LP / update_RP below do not do: the reference's class
                    # (the reference's tests/test_dmrg.py::test_dmrg_dipole_conservation[2-infinite] raised "incompatible LegCharge" in
                    # update_LP under the fused callers; tests/test_reference_excited_fused.py runs that file)
                    return False
                LP, RP = env.get_LP(i0), env.get_RP(i0 + 1)
                if int(np.max(LP.get_leg('vR').get_block_sizes())) < MIN_SECTOR:
                    return False
                if sorted(LP.get_leg_labels()) != sorted(['vR*', 'wR', 'vR']) or sorted(RP.get_leg_labels()) != sorted(['wL', 'vL', 'vL*']):
                    return False
                if not combine:         # factored form: W0, W1 applied blockwise (single numbers or small matrices), no transposed copies needed
                    return dev_mc.factored_matvec_possible(LP, RP, env.H.get_W(i0), env.H.get_W(i0 + 1))
                return True
            except Exception:
                return False

        def __init__(self, env, i0, combine=False, move_right=True):
            dev_mc.TwoSiteH.__init__(self, env, i0, combine=True, move_right=move_right, factored=not combine)
            if (not combine) and not self.factored:
                raise RuntimeError("tenpy_amd: factored matvec not applicable although _device_ok said so")
            self.combine = combine
            self.acts_on = ['(vL.p0)', '(p1.vR)'] if combine else ['vL', 'p0', 'p1', 'vR']

        def combine_theta(self, theta):
            theta = dev_mc.TwoSiteH.combine_theta(self, theta)
            return theta.itranspose(self.acts_on) if list(theta.get_leg_labels()) != self.acts_on else theta

        def matvec(self, theta):
            labels = theta.get_leg_labels()
            res = dev_mc.TwoSiteH.matvec(self, theta)
            if list(res.get_leg_labels()) != list(labels):
                res.itranspose(labels)
            return res

        def update_LP(self, env, i, U=None):
            if U is None or not (self.combine or self.factored):
                return env.get_LP(i, store=True)
            lab = '(vL.p)' if U.has_label('(vL.p)') else '(vL.p0)'
            if not U.has_label(lab):
                return env.get_LP(i, store=True)
            return dev_mc.TwoSiteH.update_LP(self, env, i, U.replace_label(lab, '(vL.p0)'))

        def update_RP(self, env, i, VH=None):
            if VH is None or not (self.combine or self.factored):
                return env.get_RP(i, store=True)
            lab = '(p.vR)' if VH.has_label('(p.vR)') else '(p1.vR)'
            if not VH.has_label(lab):
                return env.get_RP(i, store=True)
            return dev_mc.TwoSiteH.update_RP(self, env, i, VH.replace_label(lab, '(p1.vR)'))

        def to_matrix(self):
            """Contract to a matrix Array like the reference (:1392)."""
            if self.combine:
                return self.to_matrix_array()
            contr = npc.tensordot(self.LP, self.W0, axes=['wR', 'wL'])
            contr = npc.tensordot(contr, self.W1, axes=['wR', 'wL'])
            contr = npc.tensordot(contr, self.RP, axes=['wR', 'wL'])
            return contr.combine_legs([['vR*', 'p0', 'p1', 'vL*'], ['vR', 'p0*', 'p1*', 'vL']], qconj=[+1, -1])

    DeviceTwoSiteH.__name__ = 'TwoSiteH'
    DeviceTwoSiteH.__qualname__ = 'TwoSiteH'
    return DeviceTwoSiteH


def _plain_env(env):
    """Whether the device classes take this environment: not the two-thread ``H + h.c.`` environments of ``dmrg_parallel`` (``has_hc``),
    and MPOs with ``explicit_plus_hc`` only while ``mps_common.PLUS_HC`` is on -- the engines then wrap the operator as
    ``SumNpcLinearOperator(eff_H, eff_H.adjoint())``, which ``device_sum_operator`` turns into ``eff_H.plus_hc()``."""
    if getattr(env, 'has_hc', False):
        return False
    return dev_mc.PLUS_HC or not getattr(env.H, 'explicit_plus_hc', False)


def _count_hc_reference(env):
    if getattr(getattr(env, 'H', None), 'explicit_plus_hc', False) and not getattr(env, 'has_hc', False):
        stats['plus_hc_reference'] += 1
        stats['plus_hc_declined'] += 1


def device_sum_operator(Ref):
    class DeviceSumOperator(Ref):
        __doc__ = ("tenpy.linalg.sparse.SumNpcLinearOperator whose constructor hands back ``op.plus_hc()`` when it is given a device "
                   "operator and that operator's own adjoint (see tenpy_amd/algorithms/module_form.py).")
        _reference_class = Ref

        def __new__(cls, orig_operator, other_operator):
            if isinstance(other_operator, dev_mc.AdjointH) and other_operator.op is orig_operator:
                doubled = orig_operator.plus_hc()
                if doubled is not None:
                    stats['plus_hc_device'] += 1
                    return doubled                      # not an instance of cls: __init__ is skipped
                stats['plus_hc_declined'] += 1
            else:
                stats['plus_hc_other'] += 1
            return object.__new__(cls)

    DeviceSumOperator.__name__ = DeviceSumOperator.__qualname__ = 'SumNpcLinearOperator'
    return DeviceSumOperator


def device_one_site_h(Ref, boundary_envs=False):
    """``boundary_envs`` (the class bound for single-site DMRG): an environment whose legs all have 1-wide blocks -- the reference's
    ``init_LP`` / ``init_RP`` of a finite chain, which puts the bra leg before the ket leg on the right -- is taken with its legs
    relabelled in the order of the factored forms (a view, no copy) instead of being handed back to the reference's class; the last
    site of every right sweep is such a site."""
    class DeviceOneSiteH(dev_mc.OneSiteH):
        __doc__ = "Device form of tenpy.algorithms.mps_common.OneSiteH (see tenpy_amd/algorithms/module_form.py)."
        _reference_class = Ref
        _boundary_envs = boundary_envs

        def __new__(cls, env, i0, combine=False, move_right=True):
            tensors = cls._device_tensors(env, i0, combine)
            if tensors is not None:
                stats['device_one'] += 1
                self = object.__new__(cls)
                self._tensors = tensors
                return self
            stats['reference_one'] += 1
            _count_hc_reference(env)
            return Ref(env, i0, combine, move_right)          # not an instance of cls: __init__ is skipped

        @staticmethod
        def _device_tensors(env, i0, combine):
            """``(LP, W0, RP)`` if the device form covers this site, else ``None``."""
            if combine or not _plain_env(env):
                return None
            LP, W0, RP = env.get_LP(i0), env.H.get_W(i0), env.get_RP(i0)
            if boundary_envs:
                LP, RP = _boundary_view(LP, ['vR*', 'wR', 'vR']), _boundary_view(RP, ['wL', 'vL', 'vL*'])
            if list(W0.get_leg_labels()) != ['wL', 'wR', 'p', 'p*'] or dev_mc._factored_plan_class(LP, RP, W0) is None:
                return None
            return LP, W0, RP

        def __init__(self, env, i0, combine=False, move_right=True):
            LP, W0, RP = self.__dict__.pop('_tensors')
            self.move_right = move_right
            self._env = env
            self._setup(LP, W0, RP, i0, env.H.dtype)

        from_LP_W0_RP = staticmethod(lambda *args, **kwargs: Ref.from_LP_W0_RP(*args, **kwargs))      # (VUMPS: the reference's form)

    DeviceOneSiteH.__name__ = DeviceOneSiteH.__qualname__ = 'OneSiteH'
    return DeviceOneSiteH


def _boundary_view(A, labels):
    """``A`` with its legs in the order ``labels`` where that moves no data (every leg has 1-wide blocks), else ``A`` itself."""
    have = list(A.get_leg_labels())
    if have == labels or sorted(have) != sorted(labels) or not all(np.all(leg.get_block_sizes() == 1) for leg in A.legs):
        return A
    return dev_mc._relabel_view(A, labels)


def device_zero_site_h(Ref):
    class DeviceZeroSiteH(dev_mc.ZeroSiteH):
        __doc__ = "Device form of tenpy.algorithms.mps_common.ZeroSiteH (see tenpy_amd/algorithms/module_form.py)."
        _reference_class = Ref

        def __new__(cls, env, i0):
            if _plain_env(env):
                LP, RP = env.get_LP(i0), env.get_RP(i0 - 1)
                if dev_mc._envs_factorable(LP, RP):
                    stats['device_zero'] += 1
                    self = object.__new__(cls)
                    self._tensors = (LP, RP)
                    return self
            stats['reference_zero'] += 1
            _count_hc_reference(env)
            return Ref(env, i0)

        def __init__(self, env, i0):
            LP, RP = self.__dict__.pop('_tensors')
            self._env = env
            self._setup(LP, None, RP, i0, env.H.dtype)

        from_LP_RP = staticmethod(lambda *args, **kwargs: Ref.from_LP_RP(*args, **kwargs))

    DeviceZeroSiteH.__name__ = DeviceZeroSiteH.__qualname__ = 'ZeroSiteH'
    return DeviceZeroSiteH


def hinted_mixed_svd(ref_mixed_svd):
    def mixed_svd(self, theta):
        if self.mixer is None:       # plain svd_theta: the next npc.svd decomposes the theta of bond (i0, i0 + 1)
            from ..linalg import _svd_warm
            npc.svd_hint = ((_svd_warm.owner_token(self.psi), int(self.i0)), 'R' if self.move_right else 'L')
        try:
            return ref_mixed_svd(self, theta)
        finally:
            npc.svd_hint = None
    mixed_svd.__doc__ = ref_mixed_svd.__doc__
    mixed_svd._tpa_wrapped = True
    return mixed_svd


def device_mixer_mix_rho(ref_mix_rho):
    """Wraps ``DensityMatrixMixer.mix_rho`` (mps_common.py:1972-2027) IN PLACE -- the class keeps its identity, so that
    ``find_subclass(Mixer, name)`` keeps resolving: with a device ``TwoSiteH`` as ``engine.eff_H`` the density matrices come from
    ``mixer.device_mix_rho``; wherever that declines, and for every other operator, the reference's statements run."""
    from . import mixer as dev_mixer

    def mix_rho(self, engine, theta, i0, mix_left, mix_right):
        eff_H = getattr(engine, 'eff_H', None)
        plain = eff_H.plain if isinstance(eff_H, dev_mc.PlusHcH) else eff_H      # (H + h.c.: the mixer works on the plain operator)
        if isinstance(plain, dev_mc.TwoSiteH) and getattr(plain, 'i0', None) == i0:
            got = dev_mixer.device_mix_rho(eff_H, engine.env.H, theta, i0, self.amplitude, mix_left, mix_right)
            if got is not None:
                stats['mixer_device'] += 1
                return got
        stats['mixer_reference'] += 1
        return ref_mix_rho(self, engine, theta, i0, mix_left, mix_right)
    mix_rho.__doc__ = ref_mix_rho.__doc__
    mix_rho._tpa_wrapped = True
    return mix_rho


def device_subspace_expansion(ref_method, ref_mc):
    """Wraps ``SubspaceExpansion.mix_and_decompose_1site`` (mps_common.py:2133-2201) IN PLACE, like ``device_mixer_mix_rho``: with a device
    ``OneSiteH`` as ``engine.eff_H``, and where ``mixer.device_expand_1site`` does not decline, ``theta_expand`` comes from the device
    route -- ``LHeff`` / ``RHeff`` are not built -- and is decomposed by the statements of ``mixer.SubspaceExpansion`` with the
    reference's own ``svd_theta``; otherwise the reference's method runs."""
    from . import mixer as dev_mixer

    def mix_and_decompose_1site(self, engine, theta, i0, move_right):
        eff_H = getattr(engine, 'eff_H', None)
        if isinstance(eff_H, dev_mc.OneSiteH) and getattr(eff_H, 'i0', None) == i0:
            got = dev_mixer.device_expand_1site(eff_H, engine.env.H, theta, i0, self.amplitude, move_right)
            if got is not None:
                stats['expand_device'] += 1
                return dev_mixer.decompose_expanded(got[0], got[1], theta, engine.trunc_params, move_right, svd_theta=ref_mc.svd_theta)
        stats['expand_reference'] += 1
        return ref_method(self, engine, theta, i0, move_right)
    mix_and_decompose_1site.__doc__ = ref_method.__doc__
    mix_and_decompose_1site._tpa_wrapped = True
    return mix_and_decompose_1site


def device_apply_zipup(ref_method, ref_mpo):
    """Wraps ``MPO.apply_zipup`` (networks/mpo.py:1679-1767) IN PLACE, like ``device_subspace_expansion``: the statements of the reference's
    pass with the matrix of every interior site taken from ``mps_common.device_zipup_step`` -- one GEMM over chi and the MPO step on the
    device; ``tensordot(B, W)``, an intermediate of chi^2 D^2 d elements, is not built.  The two boundary sites, and interior sites the
    device route declines (counted with the reason), run the reference's own statements; what the reference refuses before its loop
    (boundary conditions, lengths, ``explicit_plus_hc``) is handed to its method."""
    def apply_zipup(self, psi, options):
        finite = psi.bc == 'finite' and self.bc == 'finite'
        if self.explicit_plus_hc or not finite:      # one decline, counted with its reason, for the whole pass
            declined = dev_mc.device_zipup_step(None, None, None, explicit_plus_hc=self.explicit_plus_hc, finite=finite)
            assert declined is None
            stats['zipup_handed_back'] += 1
            return ref_method(self, psi, options)
        if psi.L != self.L or psi.L < 3:
            return ref_method(self, psi, options)
        svd_theta, ref_npc = ref_mpo.svd_theta, ref_mpo.npc
        options = ref_mpo.asConfig(options, 'zip_up')
        m_temp = options.get('m_temp', 2, int)
        trunc_weight = options.get('trunc_weight', 1., 'real')
        trunc_params = options.subconfig('trunc_params')
        relax_trunc = trunc_params.copy()
        relax_trunc['chi_max'] *= m_temp
        if 'svd_min' in relax_trunc.keys():
            relax_trunc['svd_min'] *= trunc_weight
        trunc_err = ref_mpo.TruncationError()
        VH = None
        for i in range(psi.L):
            last = i == psi.L - 1
            B = dev_mc.device_zipup_step(VH, psi.get_B(i, 'B'), self.get_W(i)) if 0 < i and not last else None
            if B is not None:
                stats['zipup_device'] += 1
            else:
                stats['zipup_reference'] += 1
                stats['zipup_boundary'] += i == 0 or last
                B = ref_npc.tensordot(psi.get_B(i, 'B'), self.get_W(i), axes=('p', 'p*'))
                if i == 0:
                    B = B.take_slice(self.get_IdL(i), 'wL')
                else:
                    B = ref_npc.tensordot(VH, B, axes=(['wR', 'vR'], ['wL', 'vL']))
                if last:
                    B = B.take_slice(self.get_IdR(i), 'wR').combine_legs(['vL', 'p'], qconj=[-1])
                else:
                    B = B.combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1])
            U, S, VH, err, norm_new = svd_theta(B, relax_trunc, [B.qtotal, None]) if last else svd_theta(B, relax_trunc)
            trunc_err += err
            psi.norm *= norm_new
            U = U.split_legs()
            if not last:
                VH = VH.split_legs()
                VH.iscale_axis(S, 'vL')
            psi.set_SR(i, S)
            psi.set_B(i, U, 'A')
        return trunc_err
    apply_zipup.__doc__ = ref_method.__doc__
    apply_zipup._tpa_wrapped = True
    return apply_zipup


def device_measure(ref_mps):
    """Wraps ``correlation_function`` and ``expectation_value`` of the reference's ``BaseMPSExpectationValue`` (networks/mps.py:680-887,
    :462-596) IN PLACE.  The reference's own methods run -- ``_correlation_function_args``, the Jordan-Wigner decision, the diagonal,
    ``_normalize_exp_val`` -- and only the rows they ask ``_corr_up_diag`` for come from ONE stacked walk per triangle
    (``measure.device_corr_up``); a one-site ``expectation_value`` is one ``tpa_site_inner_batch`` launch per site and one host read.
    Everything else -- ``MPSEnvironment`` (bra != ket), infinite chains, multi-site operators, operators that need a string on the
    left, what ``measure.decline_reason`` names -- runs the reference's statements, counted with its reason."""
    from ..networks import measure
    Base = ref_mps.BaseMPSExpectationValue
    ref_corr, ref_exp = Base.correlation_function, Base.expectation_value

    def handed_back(why):
        stats['measure_reference'] += 1
        measure._count_why(why)

    def route_reason(self):
        if not measure.MEASURE:
            return 'switched_off'
        if not isinstance(self, ref_mps.MPS):
            return 'environment'
        if not self.finite:
            return 'infinite'
        return None

    def site_ops(self, op_list, what):
        """The operators of all sites as device Arrays (``None`` entries stay; the route reads each distinct one once per call); raises
        ``LookupError`` with a decline reason for what the route does not take."""
        out = []
        for k in range(self.L):
            op, needs_JW = self.get_op(op_list, k)
            if op is not None:
                if what != 'corr' and needs_JW:
                    raise LookupError('needs_JW')
                if op.rank != 2:
                    raise LookupError('multi_site')
            out.append(op)
        return out

    def correlation_function(self, ops1, ops2, sites1=None, sites2=None, opstr=None, str_on_first=True, hermitian=False, autoJW=True):
        why = route_reason(self)
        if why is not None:
            handed_back(why)
            return ref_corr(self, ops1, ops2, sites1, sites2, opstr, str_on_first, hermitian, autoJW)
        _, _, s1, s2, _ = self._correlation_function_args(ops1, ops2, sites1, sites2, opstr)      # (the sites as the reference sorts them)
        s1, s2 = [int(i) for i in s1], [int(j) for j in s2]
        served = {}
        ref_rows = type(self)._corr_up_diag

        def rows(o1, o2, i, j_gtr, ostr, str_first, apply_first):
            key = bool(apply_first)
            if key not in served:
                starts, ends = (s1, s2) if apply_first else (s2, s1)
                try:
                    a, b, strs = site_ops(self, o1, 'corr'), site_ops(self, o2, 'corr'), site_ops(self, ostr, 'corr')
                    strs = None if all(o is None for o in strs) else strs
                    reason = measure.decline_reason(self, a, b, strs)
                except LookupError as e:
                    reason = str(e)
                if reason is None:
                    stats['measure_device'] += 1
                    measure.measure_stats['device'] += 1
                    served[key] = (starts, ends, measure.device_corr_up(self, a, b, starts, ends, strs, str_first, apply_first))
                else:
                    handed_back(reason)
                    served[key] = None
            if served[key] is None:
                return ref_rows(self, o1, o2, i, j_gtr, ostr, str_first, apply_first)
            starts, ends, M = served[key]
            x = starts.index(int(i))
            return [M[x, ends.index(int(j))] for j in j_gtr]

        self._corr_up_diag = rows           # (an instance attribute for the duration of the call)
        try:
            return ref_corr(self, ops1, ops2, sites1, sites2, opstr, str_on_first, hermitian, autoJW)
        finally:
            del self.__dict__['_corr_up_diag']

    def expectation_value(self, ops, sites=None, axes=None):
        why = route_reason(self)
        if why is None:
            try:
                op_list, site_list, n, (ax_p, ax_pstar) = self._expectation_value_args(ops, sites, axes)
                if n != 1:
                    why = 'multi_site'
                elif list(ax_p) != ['p'] or list(ax_pstar) != ['p*']:
                    why = 'p_label'
                else:
                    per_site = site_ops(self, op_list, 'exp')
                    why = measure.decline_reason(self, per_site, per_site)
            except LookupError as e:
                why = str(e)
        if why is not None:
            handed_back(why)
            return ref_exp(self, ops, sites, axes)
        stats['measure_device'] += 1
        measure.measure_stats['device'] += 1
        E = measure.device_expectation_value(self, [per_site], [int(i) for i in site_list])[:, 0]
        return self._normalize_exp_val(E)

    correlation_function.__doc__, expectation_value.__doc__ = ref_corr.__doc__, ref_exp.__doc__
    correlation_function._tpa_wrapped = expectation_value._tpa_wrapped = True
    Base.correlation_function, Base.expectation_value = correlation_function, expectation_value


def device_mutinf(ref_mps):
    """Wraps ``MPS.mutinf_two_site`` of the reference (networks/mps.py:4180-4233) IN PLACE.  Calls that ``rho.decline_reason`` takes get
    the two-site density matrices of all pairs from the stacked walk of ``networks/rho.py`` (``device_two_site_rho``: per site and
    charge difference one GEMM pair and one ``tpa_site_rho_batch`` launch, one device-to-host copy per walk) and the entropies from
    host eigenvalues per charge block; everything else -- infinite and segment boundary conditions, subclasses, several physical
    legs, physical sectors wider than 4, ``TPA_MUTINF=0`` -- runs the reference's own method untouched, counted with its reason.
    ``PurificationMPS`` and ``UniformMPS`` override the method and are not touched."""
    from ..networks import rho
    ref_mutinf = ref_mps.MPS.mutinf_two_site

    def mutinf_two_site(self, max_range=None, n=1):
        why = rho.decline_reason(self, plain=ref_mps.MPS)
        if why is None:
            stats['mutinf_device'] += 1
        else:
            stats['mutinf_reference'] += 1
        return rho.mutinf_two_site(self, max_range, n, why=why, generic=lambda: ref_mutinf(self, max_range, n))

    mutinf_two_site.__doc__ = ref_mutinf.__doc__
    mutinf_two_site._tpa_wrapped = True
    ref_mps.MPS.mutinf_two_site = mutinf_two_site


def device_sample(ref_mps):
    """Wraps ``MPS.sample_measurements`` of the reference (networks/mps.py:4349-4442) IN PLACE and gives it the extra keyword
    ``n_samples``: ``None`` returns what the reference returns (a list and a scalar), n returns ``(ndarray (n, n_sites), ndarray (n,))``,
    outcome for outcome what n consecutive calls with the same generator return.  Calls that ``sample.decline_reason`` takes run the
    batched walk of ``networks/sample.py`` (three device steps and one host read per site for the whole batch); everything else --
    infinite and segment boundary conditions, subclasses (``UniformMPS`` comes here through ``super()``), ``first_site`` inside the
    chain, several physical legs, sites wider than ``TPA_SAMPLE_MAX_DIM``, ``TPA_SAMPLE=0`` and, with ``TPA_SAMPLE_SINGLE=0``,
    single-sample calls -- runs the reference's own method untouched, n times for a batch, counted with its reason.  ``PurificationMPS`` overrides the method and is not touched."""
    from ..networks import sample
    ref_sample = ref_mps.MPS.sample_measurements

    def sample_measurements(self, first_site=0, last_site=None, ops=None, rng=None, norm_tol=1.e-12, complex_amplitude=True, n_samples=None):
        why = 'not_plain_finite' if type(self) is not ref_mps.MPS else sample.decline_reason(self, first_site, last_site, n_samples)
        if rng is None:
            rng = np.random.default_rng()
        if why is None:
            stats['sample_device'] += 1
        else:
            stats['sample_reference'] += 1
        return sample.sample_measurements(self, first_site, last_site, ops, rng, norm_tol, complex_amplitude, n_samples, why=why,
                                          generic=lambda: ref_sample(self, first_site, last_site, ops, rng, norm_tol, complex_amplitude))

    sample_measurements.__doc__ = ref_sample.__doc__
    sample_measurements._tpa_wrapped = True
    ref_mps.MPS.sample_measurements = sample_measurements


def device_moments(ref_mpo):
    """Wraps ``MPO.expectation_value_finite`` and ``MPO.variance`` of the reference (networks/mpo.py:1144-1171, :1296-1342) IN PLACE:
    calls that ``moments.decline_reason`` does not take run the one walk of ``networks/moments.py`` -- ``variance`` without ``exp_val``
    takes both moments from it --; everything else (segment chains, ``explicit_plus_hc``, given environment data, MPOs without a plan
    class, wide MPO bonds, ``TPA_MPO_MOMENTS=0``) runs the reference's own method, counted with its reason.  The argument checks of ``variance`` are the
    reference's, in its order.  ``MPO.expectation_value`` only gains the count of the infinite MPOs it hands to the reference's
    transfer-matrix and power methods."""
    from ..networks import moments
    ref_finite, ref_var, ref_ev = ref_mpo.MPO.expectation_value_finite, ref_mpo.MPO.variance, ref_mpo.MPO.expectation_value

    def served(val_why):
        stats['moments_device' if val_why[1] is None else 'moments_reference'] += 1
        return val_why[0]

    def expectation_value_finite(self, psi, init_env_data={}):
        return served(moments.expectation_value(psi, self, lambda: ref_finite(self, psi, init_env_data), init_env_data))

    def variance(self, psi, exp_val=None):
        if self.bc != 'finite':
            raise ValueError('works only for finite systems')
        if self.L != psi.L:
            raise ValueError('expect same L')
        if psi._p_label != ['p']:
            raise NotImplementedError('not adjusted for non-standard MPS.')
        if self.explicit_plus_hc:
            raise NotImplementedError('not implemented for explicit_plus_hc flag')
        return served(moments.variance(psi, self, exp_val, lambda: ref_var(self, psi, exp_val)))

    def expectation_value(self, psi, tol=1.e-10, max_range=100, init_env_data={}):
        if not self.finite:
            stats['moments_reference'] += 1
            moments._count_why('infinite')
        return ref_ev(self, psi, tol, max_range, init_env_data)

    for new, ref in ((expectation_value_finite, ref_finite), (variance, ref_var), (expectation_value, ref_ev)):
        new.__doc__ = ref.__doc__
        new._tpa_wrapped = True
        setattr(ref_mpo.MPO, new.__name__, new)


def batched_tebd_evolve_step(ref_tebd):
    """Fused caller for the reference's ``TEBDEngine.evolve_step`` (algorithms/tebd.py:374-414): the bonds of one half-step do not
    share a site, so their decompositions go to the device as ONE batched call each (``np_conserved.svd_batched`` for
    ``TEBDEngine.update_bond``, tebd.py:416-483; ``qr_batched`` + ``svd_batched`` / ``eigh_batched`` for ``QRBasedTEBDEngine.update_bond``, :685-738).
    The per-bond statements before and after the decomposition are the reference's, in the reference's order; engines whose
    ``update_bond`` is not one of those two (subclasses), and everything else, run the reference's loop; with ``use_eig_based_svd``
    the Hermitian eigenproblems of the bond matrices are ONE ``eigh_batched`` call."""
    import numpy as np
    from ..linalg import truncation as dev_trunc
    ref_evolve_step = ref_tebd.TEBDEngine.evolve_step
    ref_update = ref_tebd.TEBDEngine.update_bond
    ref_update_qr = ref_tebd.QRBasedTEBDEngine.update_bond
    TruncationError = ref_tebd.TruncationError

    def evolve_step(self, U_idx_dt, odd):
        upd = type(self).update_bond
        qr_based = upd is ref_update_qr
        if not (upd is ref_update or qr_based) or not getattr(self.psi, 'finite', False):
            return ref_evolve_step(self, U_idx_dt, odd)
        Us = self._U[U_idx_dt]
        bonds = [int(i) for i in np.arange(int(odd) % 2, self.psi.L, 2) if Us[i] is not None]
        if len(bonds) < 2:
            return ref_evolve_step(self, U_idx_dt, odd)
        psi = self.psi
        # groups of bonds whose work areas fit the device together (algorithms/tebd.batch_group_size: ~24x the dense theta each)
        from .tebd import batch_bytes_cap
        cap = batch_bytes_cap()
        worst = max(24 * 16 * (psi.sites[i - 1].dim * len(psi.get_SL(i - 1))) * (psi.sites[i].dim * len(psi.get_SR(i))) for i in bonds)
        group = int(max(1, min(len(bonds), cap // max(worst, 1))))
        total = TruncationError()
        for g0 in range(0, len(bonds), group):
            total += _half_step_group(self, bonds[g0:g0 + group], Us, qr_based)
        self._update_index = None
        return total

    def _half_step_group(self, bonds, Us, qr_based):
        psi = self.psi
        Cs, thetas, extra = [], [], []
        for i in bonds:
            i0, i1 = i - 1, i
            C = psi.get_theta(i0, n=2, formL=0.0)
            C = npc.tensordot(Us[i], C, axes=(['p0*', 'p1*'], ['p0', 'p1']))
            C.itranspose(['vL', 'p0', 'p1', 'vR'])
            theta = C.scale_axis(psi.get_SL(i0), 'vL')
            theta = theta.combine_legs([('vL', 'p0'), ('p1', 'vR')], qconj=[+1, -1])
            Cs.append(C)
            thetas.append(theta)
            if qr_based:
                old_B_L, old_B_R = psi.get_B(i0, 'B'), psi.get_B(i1, 'B')
                extra.append((old_B_L.qtotal, old_B_R.qtotal, old_B_R.get_leg('vL'), theta, False, self._expansion_rate(i),
                              self.options.get('cbe_min_block_increase', 1, int)))
            else:
                extra.append([psi.get_B(i0, None).qtotal, None])
        total = TruncationError()
        if qr_based:
            compute_err = self.options.get('compute_err', True, bool)
            res = dev_trunc.decompose_theta_qr_based_batched(extra, self.trunc_params, compute_err, False,
                                                             use_eig_based_svd=self.options.get('use_eig_based_svd', False, bool))
            for i, C, theta, (_, S, B_R, form, err, renormalize) in zip(bonds, Cs, thetas, res):
                i0, i1 = i - 1, i
                if compute_err:         # the reference's warning (tebd.py:712-725), same condition, same text
                    chi_max = self.trunc_params.get('chi_max', None)
                    if err.eps > 1e-16 and chi_max is not None and len(S) < chi_max:
                        warnings.warn('QRBased decomposition resulted in large truncation error even though the bond '
                                      'dimension is not maxed out yet. Try increasing the expansion rate, e.g. '
                                      'via the `cbe_expand_0` and `cbe_min_block_increase` options for the engine. '
                                      'You probably should compare to a "regular" (non QR-based) engine and see how '
                                      'fast the bond dimension needs to grow for your scenario. '
                                      'See https://github.com/tenpy/tenpy/pull/513 .', stacklevel=2)
                assert form[1] == 'B'
                err = TruncationError(err.eps, err.ov)
                B_L = npc.tensordot(C.combine_legs(('p1', 'vR'), pipes=theta.legs[1]), B_R.conj(), axes=[['(p1.vR)'], ['(p*.vR*)']]) / renormalize
                B_L.ireplace_labels(['p0', 'vL*'], ['p', 'vR'])
                B_R = B_R.split_legs(1)
                psi.norm *= renormalize
                psi.set_B(i0, B_L, form='B')
                psi.set_SL(i1, S)
                psi.set_B(i1, B_R, form='B')
                self._trunc_err_bonds[i] = self._trunc_err_bonds[i] + err
                total += err
        else:
            npc.svd_engine_floor = True
            res = dev_trunc.svd_theta_batched(thetas, self.trunc_params, extra, inner_labels=['vR', 'vL'])
            for i, C, theta, (U, S, V, err, renormalize) in zip(bonds, Cs, thetas, res):
                i0, i1 = i - 1, i
                err = TruncationError(err.eps, err.ov)
                B_R = V.split_legs(1).ireplace_label('p1', 'p')
                B_L = npc.tensordot(C.combine_legs(('p1', 'vR'), pipes=theta.legs[1]), V.conj(), axes=['(p1.vR)', '(p1*.vR*)'])
                B_L.ireplace_labels(['vL*', 'p0'], ['vR', 'p'])
                B_L /= renormalize
                psi.norm *= renormalize
                psi.set_SR(i0, S)
                psi.set_B(i0, B_L, form='B')
                psi.set_B(i1, B_R, form='B')
                self._trunc_err_bonds[i] = self._trunc_err_bonds[i] + err
                total += err
        return total

    evolve_step.__doc__ = ref_evolve_step.__doc__
    evolve_step._tpa_wrapped = True
    return evolve_step
