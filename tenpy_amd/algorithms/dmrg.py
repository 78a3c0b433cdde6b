"""Minimal two-site (and single-site) DMRG driver for boxes WITHOUT TeNPy (the GPU test box: ``bench.py``, ``smoke()``, the ``-m gpu`` tests).

Where TeNPy is installed, use TeNPy's own engines on the device mirror instead -- ``tenpy_amd.install.install()`` and then
``tenpy.algorithms.dmrg.TwoSiteDMRGEngine`` etc. run unchanged (mixers, single-site DMRG, infinite systems, excited states:
all of it is the reference's code, ``tests/test_reference_suite.py``).  This file only issues the npc calls of one bond update
in the reference's order (``prepare_update_local`` -> ``update_local`` (Lanczos, ``svd_theta``, ``set_B``) ->
``update_env``) for finite chains, which is exactly BASELINE.json's timed workload; with ``mixer`` the density-matrix mixer of
``algorithms/mixer.py`` takes the place of ``svd_theta`` (reference dmrg.py:914-930).

Options (names as in the reference): ``trunc_params``, ``lanczos_params``, ``chi_list`` (dict sweep -> chi_max); ``mixer`` (``True`` /
``'DensityMatrixMixer'`` / ``None``, default ``None``), ``mixer_params`` (``amplitude``, ``decay``, ``disable_after``),
``chi_list_reactivates_mixer`` (default on: a step of ``chi_list`` switches the mixer on again, reference mps_common.py ``sweep``);
``shard_matvec`` (multi-GPU, ``algorithms/sharded.py``; with ``krylov_row_panels`` the Krylov vectors are row panels), ``profile`` (per-phase timers; synchronises the device).

``SingleSiteDMRGEngine`` (end of the file) is the single-site engine on the same footing: the reference's schedule and statements for
one optimised site, the device ``OneSiteH``, and the subspace expansion of ``algorithms/mixer.py`` as its mixer (on by default).

``orthogonal_to=[MPS, ...]`` (keyword, off by default; not with ``shard_matvec``): the search stays orthogonal to the given states
(reference ``mps_common.py:521-540``) -- the minimum the GPU tests of the projected Lanczos loop need, not an excited-state engine.
"""
import pickle
import gc
import os
import time

import numpy as np

from ..linalg import np_conserved as npc
from ..linalg.krylov_based import LanczosGroundState
from ..linalg.truncation import svd_theta
from ..networks.mpo import MPOEnvironment
from .mps_common import OneSiteH, TwoSiteH

__all__ = ['TwoSiteDMRGEngine', 'SingleSiteDMRGEngine']


_GC_PAUSE = os.environ.get('TPA_SWEEP_GC_PAUSE', '1') != '0'


def _plus_hc(eff_H):
    """``eff_H + eff_H^dagger`` for an MPO with ``explicit_plus_hc`` (reference mps_common.py:519-520, before the ``orthogonal_to``
    wrapping): one operator on the direct sum along the MPO bond where ``plus_hc`` offers it, else the sum of the two operators."""
    from ..linalg.sparse import SumNpcLinearOperator
    doubled = eff_H.plus_hc()
    return doubled if doubled is not None else SumNpcLinearOperator(eff_H, eff_H.adjoint())


class TwoSiteDMRGEngine:
    DefaultMixer = 'DensityMatrixMixer'
    use_mixer_by_default = False

    def _warm_token(self):
        """Key of this engine's warm-start bases (``linalg/_svd_warm.owner_token``: unique for the life of the engine, released with it)."""
        from ..linalg import _svd_warm
        return _svd_warm.owner_token(self)

    def __init__(self, psi, model_H, options, resume_data=None, orthogonal_to=None):
        if not psi.finite:
            raise ValueError("the stand-alone driver handles finite chains; run TeNPy's engines on the mirror for the rest")
        self.ortho_to_envs = []
        if orthogonal_to:
            if dict(options).get('shard_matvec', False):
                raise ValueError("orthogonal_to is not available together with shard_matvec")
            from ..networks.mps import OverlapEnvironment
            self.ortho_to_envs = [OverlapEnvironment(psi, ket) for ket in orthogonal_to]
        self.psi, self.H = psi, model_H
        self.options = options = dict(options)
        self.trunc_params = dict(options.get('trunc_params', {}))
        self.lanczos_params = dict(options.get('lanczos_params', {}))
        self.chi_list = options.get('chi_list')
        self.env = MPOEnvironment(psi, model_H)
        self.sweeps = 0
        self.update_stats = {k: [] for k in ('i0', 'E_total', 'N_lanczos', 'time', 'err', 'chi')}
        self.sweep_stats = {k: [] for k in ('sweep', 'E', 'S', 'time', 'max_trunc_err', 'max_chi')}
        self.profile = bool(options.get('profile', False))
        self.phase_time = {'heff': 0., 'lanczos': 0., 'svd': 0., 'env': 0., 'setB': 0.}
        self.shard_matvec = bool(options.get('shard_matvec', False))
        self._svd_group = None
        if self.shard_matvec:           # multi-GPU: the independent charge blocks of every SVD are dealt out to the ranks too
            import torch.distributed as dist
            import os
            if dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get('TPA_SHARD_FORCE')):
                self._svd_group = (None, dist.get_rank(), dist.get_world_size())
        self.mixer = None
        choice = options.get('mixer', self.use_mixer_by_default)
        self._mixer_on = choice not in (None, False)
        if choice not in (None, False, True, self.DefaultMixer):
            raise ValueError("mixer: True, %r or None (other mixers: TeNPy's engines on the mirror)" % self.DefaultMixer)
        if self._mixer_on and self.shard_matvec:
            raise ValueError("mixer is not available together with shard_matvec")
        self.mixer_activate()
        if resume_data is not None:
            self.sweeps = int(resume_data['sweeps'])
            if self._mixer_on:
                state = resume_data.get('mixer')
                self.mixer = None
                if state is not None:
                    self.mixer_activate(state['sweep_activated'])
                    self.mixer.amplitude = state['amplitude']
            for name in ('sweep_stats', 'update_stats'):
                for k, v in resume_data.get(name, {}).items():
                    getattr(self, name)[k] = list(v)
            if resume_data.get('chi_max') is not None:
                self.trunc_params['chi_max'] = resume_data['chi_max']
            if resume_data.get('lanczos_params') is not None:
                self.lanczos_params = dict(resume_data['lanczos_params'])

    def mixer_activate(self, sweep_activated=None):
        """(Re-)create the mixer from ``mixer_params`` (reference ``Sweep.mixer_activate``)."""
        if self._mixer_on:
            from . import mixer
            self.mixer = getattr(mixer, self.DefaultMixer)(self.options.get('mixer_params'), self.sweeps if sweep_activated is None else sweep_activated)

    def mixer_cleanup(self):
        """After a sweep: let the amplitude decay; drop the mixer when its time is over (reference ``Sweep.mixer_cleanup``)."""
        if self.mixer is not None:
            self.mixer = self.mixer.update_amplitude(self.sweeps)

    # ---- checkpoint / resume: the state (device arrays pickle through the host), counters, statistics --------------------
    def get_resume_data(self):
        """Not interchangeable with the reference's checkpoints (those hold TeNPy's own MPS class); environments are rebuilt
        from the state on demand."""
        mixer = None if self.mixer is None else {'amplitude': self.mixer.amplitude, 'sweep_activated': self.mixer.sweep_activated}
        return {'psi': self.psi, 'sweeps': self.sweeps, 'chi_max': self.trunc_params.get('chi_max'), 'mixer': mixer,
                'lanczos_params': dict(self.lanczos_params),
                'sweep_stats': {k: list(v) for k, v in self.sweep_stats.items()},
                'update_stats': {k: list(v) for k, v in self.update_stats.items()}}

    def save_checkpoint(self, filename):
        with open(filename, 'wb') as f:
            pickle.dump(self.get_resume_data(), f, protocol=4)

    @classmethod
    def from_checkpoint(cls, filename, model_H, options):
        with open(filename, 'rb') as f:
            data = pickle.load(f)
        return cls(data['psi'], model_H, options, resume_data=data)

    # ---- one sweep = 2 (L - 2) bond updates ----------------------------------------------------------------------------------
    def sweep(self):
        if self.chi_list is not None:
            due = [s for s in self.chi_list if s <= self.sweeps]
            if due:
                self.trunc_params['chi_max'] = self.chi_list[max(due)]
                # a sweep that is a key of chi_list switches the mixer on again (reference mps_common.py:377-382)
                if self.sweeps in self.chi_list and self.options.get('chi_list_reactivates_mixer', True):
                    self.mixer_activate()
        L = self.psi.L
        t0 = time.time()
        worst = 0.
        # The cyclic garbage collector is paused for the duration of a sweep: a bond update allocates ~2000 short-lived containers
        # (all freed by reference counting), which triggers a generation-0 pass every few hundred microseconds and, every ~100 bonds, a
        # full pass over the plan caches (10^5 objects) -- host time in front of an idle device.  Collected once per sweep instead.
        gc_was_on = _GC_PAUSE and gc.isenabled()
        if gc_was_on:
            gc.disable()
        try:
            for update in self._sweep_updates():
                worst = max(worst, update().eps)
        finally:
            if gc_was_on:
                gc.enable()
        self.sweeps += 1
        self.mixer_cleanup()
        st = self.sweep_stats
        st['sweep'].append(self.sweeps)
        st['E'].append(self.update_stats['E_total'][-1])
        st['S'].append(float(np.max(self.psi.entanglement_entropy())))
        st['time'].append(time.time() - t0)
        st['max_trunc_err'].append(worst)
        st['max_chi'].append(int(np.max(self.psi.chi)))
        return worst

    def _sweep_updates(self):
        """The updates of one sweep, in order, as calls that return the truncation error: 2 (L - 2) bond updates."""
        L = self.psi.L
        for i0 in range(L - 2):
            yield lambda i0=i0: self.update_bond(i0, move_right=True)
        for i0 in range(L - 2, 0, -1):
            yield lambda i0=i0: self.update_bond(i0, move_right=False)

    def update_bond(self, i0, move_right=True):
        t0 = time.time()
        psi, env = self.psi, self.env
        self._tick(None)
        if self.shard_matvec:
            from .sharded import ShardedTwoSiteH
            eff_H = ShardedTwoSiteH(env, i0, combine=True, move_right=move_right)
            # the row-panel tables of this bond's previous visit (validated by their keys in `matvec_program`): building them is
            # ~0.8 ms of host time per bond, with the device idle
            eff_H._sharded_cache = self.__dict__.setdefault('_sharded_plans', {}).setdefault(i0, {})
        else:
            eff_H = TwoSiteH(env, i0, combine=True, move_right=move_right)
        if getattr(self.H, 'explicit_plus_hc', False):
            eff_H = _plus_hc(eff_H)
        if not self.shard_matvec:
            # the contraction plans of this bond's previous visit (same block structure once chi has saturated: checked by their keys)
            eff_H.adopt_plans(self.__dict__.setdefault('_heff_plans', {}).get(i0))
        theta = eff_H.combine_theta(psi.get_theta(i0, n=2))
        self.eff_H = eff_H                                    # (the mixer looks at the operator itself, not at the projected one)
        if self.mixer is not None:
            # the HERK tables of this bond's previous visit (validated by the structure keys of their operands, like `_heff_plans`)
            plain = getattr(eff_H, 'plain', eff_H)           # (H + h.c.: the mixer works on the plain operator behind PlusHcH)
            if type(plain) is TwoSiteH:
                plain._mixplans = self.__dict__.setdefault('_mix_plans', {}).setdefault(i0, {})
        if self.ortho_to_envs:
            eff_H = self._wrap_ortho_eff_H(eff_H, i0, theta.get_leg_labels())
        self._tick('heff')
        if self.shard_matvec and self.options.get('krylov_row_panels', False):
            from .sharded import lanczos_row_panels          # north_star: Krylov vectors as row panels, scalars by all-reduce
            E0, theta, N = lanczos_row_panels(eff_H, theta, self.lanczos_params)
        else:
            E0, theta, N = LanczosGroundState(eff_H, theta, self.lanczos_params).run()
        kept = None if self.shard_matvec else eff_H.plans_to_keep()
        if kept is not None:
            self._heff_plans[i0] = kept
        theta = eff_H.prepare_svd(theta)                      # fused matrix [(vL.p0), (p1.vR)]
        self._tick('lanczos')
        previous = npc.SVD_DIST_GROUP
        npc.SVD_DIST_GROUP = self._svd_group                  # scoped to this call (other SVDs in the process stay local)
        # warm start of the block SVD: the right (left) singular vectors this bond produced on the previous visit span
        # theta_0 = M . B_{i0+1} (A_{i0} . M) of this one (linalg/_svd_warm.py); consumed by the next npc.svd call
        # (no hint on mixer updates: the decomposition is two eigh of density matrices, not an SVD of theta)
        npc.svd_hint = ((self._warm_token(), i0), 'R' if move_right else 'L') if self.mixer is None else None
        try:
            if self.mixer is None:
                U, S, VH, err, _ = svd_theta(theta, self.trunc_params, qtotal_LR=[psi.get_B(i0, None).qtotal, None],
                                             inner_labels=['vR', 'vL'])
            else:       # the side the sweep moves to is mixed; the total charges stay "as before" (reference dmrg.py:925-926)
                qL = psi.get_B(i0, None).qtotal
                U, S, VH, err, _ = self.mixer.mix_and_decompose_2site(self, theta, i0, mix_left=move_right, mix_right=not move_right,
                                                                      qtotal_LR=[qL, theta.chinfo.make_valid(theta.qtotal - qL)])
        finally:
            npc.SVD_DIST_GROUP = previous
            npc.svd_hint = None
        self._tick('svd')
        i1 = i0 + 1
        if move_right:
            eff_H.update_LP(env, i1, U)
        else:
            eff_H.update_RP(env, i0, VH)
        self._tick('env')
        psi.set_B(i0, U.split_legs(['(vL.p0)']).ireplace_label('p0', 'p'), form='A')
        psi.set_B(i1, VH.split_legs(['(p1.vR)']).ireplace_label('p1', 'p'), form='B')
        psi.set_SR(i0, S)
        env.invalidate(i0, i1, keep_LP=move_right, keep_RP=not move_right)
        for o_env in self.ortho_to_envs:
            o_env.invalidate(i0, i1)
        self._tick('setB')
        us = self.update_stats
        us['i0'].append(i0)
        us['E_total'].append(float(E0))
        us['N_lanczos'].append(N)
        us['time'].append(time.time() - t0)
        us['err'].append(err.eps)
        us['chi'].append(min(S.shape) if isinstance(S, npc.Array) else len(S))
        return err

    def _wrap_ortho_eff_H(self, eff_H, i0, labels):
        """The statements of the reference's ``_wrap_ortho_eff_H`` (mps_common.py:524-540): the states to stay orthogonal to as
        vectors of this bond, ``LP . theta_ket . RP`` of the ``<psi|ket>`` environments."""
        from ..linalg.sparse import OrthogonalNpcLinearOperator
        ortho_vecs = []
        for o_env in self.ortho_to_envs:
            theta = o_env.ket.get_theta(i0, n=2)
            theta = npc.tensordot(o_env.get_LP(i0, store=True), theta, axes=('vR', 'vL'))
            theta = npc.tensordot(theta, o_env.get_RP(i0 + 1, store=True), axes=('vR', 'vL'))
            theta.ireplace_labels(['vR*', 'vL*'], ['vL', 'vR'])
            theta = eff_H.combine_theta(theta)
            ortho_vecs.append(theta if list(theta.get_leg_labels()) == list(labels) else theta.transpose(labels))
        return OrthogonalNpcLinearOperator(eff_H, ortho_vecs)

    def _tick(self, phase):
        """Phase timer (the reference's DEBUG_PRINT phases, _npc_helper.pyx:13); synchronises only when profiling."""
        if not self.profile:
            return
        from ..linalg import _device as dev
        dev.torch().cuda.synchronize()
        now = time.time()
        if phase is not None:
            self.phase_time[phase] += now - self._t_phase
        self._t_phase = now


class SingleSiteDMRGEngine(TwoSiteDMRGEngine):
    """Single-site DMRG for finite chains (reference ``SingleSiteDMRGEngine``, dmrg.py:955-1140, ``combine=False``) with the subspace
    expansion of ``algorithms/mixer.py`` as its mixer.  The schedule is the reference's ``Sweep.get_sweep_schedule`` for one optimised
    site: sites 0 .. L - 2 moving right (``LP`` is updated), then L - 1 .. 1 moving left (``RP``).  Per update: the device ``OneSiteH``
    (its plans handed from visit to visit), ``LanczosGroundState``, ``prepare_svd``, ``mixed_svd``, ``set_B``, the environment.

    Options as for ``TwoSiteDMRGEngine`` with ``mixer``: ``True`` / ``'SubspaceExpansion'`` / ``None``, default ``True`` (the
    reference's ``use_mixer_by_default``).  While the mixer is on the bond next to the updated site holds a general 2D matrix
    (S . VH moving right, U . S moving left; the neighbouring tensor stays as it is); without it, 1D singular values.
    ``shard_matvec`` and ``orthogonal_to`` are not available."""
    DefaultMixer = 'SubspaceExpansion'
    use_mixer_by_default = True

    def __init__(self, psi, model_H, options, resume_data=None, orthogonal_to=None):
        if orthogonal_to:
            raise ValueError("orthogonal_to is not available for the stand-alone single-site engine")
        if dict(options).get('shard_matvec', False):
            raise ValueError("shard_matvec is not available for the stand-alone single-site engine")
        if psi.L < 2:
            raise ValueError("single-site DMRG needs at least two sites")
        super().__init__(psi, model_H, options, resume_data=resume_data)

    def get_sweep_schedule(self):
        """``(i0, move_right, (update_LP, update_RP))`` of one sweep (reference mps_common.py:438-444 with n = 1)."""
        L = self.psi.L
        return [(i0, True, (True, False)) for i0 in range(L - 1)] + [(i0, False, (False, True)) for i0 in range(L - 1, 0, -1)]

    def _sweep_updates(self):
        for i0, move_right, update_LP_RP in self.get_sweep_schedule():
            yield lambda a=(i0, move_right, update_LP_RP): self.update_site(*a)

    def prepare_svd(self, theta, move_right):
        """``theta`` as the matrix of the SVD: the physical leg points away from the direction of the move (reference :978-994)."""
        if move_right:
            return theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0)
        return theta.combine_legs(['p0', 'vR'], qconj=-1, new_axes=1)

    def mixed_svd(self, theta, i0, move_right):
        """``U [(vL.p), vR]``, ``S``, ``VH [vL, (p.vR)]``, ``err`` on the two sites of the bond (reference :996-1110): without a mixer the
        plain ``svd_theta`` with VH (U) absorbed into the next tensor; with the mixer its decomposition, S . VH (U . S) as the 2D bond
        matrix and the next tensor unchanged."""
        psi = self.psi
        if move_right:
            nxt = psi.get_B(i0 + 1, form='B').combine_legs(['p', 'vR'], qconj=-1, new_axes=1)
        else:
            nxt = psi.get_B(i0 - 1, form='A').combine_legs(['vL', 'p'], qconj=+1, new_axes=0)
        if self.mixer is None:
            qtotal = [theta.qtotal, None] if move_right else [None, theta.qtotal]
            U, S, VH, err, _ = svd_theta(theta, self.trunc_params, qtotal_LR=qtotal, inner_labels=['vR', 'vL'])
            if move_right:
                VH = npc.tensordot(VH, nxt, axes=['vR', 'vL'])
                U.ireplace_label('(vL.p0)', '(vL.p)')
            else:
                U = npc.tensordot(nxt, U, axes=['vR', 'vL'])
                VH.ireplace_label('(p0.vR)', '(p.vR)')
        else:
            U, S, VH, err = self.mixer.mix_and_decompose_1site(self, theta, i0, move_right)
            if move_right:
                S = npc.tensordot(S, VH, axes=['vR', 'vL']) if isinstance(S, npc.Array) else VH.iscale_axis(S, 'vL')
                VH = nxt
                U.ireplace_label('(vL.p0)', '(vL.p)')
            else:
                S = npc.tensordot(U, S, axes=['vR', 'vL']) if isinstance(S, npc.Array) else U.iscale_axis(S, 'vR')
                U = nxt
                VH.ireplace_label('(p0.vR)', '(p.vR)')
        return U, S, VH, err

    def update_site(self, i0, move_right, update_LP_RP=None):
        t0 = time.time()
        psi, env = self.psi, self.env
        update_LP, update_RP = update_LP_RP if update_LP_RP is not None else (move_right, not move_right)
        self._tick(None)
        eff_H = plain = OneSiteH(env, i0, combine=False, move_right=move_right)
        cache = self.__dict__.setdefault('_heff_plans', {})
        plain.adopt_plans(cache.get(i0))                      # the plans of this site's previous visit (validated by their keys)
        plain._expandplans = self.__dict__.setdefault('_expand_plans', {}).setdefault(i0, {})
        if getattr(self.H, 'explicit_plus_hc', False):
            eff_H = _plus_hc(eff_H)
        theta = plain.combine_theta(psi.get_theta(i0, n=1))
        self.eff_H = plain                                    # (the mixer looks at the plain operator)
        self._tick('heff')
        E0, theta, N = LanczosGroundState(eff_H, theta, self.lanczos_params).run()
        kept = plain.plans_to_keep()
        if kept is not None:
            cache[i0] = kept
        theta = self.prepare_svd(theta, move_right)
        self._tick('lanczos')
        U, S, VH, err = self.mixed_svd(theta, i0, move_right)
        self._tick('svd')
        i_L, i_R = (i0, i0 + 1) if move_right else (i0 - 1, i0)
        psi.set_B(i_L, U.split_legs(['(vL.p)']), form='A')
        psi.set_B(i_R, VH.split_legs(['(p.vR)']), form='B')
        psi.set_SR(i_L, S)
        self._tick('setB')
        env.invalidate(i_L, i_R, keep_LP=False, keep_RP=False)
        if update_LP:
            plain.update_LP(env, i_R, U)
        if update_RP:
            plain.update_RP(env, i_L, VH)
        self._tick('env')
        us = self.update_stats
        us['i0'].append(i0)
        us['E_total'].append(float(E0))
        us['N_lanczos'].append(N)
        us['time'].append(time.time() - t0)
        us['err'].append(err.eps)
        us['chi'].append(min(S.shape) if isinstance(S, npc.Array) else len(S))
        return err
