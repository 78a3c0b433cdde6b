"""Minimal TDVP drivers for boxes WITHOUT TeNPy (the ``-m gpu`` tests): finite chains, real-time step ``dt``, time-independent
``H`` (MPOs with ``explicit_plus_hc``: ``H + h.c.``), no mixer.  Where TeNPy is installed, its own ``tenpy.algorithms.tdvp`` engines run unchanged on the device
mirror (``tenpy_amd.install.install(fused=True)`` hands them the device ``LanczosEvolution`` / ``OneSiteH`` / ``ZeroSiteH``).

This file only issues the npc calls of the reference's sweeps in the reference's order (tdvp.py:253-315 two-site: evolve theta by
``-i dt/2`` -- doubled at the turning bond --, ``svd_theta``, ``set_B`` A / B, environment update, backward one-site evolution by
``+i dt/2``; :335-425 single-site: one-site evolve, untruncated SVD, backward zero-site evolution of the bond matrix, absorbed into
the neighbour in form ``'Th'``).  Options (names as in the reference): ``dt``, ``N_steps``, ``trunc_params``, ``lanczos_params``, ``preserve_norm``.
"""
import numpy as np

from ..linalg import np_conserved as npc
from ..linalg.krylov_based import LanczosEvolution
from ..linalg.truncation import svd_theta
from ..networks.mpo import MPOEnvironment
from .dmrg import _plus_hc
from .mps_common import OneSiteH, TwoSiteH, ZeroSiteH

__all__ = ['TwoSiteTDVPEngine', 'SingleSiteTDVPEngine']


class _TDVPEngine:
    def __init__(self, psi, model_H, options):
        if not psi.finite:
            raise NotImplementedError("Only finite TDVP is implemented")
        self.psi, self.H = psi, model_H
        self.options = options = dict(options)
        self.dt = options.get('dt', 0.1)
        self.N_steps = int(options.get('N_steps', 1))
        self.trunc_params = dict(options.get('trunc_params', {}))
        self.lanczos_params = dict(options.get('lanczos_params', {}))
        self.env = MPOEnvironment(psi, model_H)
        self.evolved_time = 0.
        self.trunc_err_list = []

    def run(self):
        """Evolve by ``N_steps * dt``.  ``preserve_norm`` (default: real ``dt``) puts ``psi.norm`` back to its value before the steps, as
        the reference does (algorithm.py:431-442): what a truncation takes off the norm is not decay."""
        preserve_norm = self.options.get('preserve_norm')
        if preserve_norm is None:
            preserve_norm = not np.iscomplex(self.dt)
        old_norm = self.psi.norm
        for _ in range(self.N_steps):
            self.sweep()
        if preserve_norm:
            self.psi.norm = old_norm
        self.evolved_time += self.N_steps * self.dt
        return self.psi

    def _krylov_evolve(self, H, theta, dt):
        return LanczosEvolution(H, theta, self.lanczos_params).run(dt, normalize=self.lanczos_params.get('normalize'))

    def _hc(self, eff_H):
        """The operator the evolution sees: ``eff_H``, plus its h.c. for an MPO with ``explicit_plus_hc`` (reference tdvp.py:310, :422)."""
        return _plus_hc(eff_H) if getattr(self.H, 'explicit_plus_hc', False) else eff_H

    def _site_changed(self, i):
        """Drop every stored environment that contains site ``i``."""
        self.env.invalidate(i, i, keep_LP=True, keep_RP=True)


class TwoSiteTDVPEngine(_TDVPEngine):
    def sweep(self):
        L = self.psi.L
        for i0 in range(L - 2):
            self.update_local(i0, True)
        for i0 in range(L - 2, 0, -1):
            self.update_local(i0, False)
        self.update_local(0, None)

    def update_local(self, i0, move_right):
        psi, env, i1 = self.psi, self.env, i0 + 1
        eff_H = self._hc(TwoSiteH(env, i0, combine=True, move_right=move_right is not False))
        theta = eff_H.combine_theta(psi.get_theta(i0, n=2))
        dt = -0.5j * self.dt
        if i0 == psi.L - 2:
            dt = 2. * dt        # instead of updating the last pair of sites twice, the time is doubled
        theta, N = self._krylov_evolve(eff_H, theta, dt)
        theta = eff_H.prepare_svd(theta)
        U, S, VH, err, renorm = svd_theta(theta, self.trunc_params, qtotal_LR=[psi.get_B(i0, None).qtotal, None],
                                          inner_labels=['vR', 'vL'])
        psi.norm *= renorm
        self.trunc_err_list.append(err.eps)
        if move_right:
            eff_H.update_LP(env, i1, U)
        elif move_right is False:
            eff_H.update_RP(env, i0, VH)
        psi.set_B(i0, U.split_legs(['(vL.p0)']).ireplace_label('p0', 'p'), form='A')
        psi.set_B(i1, VH.split_legs(['(p1.vR)']).ireplace_label('p1', 'p'), form='B')
        psi.set_SR(i0, S)
        env.invalidate(i0, i1, keep_LP=move_right is True, keep_RP=move_right is False)
        if move_right:
            self.one_site_update(i1, 0.5j * self.dt)
        elif move_right is False:
            self.one_site_update(i0, 0.5j * self.dt)
        return {'err': err, 'N': N}

    def one_site_update(self, i, dt):
        H1 = self._hc(OneSiteH(self.env, i, combine=False))
        theta = H1.combine_theta(self.psi.get_theta(i, n=1))
        theta, _ = self._krylov_evolve(H1, theta, dt)
        self.psi.set_B(i, theta.replace_label('p0', 'p'), form='Th')        # (stored environments hold i on neither side here)


class SingleSiteTDVPEngine(_TDVPEngine):
    def sweep(self):
        L = self.psi.L
        for i0 in range(L - 1):
            self.update_local(i0, True)
        for i0 in range(L - 1, 0, -1):
            self.update_local(i0, False)
        self.update_local(0, None)

    def update_local(self, i0, move_right):
        eff_H = self._hc(OneSiteH(self.env, i0, combine=False, move_right=move_right is not False))
        theta = eff_H.combine_theta(self.psi.get_theta(i0, n=1))
        dt = -0.5j * self.dt
        if i0 == self.psi.L - 1:
            dt = 2. * dt
        theta, N = self._krylov_evolve(eff_H, theta, dt)
        if move_right:
            self.right_moving_update(i0, theta)
        else:
            self.left_moving_update(i0, theta)
        self.trunc_err_list.append(0.)
        return {'N': N}

    def _svd(self, theta, qtotal_LR):
        U, S, VH = npc.svd(theta, qtotal_LR=qtotal_LR, inner_labels=['vR', 'vL'])
        renorm = float(np.linalg.norm(S))
        self.psi.norm *= renorm
        return U, S / renorm, VH

    def right_moving_update(self, i0, theta):
        psi = self.psi
        theta = theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0)
        U, S, VH = self._svd(theta, [theta.qtotal, None])
        psi.set_B(i0, U.split_legs(['(vL.p0)']).replace_label('p0', 'p'), form='A')
        psi.set_SR(i0, S)
        self._site_changed(i0)
        theta = self.zero_site_update(i0 + 1, VH.scale_axis(S, 'vL'), 0.5j * self.dt)
        psi.set_B(i0 + 1, npc.tensordot(theta, psi.get_B(i0 + 1, form='B'), axes=['vR', 'vL']), form='Th')
        self._site_changed(i0 + 1)

    def left_moving_update(self, i0, theta):
        psi = self.psi
        theta = theta.combine_legs(['p0', 'vR'], qconj=-1, new_axes=1)
        U, S, VH = self._svd(theta, [None, theta.qtotal])
        if i0 == 0:
            assert U.shape == (1, 1)
            VH = VH * U.to_ndarray()[0, 0]        # just a global phase, but better keep it
        psi.set_B(i0, VH.split_legs(['(p0.vR)']).replace_label('p0', 'p'), form='B')
        psi.set_SL(i0, S)
        if i0 != 0:
            self._site_changed(i0)
            theta = self.zero_site_update(i0, U.scale_axis(S, 'vR'), 0.5j * self.dt)
            psi.set_B(i0 - 1, npc.tensordot(psi.get_B(i0 - 1, form='A'), theta, axes=['vR', 'vL']), form='Th')
            self._site_changed(i0 - 1)

    def zero_site_update(self, i, theta, dt):
        """Zero-site update of the bond matrix left of site ``i``."""
        theta, _ = self._krylov_evolve(self._hc(ZeroSiteH(self.env, i)), theta, dt)
        return theta
