"""The reduced density matrices of the density-matrix mixer on the device (reference ``DensityMatrixMixer.mix_rho``,
mps_common.py:1972-2027).

    rho_L = X diag(mix_L) X^dagger,   X = LP . theta . W0   [rows (vR*, p0) | wR, p1, vR]
    rho_R = X diag(mix_R) X^dagger,   X = theta . RP . W1   [vL, p0, wL | rows (p1, vL*)]

The reference forms X through ``LHeff`` / ``RHeff`` and the product as a general tensordot of ``X`` scaled along ``wR`` with a
conjugated copy.  Here the product is ONE launch of ``tpa_herk_chain`` (include/tenpy_amd.h, K1h) over the blocks of X: a block of X
is a link, the MPO bond leg supplies the weights (a scalar per link for bond blocks of width 1, the periodic form for wider blocks),
a pair of pipe slices inside a charge sector is a task -- Hermitian on the diagonal, with a mirror below it -- and only the tiles on
and below the diagonal of a sector are computed.  With a factored ``TwoSiteH`` X is built from ``LP . theta`` (contracted index chi,
not d chi) and the MPO tensor; ``LHeff`` / ``RHeff`` are not built.

``device_mix_rho`` returns ``None`` where this route does not apply (the caller then issues the reference's statements): an operator
that is neither a plain ``TwoSiteH``, its module form, nor a ``PlusHcH`` around one (sharded operators, sums of operators), infinite
systems, ``bra is not ket``, mixed dtypes, charged environments, ``TPA_MIXER_DEVICE=0``.

MPOs with ``explicit_plus_hc`` (the tensors hold half of H): the reference takes the tensors of the plain operator, the weights of
``_mix_LR`` with ``one = 0.5`` and adds ``rho + rho^dagger`` (:2007, :2021).  ``X diag(s) X^dagger`` with real ``s`` is Hermitian, so
``rho + rho^dagger = 2 rho = X diag(2 s) X^dagger``: the factor 2 goes on the weights (exact, a power of two), the kernel's result is
Hermitian bit for bit, and the unmixed term of ``IdL is None`` is added afterwards as in the reference."""
import os

import numpy as np

from ..linalg import _device as dev
from ..linalg import _herk
from ..linalg import np_conserved as npc
from ..linalg.charges import LegPipe
from ..linalg.truncation import svd_theta, truncate
from . import mps_common

stats = {'device_mix_rho': 0, 'declined': 0, 'plans_built': 0, 'why': {}, 'device_expand': 0, 'expand_declined': 0, 'expand_plans_built': 0}


def enabled():
    return os.environ.get('TPA_MIXER_DEVICE', '1') != '0'


def mix_weights(H, i0, amplitude):
    """``(mix_L, mix_R, IdL, IdR)`` of the bond right of site ``i0`` (reference ``_mix_LR``, mps_common.py:1846-1882)."""
    chi = H.get_W(i0).get_leg('wR').ind_len
    if hasattr(H, 'get_IdL'):
        IdL, IdR = H.get_IdL(i0 + 1), H.get_IdR(i0)
    elif getattr(H, 'IdL_bonds', None) is not None:       # one index per bond (an MPO taken over from elsewhere): bond j is left of site j
        IdL, IdR = H.IdL_bonds[i0 + 1], H.IdR_bonds[i0 + 1]
    else:
        IdL, IdR = H.IdL, H.IdR
    IdL = None if IdL is None else int(IdL) % chi
    IdR = None if IdR is None else int(IdR) % chi
    mix_L, mix_R = np.full(chi, float(amplitude)), np.full(chi, float(amplitude))
    one = 0.5 if getattr(H, 'explicit_plus_hc', False) else 1.
    if IdL is not None:
        mix_L[IdL], mix_R[IdL] = one, 0.
    if IdR is not None:
        mix_L[IdR], mix_R[IdR] = 0., one
    return mix_L, mix_R, IdL, IdR


class _Source:
    """How one operand X enters a plan: its row axes (the incoming legs of the pipe, or the pipe itself), the MPO bond axis that
    carries the weights (or None) and whether the rows are the first or the last axes."""

    def __init__(self, X, n_row, rows_first, w_axis):
        self.X = X
        self.n_row, self.rows_first, self.w_axis = n_row, rows_first, w_axis
        self.fused = n_row == 1

    @property
    def key(self):
        return (self.X._struct_key(), self.n_row, self.rows_first, self.w_axis)


class RhoPlan:
    """Tables of ``tpa_herk_chain`` for ``rho = sum_sources X diag(s) X^dagger`` on the charge sectors of ``pipe``; the first source
    overwrites, every further source accumulates (``IdL is None``: the unmixed term on theta's arena, reference :2009, :2023).
    Every block of a sector that some source populates is written completely: tasks without links are included."""

    def __init__(self, pipe, Xs, sources, dtype):
        self.dtype = np.dtype(dtype)
        self._w_host = self._w_dev = None
        self.key = tuple(s.key for s in sources)
        bt = _herk.tile_rows(self.dtype)
        is_pipe = isinstance(pipe, LegPipe)
        sizes = pipe.get_block_sizes()
        per_source, sectors = [], set()
        for X, s in zip(Xs, sources):
            qd, offs, shapes = X._qdata, X._offsets, X._block_shapes()
            rank = X.rank
            row_axes = list(range(s.n_row)) if s.rows_first else list(range(rank - s.n_row, rank))
            other = [a for a in range(rank) if a not in row_axes]
            if s.fused:         # the row leg is the pipe itself: a block covers its whole sector
                X.legs[row_axes[0]].test_contractible(pipe.conj())
                q = qd[:, row_axes[0]]
                sl = np.stack([np.zeros(len(qd), np.int64), sizes[q], q], axis=1).astype(np.int64)
            else:               # the row legs are the incoming legs of the pipe: a block covers one slice of its sector
                for a, leg in zip(row_axes, pipe.legs):
                    X.legs[a].test_contractible(leg.conj())
                sl = pipe.q_map[pipe._map_incoming_qind(qd[:, row_axes]), :3].astype(np.int64)
            blocks = {}
            for b in range(len(qd)):
                m = int(np.prod(shapes[b, row_axes]))
                w = int(shapes[b, s.w_axis]) if s.w_axis is not None else 1
                k = int(np.prod(shapes[b, other]))
                rs, ks = (k, 1) if s.rows_first else (1, m)
                w_inner = int(np.prod(shapes[b, [a for a in other if a > s.w_axis]])) if s.w_axis is not None else 1
                w_off = int(X.legs[s.w_axis].slices[qd[b, s.w_axis]]) if s.w_axis is not None else -1
                assert m == sl[b, 1] - sl[b, 0]
                sec, b0 = int(sl[b, 2]), int(sl[b, 0])
                blocks.setdefault(sec, {}).setdefault(b0, {})[tuple(qd[b, other].tolist())] = (int(offs[b]), k, rs, ks, w_off, w, w_inner)
                sectors.add(sec)
            per_source.append(blocks)
        self.sectors = np.array(sorted(sectors), np.int64)
        sec_off = np.concatenate([[0], np.cumsum(sizes[self.sectors] ** 2)]).astype(np.int64)
        self.total = int(sec_off[-1])
        self.offsets = sec_off[:-1].copy()
        self.qdata = np.stack([self.sectors, self.sectors], axis=1).astype(np.intp)
        if is_pipe and pipe.q_map is not None:
            slices_of = {int(q): sorted((int(r[0]), int(r[1])) for r in pipe.q_map[pipe.q_map[:, 2] == q]) for q in self.sectors}
        else:
            slices_of = {int(q): [(0, int(sizes[q]))] for q in self.sectors}
        self.launches = []
        self.flops = 0              # of the full product (both triangles), as a general GEMM would execute it
        self.flops_tiles = 0        # of the tiles that are scheduled (on and below the diagonal of every sector; edge tiles by their real size)
        for si, blocks in enumerate(per_source):
            tasks, links = [], []
            for q, base in zip(self.sectors.tolist(), self.offsets.tolist()):
                ld = int(sizes[q])
                mine = blocks.get(q, {})
                if si > 0 and not mine:
                    continue                      # an accumulating source has nothing to add to this sector
                sl = [(0, ld)] if sources[si].fused else slices_of[q]
                for ip, (p0, p1) in enumerate(sl):
                    for (r0, r1) in sl[:ip + 1]:
                        A, B = mine.get(p0, {}), mine.get(r0, {})
                        l0 = len(links)
                        for ck in sorted(set(A) & set(B)):
                            (a_off, k, rs, ks, w_off, w, w_inner), (b_off, _, b_rs, b_ks) = A[ck], B[ck][:4]
                            links.append(_herk.link_row(a_off, b_off, k, rs, ks, b_rs, b_ks, w_off, w, w_inner))
                            self.flops += 2 * k * (p1 - p0) * (r1 - r0) * (1 if p0 == r0 else 2)
                        if p0 == r0:
                            tasks.append(_herk.task_row(base + p0 * ld + p0, p1 - p0, p1 - p0, ld, l0, len(links) - l0, int(si > 0), 1))
                        else:
                            tasks.append(_herk.task_row(base + p0 * ld + r0, p1 - p0, r1 - r0, ld, l0, len(links) - l0, int(si > 0), 0,
                                                        base + r0 * ld + p0, ld))
            tasks = np.array(tasks, np.int64).reshape(-1, _herk.TASK_W)
            links = np.array(links, np.int64).reshape(-1, _herk.LINK_W)
            if len(links) == 0:
                links = np.zeros((1, _herk.LINK_W), np.int64)
            tiles = _herk.tile_table(tasks, links, bt)
            if len(tiles):
                kcum = np.concatenate([[0], np.cumsum(np.maximum(links[:, 2], 0))])
                tt = tasks[tiles[:, 0]]
                area = np.minimum(bt, tt[:, 1] - tiles[:, 1] * bt) * np.minimum(bt, tt[:, 2] - tiles[:, 2] * bt)
                self.flops_tiles += int(np.sum(2 * (kcum[tt[:, 4] + tt[:, 5]] - kcum[tt[:, 4]]) * area))
            self.launches.append(dev.to_device_packed(tasks, links, tiles) + (len(tiles),))
        stats['plans_built'] += 1

    def apply(self, pipe, Xs, weights, labels):
        rho = npc.Array([pipe, pipe.conj()], self.dtype, labels=labels)
        arena = dev.empty(self.total, self.dtype)
        wd = None
        if weights is not None:      # the device copy of the weights stays with the plan (one upload per bond and amplitude)
            w = np.ascontiguousarray(weights, np.float64)
            if self._w_host is None or not np.array_equal(self._w_host, w):
                self._w_host, self._w_dev = w.copy(), dev.to_device(w)
            wd = self._w_dev
        for X, (tasks, links, tiles, n_tiles) in zip(Xs, self.launches):
            _herk.herk_chain(self.dtype, tasks, links, tiles, n_tiles, X._arena, X._arena, wd, arena)
        rho._adopt_blocks(self.qdata, self.offsets, arena, True)
        return rho


def _rho(eff_H, side, pipe, Xs, sources, weights, labels, dtype, handover):
    """``handover``: the structure keys of theta, ``LP``, ``RP`` and the two MPO tensors.  A plan handed over from the previous visit of the bond is
    validated by them (the structure of X follows from them); the structure key of X itself is only computed when a plan is built."""
    cache = eff_H.__dict__.setdefault('_mixplans', {})
    plan = cache.get(side)
    if plan is None or plan.handover != handover or plan.dtype != np.dtype(dtype) or len(plan.launches) != len(Xs):
        plan = cache[side] = RhoPlan(pipe, Xs, sources, dtype)
        plan.handover = handover
    return plan.apply(pipe, Xs, weights, labels)


def _apply_mpo(T, W, left, out_labels):
    """One MPO tensor applied to ``T`` with the other physical leg as a spectator: W0 going left to right (``left``), else W1 going
    right to left.  ``MpoApplyPlan`` (MPO blocks that are single numbers) works on whole blocks of ``T`` whatever its further legs: one
    ``tpa_lincomb_batch`` launch, written in the leg order the HERK wants.  The block and entry plan classes lay out their jobs for
    the legs of a one-site vector; for those MPOs X is the generic ``tensordot`` and a transposing copy."""
    if mps_common._mpo_plan_class(W) is mps_common.MpoApplyPlan:
        return (mps_common._mpo_step_lr if left else mps_common._mpo_step_rl)(T, W, out_labels=out_labels).apply(T)
    x_w, x_p, w_in, _, _, p_in = mps_common._STEP_LR if left else mps_common._STEP_RL
    return npc.tensordot(T, W, axes=([x_w, x_p], [w_in, p_in])).transpose(list(out_labels))


def _declines(eff_H, H, theta):
    """Why the device route does not take this call (counted in ``stats['why']``), or ``None``."""
    # the plain operator of the stand-alone driver, or its module form (which names the reference's class it stands in for)
    if not enabled():
        return 'switched off'
    if not (type(eff_H) is mps_common.TwoSiteH or (isinstance(eff_H, mps_common.TwoSiteH) and
                                                   getattr(type(eff_H), '_reference_class', None) is not None)):
        return 'operator'
    if not getattr(H, 'finite', True):
        return 'infinite'
    if not dev.lib_provides('tpa_herk_chain'):      # an emulation that predates the entry point: never forwarded to the real library
        return 'entry point'
    env = getattr(eff_H, '_env', None)
    if env is not None and getattr(env, 'bra', None) is not getattr(env, 'ket', None):
        return 'bra is not ket'
    if len({np.dtype(t.dtype) for t in (theta, eff_H.LP, eff_H.RP, eff_H.W0, eff_H.W1)}) != 1:
        return 'mixed dtypes'
    if np.any(eff_H.LP.qtotal != 0) or np.any(eff_H.RP.qtotal != 0):
        return 'charged environment'
    if theta.stored_blocks == 0:
        return 'empty theta'
    return None


def device_mix_rho(eff_H, H, theta, i0, amplitude, mix_left, mix_right, weights=None):
    """``(rho_L, rho_R)`` with the legs and labels of the reference's ``mix_rho`` after its transpositions: ``['(vL.p0)', '(vL*.p0*)']``
    on ``[pipeL, pipeL.conj()]`` and ``['(p1.vR)', '(p1*.vR*)']`` on ``[pipeR, pipeR.conj()]``, block diagonal with every block of a
    populated sector complete and Hermitian bit for bit; or ``None`` where the route declines (module docstring).
    ``theta``: the two-site wave function as ``[(vL.p0), (p1.vR)]`` or ``[vL, p0, p1, vR]``.  ``weights``: ``(mix_L, mix_R, IdL, IdR)``
    in place of ``mix_weights(H, i0, amplitude)``."""
    if isinstance(eff_H, mps_common.PlusHcH):        # the mixer works on the tensors of the plain operator (module docstring)
        eff_H = eff_H.plain
    why = _declines(eff_H, H, theta)
    if why is not None:
        stats['declined'] += 1
        stats['why'][why] = stats['why'].get(why, 0) + 1
        return None
    mix_L, mix_R, IdL, IdR = weights if weights is not None else mix_weights(H, i0, amplitude)
    if getattr(H, 'explicit_plus_hc', False):         # rho + rho^dagger = X diag(2 s) X^dagger
        mix_L, mix_R = 2. * np.asarray(mix_L), 2. * np.asarray(mix_R)
    pipeL, pipeR = eff_H.pipeL, eff_H.pipeR
    th2 = theta if theta.rank == 2 else theta.combine_legs([['vL', 'p0'], ['p1', 'vR']], pipes=[pipeL, pipeR])
    th2 = th2 if list(th2.get_leg_labels()) == ['(vL.p0)', '(p1.vR)'] else th2.transpose(['(vL.p0)', '(p1.vR)'])
    th4 = None
    if eff_H.factored and (mix_left or mix_right):
        th4 = eff_H.combine_theta(theta)                                         # vL, p0, p1, vR
    dtype = theta.dtype
    handover = (th2._struct_key(), eff_H.LP._struct_key(), eff_H.RP._struct_key(), eff_H.W0._struct_key(), eff_H.W1._struct_key())
    plain_L, plain_R = _Source(th2, 1, True, None), _Source(th2, 1, False, None)
    # ---- left
    if mix_left:
        if eff_H.factored:
            T1 = npc.tensordot(eff_H._LPf, th4, axes=['vR', 'vL'])              # vR*, wR, p0, p1, vR  (contracted index: chi)
            X = _apply_mpo(T1, eff_H.W0, True, ('vR*', 'p0', 'wR', 'p1', 'vR'))
            src = _Source(X, 2, True, 2)
        else:
            X = npc.tensordot(eff_H.LHeff, th2, axes=['(vR.p0*)', '(vL.p0)'])    # (vR*.p0), wR, (p1.vR): the first GEMM of the matvec
            src = _Source(X, 1, True, 1)
        Xs, sources = [X], [src]
        if IdL is None:
            Xs, sources = Xs + [th2], sources + [plain_L]
        rho_L = _rho(eff_H, 'L', pipeL, Xs, sources, mix_L, ['(vL.p0)', '(vL*.p0*)'], dtype, handover)
    else:
        rho_L = _rho(eff_H, 'L0', pipeL, [th2], [plain_L], None, ['(vL.p0)', '(vL*.p0*)'], dtype, handover)
    # ---- right
    if mix_right:
        if eff_H.factored:
            T1 = npc.tensordot(th4, eff_H._RPf, axes=['vR', 'vL'])              # vL, p0, p1, wL, vL*
            X = _apply_mpo(T1, eff_H.W1, False, ('vL', 'p0', 'wL', 'p1', 'vL*'))
            src = _Source(X, 2, False, 2)
        else:
            X = npc.tensordot(th2, eff_H.RHeff, axes=['(p1.vR)', '(p1*.vL)'])    # (vL.p0), wL, (p1.vL*)
            src = _Source(X, 1, False, 1)
        Xs, sources = [X], [src]
        if IdR is None:
            Xs, sources = Xs + [th2], sources + [plain_R]
        rho_R = _rho(eff_H, 'R', pipeR, Xs, sources, mix_R, ['(p1.vR)', '(p1*.vR*)'], dtype, handover)
    else:
        rho_R = _rho(eff_H, 'R0', pipeR, [th2], [plain_R], None, ['(p1.vR)', '(p1*.vR*)'], dtype, handover)
    stats['device_mix_rho'] += 1
    return rho_L, rho_R


def generic_mix_rho(eff_H, H, theta, i0, amplitude, mix_left, mix_right, weights=None):
    """The same density matrices by generic ``npc`` calls through ``LHeff`` / ``RHeff`` (the route of the reference, :2000-2026):
    what ``DensityMatrixMixer.mix_rho`` issues where ``device_mix_rho`` declines."""
    mix_L, mix_R, IdL, IdR = weights if weights is not None else mix_weights(H, i0, amplitude)
    plus_hc = bool(getattr(H, 'explicit_plus_hc', False))
    if theta.rank != 2:
        theta = theta.combine_legs([['vL', 'p0'], ['p1', 'vR']], pipes=[eff_H.pipeL, eff_H.pipeR])

    def plain(left):
        if left:
            return npc.tensordot(theta, theta.conj(), axes=['(p1.vR)', '(p1*.vR*)'])
        return npc.tensordot(theta.conj(), theta, axes=['(vL*.p0*)', '(vL.p0)'])
    if mix_left:
        X = npc.tensordot(eff_H.LHeff, theta, axes=['(vR.p0*)', '(vL.p0)']).ireplace_label('(vR*.p0)', '(vL.p0)')
        rho_L = npc.tensordot(X.scale_axis(mix_L, 'wR'), X.conj(), axes=[['wR', '(p1.vR)'], ['wR*', '(p1*.vR*)']])
        if plus_hc:
            rho_L = rho_L + rho_L.conj().itranspose()
        if IdL is None:
            rho_L = rho_L + plain(True)
    else:
        rho_L = plain(True)
    if mix_right:
        X = npc.tensordot(theta, eff_H.RHeff, axes=['(p1.vR)', '(p1*.vL)']).ireplace_label('(p1.vL*)', '(p1.vR)')
        rho_R = npc.tensordot(X.conj(), X.scale_axis(mix_R, 'wL'), axes=[['wL*', '(vL*.p0*)'], ['wL', '(vL.p0)']])
        if plus_hc:
            rho_R = rho_R + rho_R.conj().itranspose()
        if IdR is None:
            rho_R = rho_R + plain(False)
    else:
        rho_R = plain(False)
    return rho_L.itranspose(['(vL.p0)', '(vL*.p0*)']), rho_R.itranspose(['(p1.vR)', '(p1*.vR*)'])


# ---------------------------------------------------------------------------------------------------------------------
# Subspace expansion of single-site DMRG (reference ``SubspaceExpansion``, mps_common.py:2082-2201).  Moving right the reference
# decomposes
#     theta_expand[(vL.p0), (wR.vR)] = LHeff . diag(mix_L on wR) . theta
# (moving left ``theta . diag(mix_R on wL) . RHeff`` as ``[(vL.wL), (p0.vR)]``) and gets it through ``LHeff``, a scaling pass, a
# tensordot over the fused leg of length d chi and a ``combine_legs`` copy.  With a factored ``OneSiteH`` the same matrix is
# ``T1 = LP . theta`` -- a GEMM over chi, the first step of the matvec -- and ONE ``tpa_mpo_expand_batch`` launch that applies W0 entry by
# entry with the weights multiplied in and writes straight into the charge blocks of the fused matrix (``mps_common.MpoExpandPlan``).
def expand_enabled():
    return os.environ.get('TPA_EXPAND_DEVICE', '1') != '0'


def _expand_declines(eff_H, H, theta):
    """Why the device route of the subspace expansion does not take this call (counted in ``stats['why']``), or ``None``."""
    if not expand_enabled():
        return 'switched off'
    if not ((type(eff_H) is mps_common.OneSiteH or (isinstance(eff_H, mps_common.OneSiteH) and
                                                    getattr(type(eff_H), '_reference_class', None) is not None))
            and getattr(eff_H, 'factored', False)):
        return 'operator'
    if getattr(H, 'explicit_plus_hc', False):        # (the stacked form with the adjoint part: the generic route serves it)
        return 'explicit_plus_hc'
    if not getattr(H, 'finite', True):
        return 'infinite'
    if not dev.lib_provides('tpa_mpo_expand_batch'):      # an emulation that predates the entry point: never forwarded to the real library
        return 'entry point'
    env = getattr(eff_H, '_env', None)
    if env is not None and getattr(env, 'bra', None) is not getattr(env, 'ket', None):
        return 'bra is not ket'
    if len({np.dtype(t.dtype) for t in (theta, eff_H.LP, eff_H.RP, eff_H.W0)}) != 1:
        return 'mixed dtypes'
    if np.any(eff_H.LP.qtotal != 0) or np.any(eff_H.RP.qtotal != 0):
        return 'charged environment'
    if theta.stored_blocks == 0:
        return 'empty theta'
    return None


def _expand_weights(H, i0, amplitude, move_right, weights):
    """``(mix, Id, proj)`` on the outgoing MPO bond leg of site ``i0``: the weights (``mix_L`` of the bond to the right, moving right;
    ``mix_R`` of the bond to the left), the index whose slice is the unperturbed theta and -- that index is ``None``: the stacked form
    -- the mask of the indices that stay next to theta itself.  ``amplitude`` as the mixer holds it: the weights carry its root, so
    that it means the same for both mixers (reference :2134-2138)."""
    bond = i0 if move_right else i0 - 1
    mix_L, mix_R, IdL, IdR = weights if weights is not None else mix_weights(H, bond, np.sqrt(amplitude))
    mix, Id = (mix_L, IdL) if move_right else (mix_R, IdR)
    proj = None
    if Id is None:
        proj = np.ones(len(mix), bool)
        for k in (IdL, IdR):
            if k is not None:
                proj[k] = False
        mix = np.full(len(mix), float(np.sqrt(amplitude)))
    return np.asarray(mix, np.float64), Id, proj


def device_expand_1site(eff_H, H, theta, i0, amplitude, move_right, weights=None):
    """``(theta_expand, Id)``: the matrix that ``SubspaceExpansion.mix_and_decompose_1site`` hands to ``svd_theta``, with the legs and
    labels of the reference after its ``combine_legs`` -- ``['(vL.p0)', '(wR.vR)']`` moving right, ``['(vL.wL)', '(p0.vR)']`` moving
    left -- and the index of the outgoing MPO bond leg whose slice is the unperturbed theta (0 in the stacked form); or ``None``
    where the route declines (``_expand_declines``).  ``theta``: ``[vL, p0, vR]``, or prepared for the SVD as ``[(vL.p0), vR]`` /
    ``[vL, (p0.vR)]`` -- its pipe is then the pipe of the result.  ``weights``: ``(mix_L, mix_R, IdL, IdR)`` in place of
    ``mix_weights(H, bond, sqrt(amplitude))``."""
    why = _expand_declines(eff_H, H, theta)
    if why is not None:
        stats['expand_declined'] += 1
        stats['why'][why] = stats['why'].get(why, 0) + 1
        return None
    mix, Id, proj = _expand_weights(H, i0, amplitude, move_right, weights)
    pipe = None
    if theta.rank == 2:
        want = ['(vL.p0)', 'vR'] if move_right else ['vL', '(p0.vR)']
        theta = theta if list(theta.get_leg_labels()) == want else theta.transpose(want)
        pipe = theta.legs[0 if move_right else 1]
        theta = theta.split_legs()
    th3 = eff_H.combine_theta(theta)                                            # vL, p0, vR
    if move_right:          # vR*, wR, p0, vR (contracted index: chi, not d chi): the first GEMM of the matvec, by its cached plan p1
        fp = eff_H._plans(th3)
        T1 = fp['p1'].apply(eff_H._LPf, th3) if fp is not None else npc.tensordot(eff_H._LPf, th3, axes=['vR', 'vL'])
    else:                   # vL, p0, wL, vL* (the matvec has no such step: the plan cache of `tensordot`)
        T1 = npc.tensordot(th3, eff_H._RPf, axes=['vR', 'vL'])
    handover = (th3._struct_key(), eff_H.LP._struct_key(), eff_H.RP._struct_key(), eff_H.W0._struct_key(), bool(move_right),
                (mix == 0).tobytes(), None if proj is None else proj.tobytes(), None if pipe is None else pipe._content_key())
    cache = eff_H.__dict__.setdefault('_expandplans', {})
    plan = cache.get(move_right)
    if plan is None or plan.handover != handover or plan.dtype != np.dtype(T1.dtype):
        try:
            plan = mps_common.MpoExpandPlan.get(T1, eff_H.W0, move_right, mix == 0, proj, th3 if proj is not None else None, pipe)
        except mps_common.ExpandJobLimit:
            stats['expand_declined'] += 1
            stats['why']['too many jobs'] = stats['why'].get('too many jobs', 0) + 1
            return None
        if getattr(plan, 'handover', None) is None:
            stats['expand_plans_built'] += 1
        plan.handover = handover
        cache[move_right] = plan
    res = plan.apply(T1, mix, th3 if proj is not None else None)
    stats['device_expand'] += 1
    return res, (0 if proj is not None else Id)


def _heff_1site(eff_H, left):
    """``LHeff [(vR*.p0), wR, (vR.p0*)]`` / ``RHeff [(p0*.vL), wL, (p0.vL*)]`` of a one-site operator (the reference's
    ``_get_LHeff`` / ``_get_RHeff``, on site ``i0`` with the labels of ``p0``)."""
    W = eff_H.W0
    if left:
        H = npc.tensordot(eff_H.LP, W, axes=['wR', 'wL'])
        H = H.combine_legs([['vR*', 'p0'], ['vR', 'p0*']], qconj=[+1, -1])
        return H.transpose(['(vR*.p0)', 'wR', '(vR.p0*)'])
    H = npc.tensordot(W, eff_H.RP, axes=['wR', 'wL'])
    H = H.combine_legs([['p0*', 'vL'], ['p0', 'vL*']], qconj=[+1, -1])
    return H.transpose(['(p0*.vL)', 'wL', '(p0.vL*)'])


def generic_expand_1site(eff_H, H, theta, i0, amplitude, move_right, weights=None):
    """The same ``(theta_expand, Id)`` by the reference's statements (:2140-2164, :2170-2194) through ``LHeff`` / ``RHeff``: what
    ``SubspaceExpansion`` issues where ``device_expand_1site`` declines, and the in-process comparison of the tests.  The stacked form
    moving left is written as the mirror image of the one moving right -- the reference's lines name the leg ``wR`` there and leave
    the amplitude out -- and ``explicit_plus_hc`` adds the adjoint part as the reference does."""
    bond = i0 if move_right else i0 - 1
    mix_L, mix_R, IdL, IdR = weights if weights is not None else mix_weights(H, bond, np.sqrt(amplitude))
    plus_hc = bool(getattr(H, 'explicit_plus_hc', False))
    if theta.rank != 2:
        theta = theta.combine_legs(['vL', 'p0'], qconj=+1, new_axes=0) if move_right else theta.combine_legs(['p0', 'vR'], qconj=-1, new_axes=1)
    w, Id = ('wR', IdL) if move_right else ('wL', IdR)
    Heff = _heff_1site(eff_H, move_right)

    def dot(Heff_, th):
        if move_right:
            return npc.tensordot(Heff_, th, axes=['(vR.p0*)', '(vL.p0)']).ireplace_label('(vR*.p0)', '(vL.p0)')
        return npc.tensordot(th, Heff_, axes=['(p0.vR)', '(p0*.vL)']).ireplace_label('(p0.vL*)', '(p0.vR)')
    if not plus_hc and Id is not None:
        expand = dot(Heff.iscale_axis(mix_L if move_right else mix_R, w), theta)
    else:
        wleg = Heff.get_leg(w)
        stack = [theta.add_trivial_leg(1, w, wleg.qconj)]          # theta itself
        proj = np.ones(wleg.ind_len, bool)
        for k in (IdL, IdR):
            if k is not None:
                proj[k] = False
        Heff.iproject(proj, w)
        Heff = Heff * np.sqrt(amplitude)
        stack.append(dot(Heff, theta))
        if plus_hc:         # (Heff^dagger theta) = conj(Heff^T conj(theta))
            if move_right:
                th = npc.tensordot(Heff, theta.conj(), axes=['(vR*.p0)', '(vL*.p0*)'])
                stack.append(th.itranspose(['(vR.p0*)', 'wR', 'vR*']).iconj())
            else:
                th = npc.tensordot(theta.conj(), Heff, axes=['(p0*.vR*)', '(p0.vL*)'])
                stack.append(th.itranspose(['vL*', 'wL', '(p0*.vL)']).iconj())
        expand = npc.concatenate(stack, axis=w)
        Id = 0
    if move_right:
        return expand.combine_legs(['wR', 'vR'], qconj=-1), Id
    return expand.combine_legs(['vL', 'wL'], qconj=+1), Id


class DensityMatrixMixer:
    """The density-matrix mixer of two-site DMRG for the stand-alone driver, with the reference's options and semantics
    (``Mixer`` :1617-1653, ``DensityMatrixMixer`` :1962-2079): ``amplitude`` (1e-5), ``decay`` (2: the amplitude is divided by it after
    every sweep; None: no decay), ``disable_after`` (15 sweeps after activation; None: never)."""

    def __init__(self, options=None, sweep_activated=0):
        options = dict(options or {})
        self.amplitude = options.get('amplitude', 1.e-5)
        self.decay = options.get('decay', 2.)
        self.disable_after = options.get('disable_after', 15)
        assert self.decay is None or self.decay >= 1.
        assert self.disable_after is None or self.disable_after > 0
        assert self.amplitude <= 1.
        self.sweep_activated = sweep_activated

    def update_amplitude(self, sweeps):
        """After a sweep: divide the amplitude by ``decay``; ``None`` when the mixer is to be dropped, else ``self``."""
        disable = self.disable_after is not None and sweeps >= self.sweep_activated + self.disable_after
        if self.amplitude is not None and self.decay is not None:
            self.amplitude /= self.decay
            if self.amplitude <= np.finfo('float').eps:
                disable = True
        return None if disable else self

    def mix_rho(self, engine, theta, i0, mix_left, mix_right):
        eff_H = engine.eff_H
        got = device_mix_rho(eff_H, engine.env.H, theta, i0, self.amplitude, mix_left, mix_right)
        if got is None:
            got = generic_mix_rho(eff_H, engine.env.H, theta, i0, self.amplitude, mix_left, mix_right)
        return got

    def mixed_svd_2site(self, engine, theta, i0, mix_left, mix_right, qtotal_LR=[None, None]):
        rho_L, rho_R = self.mix_rho(engine, theta, i0, mix_left, mix_right)
        return self.svd_from_rho(engine, rho_L, rho_R, theta, qtotal_LR)

    mix_and_decompose_2site = mixed_svd_2site

    @staticmethod
    def _isometry(rho, trunc_params):
        """Eigenvectors of a density matrix to the kept eigenvalues: (vectors [row leg, new leg], kept mask, sqrt of the clipped and
        normalised eigenvalues, truncation error)."""
        val, vec = npc.eigh(rho)
        val[val < 0.] = 0.                    # (stability: reference :2054)
        val /= np.sum(val)
        S_a = np.sqrt(val)
        keep, _, err = truncate(S_a, trunc_params)
        return vec, keep, S_a, err

    def svd_from_rho(self, engine, rho_L, rho_R, theta, qtotal_LR):
        """``theta = U S VH`` with the eigenvectors of ``rho_L`` / ``rho_R`` as isometries and a general bond matrix
        ``S = U^dagger theta VH^dagger`` of norm 1 (reference :2044-2079).  No kernel of its own: two ``eigh``, truncation, projection,
        two tensordots and a norm through ``npc``.  -> ``(U, S, VH, err, S_approx)``."""
        chinfo = theta.chinfo
        qL, qR = (None, None) if qtotal_LR is None else qtotal_LR
        if qL is None and qR is None:
            qL, qR = chinfo.make_valid(), theta.qtotal
        elif qL is None:
            qL = chinfo.make_valid(theta.qtotal - qR)
        elif qR is None:
            qR = chinfo.make_valid(theta.qtotal - qL)
        if not np.all(chinfo.make_valid(np.asarray(qL) + np.asarray(qR)) == theta.qtotal):
            raise ValueError("qtotal_LR must add up to theta.qtotal")
        rho_L.itranspose(['(vL.p0)', '(vL*.p0*)'])
        rho_R.itranspose(['(p1.vR)', '(p1*.vR*)'])
        U, keep_L, S_a, err_L = self._isometry(rho_L, engine.trunc_params)
        U.iset_leg_labels(['(vL.p0)', 'vR'])
        U.iproject(keep_L, axes='vR')
        U = U.gauge_total_charge(1, qL)
        Vc, keep_R, _, err_R = self._isometry(rho_R, engine.trunc_params)
        Vc.iset_leg_labels(['(p1.vR)', 'vL'])
        VH = Vc.itranspose(['vL', '(p1.vR)'])
        VH.iproject(keep_R, axes='vL')
        VH = VH.gauge_total_charge(0, qR)
        S = npc.tensordot(U.conj(), theta, axes=['(vL*.p0*)', '(vL.p0)'])
        S = npc.tensordot(S, VH.conj(), axes=['(p1.vR)', '(p1*.vR*)'])
        S.ireplace_labels(['vR*', 'vL*'], ['vL', 'vR'])
        S /= S.norm()
        assert np.all(S.qtotal == 0)
        return U, S, VH, err_L + err_R, S_a[keep_L]


def decompose_expanded(theta_expand, Id, theta, trunc_params, move_right, svd_theta=svd_theta):
    """``svd_theta`` of the expanded matrix with the total charge of ``theta`` on the side of the site, then the slice ``Id`` of the
    outgoing MPO bond leg of VH (U): ``U S VH`` is the truncated ``theta`` (reference :2164-2169, :2194-2199).  ``svd_theta``: the
    module form passes the reference's own."""
    if move_right:
        U, S, VH, err, _ = svd_theta(theta_expand, trunc_params, qtotal_LR=[theta.qtotal, None], inner_labels=['vR', 'vL'])
        VH = VH.split_legs('(wR.vR)').take_slice(Id, 'wR')
    else:
        U, S, VH, err, _ = svd_theta(theta_expand, trunc_params, qtotal_LR=[None, theta.qtotal], inner_labels=['vR', 'vL'])
        U = U.split_legs('(vL.wL)').take_slice(Id, 'wL')
    return U, S, VH, err


class SubspaceExpansion:
    """The subspace expansion of single-site DMRG for the stand-alone driver, with the reference's options and semantics (``Mixer``
    :1617-1653, ``SubspaceExpansion`` :2082-2201): ``amplitude`` (1e-5), ``decay`` (2), ``disable_after`` (15).  The expanded matrix
    comes from ``device_expand_1site`` -- one GEMM over chi and one ``tpa_mpo_expand_batch`` launch -- or, where that declines, from
    the reference's statements (``generic_expand_1site``); the decomposition is the reference's."""
    can_decompose_1site = True

    def __init__(self, options=None, sweep_activated=0):
        options = dict(options or {})
        self.amplitude = options.get('amplitude', 1.e-5)
        self.decay = options.get('decay', 2.)
        self.disable_after = options.get('disable_after', 15)
        assert self.decay is None or self.decay >= 1.
        assert self.disable_after is None or self.disable_after > 0
        assert self.amplitude <= 1.
        self.sweep_activated = sweep_activated

    update_amplitude = DensityMatrixMixer.update_amplitude

    def expand(self, engine, theta, i0, move_right):
        """``(theta_expand, Id)`` on the device route, else by the reference's statements."""
        eff_H = engine.eff_H
        got = device_expand_1site(eff_H, engine.env.H, theta, i0, self.amplitude, move_right)
        if got is None:
            got = generic_expand_1site(eff_H, engine.env.H, theta, i0, self.amplitude, move_right)
        return got

    def mix_and_decompose_1site(self, engine, theta, i0, move_right):
        """``(U, S, VH, err)`` of the expanded ``theta`` (prepared for the SVD: ``[(vL.p0), vR]`` moving right, ``[vL, (p0.vR)]`` moving
        left), projected back such that ``U S VH`` is the truncated ``theta`` (reference :2164-2169, :2194-2199)."""
        theta_expand, Id = self.expand(engine, theta, i0, move_right)
        return decompose_expanded(theta_expand, Id, theta, engine.trunc_params, move_right)
