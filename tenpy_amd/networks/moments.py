"""MPO expectation value and energy variance on the device: ``<psi| H |psi>`` and ``<psi| H^2 |psi>`` of a finite chain from ONE
left-to-right walk.

The reference's ``MPO.variance`` (networks/mpo.py:1296-1342) contracts ``contr[vR*, wR1, wR2, vR]`` site by site with four
``npc.tensordot`` calls, two of them over an MPO bond leg of 1-wide blocks (thousands of K = 1 GEMM tasks and transposed copies of the
largest tensors of the whole project, ``D^2 d`` bond matrices); ``expectation_value_finite`` (:1144-1171) does the same for one layer
through ``MPOEnvironment``.  Here the single-layer rows ``[vR*, wR, vR]`` and the pair rows ``[vR*, wR1, wR2, vR]`` advance together,
and per site each of them takes

1. one grouped GEMM ``contr . B`` (no transposed copy: asserted),
2. the MPO step as one launch of the plan family of the MPO (``mps_common._mpo_plan_class``; two layers: ``MpoPairPlan``), which
   puts the physical leg next to ``vR*``,
3. one grouped GEMM with ``B^*``, conjugated by the link flag of the GEMM (no conjugated copy of B).

Site 0 is ``get_theta(0, n=1)`` against a boundary tensor that is 1 at ``IdL`` (the ``take_slice(IdL)`` of the reference as a one-entry
row, so that the first site runs the statements of every other one), the last site ends at ``IdR`` with the trace over the one-dimensional outer
bond, and one device-to-host copy of both numbers ends the call.  ``psi.norm`` is ignored, as in the reference.

A call that the walk does not take runs the reference's statements, counted with its reason in ``moments_stats['why']``: ``infinite``
(also segment chains), ``p_label``, ``switched_off``, ``plus_hc``, ``init_env`` (given environment data), ``memory``, ``plan`` (no plan
class for the MPO) and ``wide_mpo`` -- an MPO bond so wide that the pair step would exceed the job table of a launch or that building
its plans on the first call would cost more than the statements (``MpoPairPlan.MAX_JOBS``, ``MAX_MATCH``: D above about 8 for a spin
chain; measured in ``profiles/mpo_moments.txt``).

``TPA_MPO_MOMENTS=0`` switches the route off; ``TPA_MPO_MOMENTS_PAIR`` = ``auto`` (default: the mode with fewer terms) / ``product`` /
``two_pass`` fixes the mode of the pair step (measurement knob).  The defaults follow ``profiles/mpo_moments.txt``
(``scripts/moments_bench.py``).
"""
import os

import numpy as np

from ..algorithms import mps_common as mc
from ..linalg import _device as dev
from ..linalg import np_conserved as npc
from . import measure

__all__ = ['moments_stats', 'reset_stats', 'enabled', 'decline_reason', 'device_mpo_moments', 'expectation_value', 'variance',
           'expectation_value_generic', 'variance_generic']

MOMENTS_DEFAULT = '1'       # profiles/mpo_moments.txt

moments_stats = {}


def reset_stats():
    """Counters: ``walks``; ``gemms`` (grouped GEMM launches of the walks); ``steps_1`` / ``steps_2`` (MPO steps of the single-layer and
    of the pair rows, one per site) and ``step_launches`` (their kernel launches: a ``two_pass`` pair step takes two); ``modes`` (pair
    steps by mode); ``d2h`` (result copies); ``device`` / ``reference`` (calls served by either route) and ``why`` (decline reasons)."""
    moments_stats.clear()
    moments_stats.update(walks=0, gemms=0, steps_1=0, steps_2=0, step_launches=0, modes={'product': 0, 'two_pass': 0}, d2h=0, device=0,
                         reference=0, why={})


reset_stats()


def enabled():
    return os.environ.get('TPA_MPO_MOMENTS', MOMENTS_DEFAULT) != '0'


def _pair_mode():
    return {'product': False, 'two_pass': True}.get(os.environ.get('TPA_MPO_MOMENTS_PAIR', 'auto'))


def _count_why(reason):
    moments_stats['reference'] += 1
    moments_stats['why'][reason] = moments_stats['why'].get(reason, 0) + 1


def _Id(H, i, left):
    """Index of the "only identities to the left / right" state on the bond left / right of site i, ``None`` if the MPO has none."""
    if hasattr(H, 'get_IdL'):           # the reference's MPO; the stand-alone class has its own two readers
        Id = H.get_IdL(i) if left else H.get_IdR(i)
    else:
        Id = H._zipup_IdL(i) if left else H._zipup_IdR(i)
    return None if Id is None else int(Id) % H.get_W(i).get_leg('wL' if left else 'wR').ind_len


def _walk_bytes(psi, H, order):
    """Upper estimate (dense bond dimensions) of what the widest site of the walk holds at once: ``contr``, ``T1 = contr . B`` and
    ``T3``, the result of the MPO step, of every row set."""
    isz = 16 if np.result_type(psi.dtype, H.dtype).kind == 'c' else 8
    worst = 0
    for i in range(psi.L):
        B, W = psi.get_B(i, None), H.get_W(i)
        vl, d, vr = (B.get_leg(l).ind_len for l in ('vL', 'p', 'vR'))
        Dl, Dr = W.get_leg('wL').ind_len, W.get_leg('wR').ind_len
        rows = sum(vl * vl * Dl**k + vl * d * vr * (Dl**k + Dr**k) for k in range(1, order + 1))
        worst = max(worst, rows)
    return isz * worst


def decline_reason(psi, H, order, init_env_data=None):
    """``None`` when the walk serves ``<H>`` (``order`` 1) or ``<H>`` and ``<H^2>`` (2) of ``psi``, else the reason the call runs the
    reference's statements (counted by the callers in ``moments_stats['why']``)."""
    if getattr(psi, 'bc', 'finite') != 'finite' or getattr(H, 'bc', 'finite') != 'finite':
        return 'infinite'
    if list(getattr(psi, '_p_label', ['p'])) != ['p'] or set(psi.get_B(0, None).get_leg_labels()) != {'vL', 'p', 'vR'}:
        return 'p_label'
    if not enabled():
        return 'switched_off'
    if getattr(H, 'explicit_plus_hc', False):
        return 'plus_hc'
    if init_env_data:
        return 'init_env'
    if psi.L != H.L or psi.get_B(0, None).get_leg('vL').ind_len != 1 or psi.get_B(psi.L - 1, None).get_leg('vR').ind_len != 1:
        return 'infinite'       # (an open outer bond is a segment, whatever the chain calls itself)
    if _walk_bytes(psi, H, order) > measure._budget():
        return 'memory'
    if _Id(H, 0, True) is None or _Id(H, H.L - 1, False) is None:
        return 'plan'
    for i in range(H.L):
        W = H.get_W(i)
        if set(W.get_leg_labels()) != {'wL', 'wR', 'p', 'p*'} or W.stored_blocks == 0 or mc._mpo_plan_class(W) is None:
            return 'plan'
        # blocks of X and Y at this site: at most one per row sector, MPO bond block(s) and physical sector (the column sector
        # follows from the charges); one job each, and the job tables of the MPO-step plans take 60000
        rows = psi.get_B(i, None).get_leg('vL').block_number * W.get_leg('p').block_number
        width = max(W.get_leg('wL').block_number, W.get_leg('wR').block_number)
        if rows * width**order > mc.MpoPairPlan.MAX_JOBS:
            return 'wide_mpo'
        if order == 2:
            if len(mc.MpoPairPlan.modes_within_reach(W, rows * width**2, _pair_mode())) < (2 if _pair_mode() is None else 1):
                return 'wide_mpo'
            if mc.MpoPairPlan.family(W) is None:
                return 'plan'
    return None


def _std(B):
    return B if list(B._labels) == ['vL', 'p', 'vR'] else B.transpose(['vL', 'p', 'vR'])


def _conj_view(B):
    """``B.conj()`` without its data: conjugated legs, labels and total charge on the arena of B (the GEMM conjugates on its way)."""
    Bc = B.copy(deep=False)
    Bc.legs = [leg.conj() for leg in B.legs]
    Bc._labels = [npc.Array._conj_leg_label(l) for l in B._labels]
    Bc.qtotal = B.chinfo.make_valid(-B.qtotal)
    return Bc


def _boundary(leg_ket, leg_w, Id, n_w, dtype):
    """The row set before site 0: ``[vR*, wR, vR]`` (``n_w`` = 1) or ``[vR*, wR1, wR2, vR]`` (2), the unit matrix of the outer bond at
    ``Id`` of every MPO leg."""
    chi = leg_ket.ind_len
    dense = np.zeros((chi,) + (leg_w.ind_len,) * n_w + (chi,), dtype=dtype)
    dense[(np.arange(chi),) + (Id,) * n_w + (np.arange(chi),)] = 1.
    labels = ['vR*'] + (['wR'] if n_w == 1 else ['wR1', 'wR2']) + ['vR']
    return npc.Array.from_ndarray(dense, [leg_ket] + [leg_w] * n_w + [leg_ket.conj()], dtype=dtype, labels=labels)


def _step_plan(X, W, n_w):
    if n_w == 1:
        return mc._mpo_plan_class(W).get(X, W, 'wR', 'p', 'wL', 'wR', 'p', 'p*', ('vR*', 'p', 'wR', 'vR'))
    return mc.MpoPairPlan.get(X, W, _pair_mode())


def _advance(contr, B, Bc, W, n_w):
    """One site of one row set; ``None`` when nothing is left of it (the moment is then zero)."""
    p1, c_use, b_use = npc.plan_tensordot(contr, B, axes=['vR', 'vL'])
    assert c_use is contr and b_use is B, "moments step 1 must not need a transpose"
    if p1.empty:
        return None
    X = p1.apply(contr, B)                                      # vR*, wR [wR1, wR2], p, vR
    plan = _step_plan(X, W, n_w)
    if plan.empty:
        return None
    Y = plan.apply(X)                                           # vR*, p, wR [wR1, wR2], vR
    launches = 1 if n_w == 1 else plan.launches
    moments_stats['steps_%d' % n_w] += 1
    moments_stats['step_launches'] += launches
    if n_w == 2:
        moments_stats['modes'][plan.mode] += 1
    p2, b_use, y_use = npc.plan_tensordot(Bc, Y, axes=[['vL*', 'p*'], ['vR*', 'p']])
    assert b_use is Bc and y_use is Y, "moments step 3 must not need a transpose"
    moments_stats['gemms'] += 2
    if p2.empty:
        return None
    return _apply_conj_a(p2, Bc, Y)                             # vR*, wR [wR1, wR2], vR


def _conj_a_links(plan):
    """The link tables of a contraction plan (its own, its split-K part's) with flag bit 0 set -- the GEMM conjugates A on its way
    (include/tenpy_amd.h, ``tpa_gemm_chain``) --, uploaded once and kept on the plan."""
    t = plan.__dict__.get('_tpa_conj_a')
    if t is None:
        def flagged(links):
            links = links.copy()
            links[:, 7] |= 1
            return dev.to_device(links)
        t = plan._tpa_conj_a = (flagged(plan.links_host), None if plan.sk is None else flagged(plan.sk.links_host))
    return t


def _apply_conj_a(plan, a, b):
    """``plan.apply(a, b)`` where ``a`` stands for its complex conjugate: the caller has conjugated its legs (``_conj_view``), the GEMM
    conjugates the data, so that no conjugated copy is made.  The launches of ``TensordotPlan.apply`` with the flagged links; real
    data needs no flag and goes through ``apply`` itself."""
    if plan.dtype.kind != 'c':
        return plan.apply(a, b)
    res = plan.apply(a, b, launch=False)
    links, sk_links = _conj_a_links(plan)
    L, code, sk = dev.lib(), dev.code(plan.dtype), plan.sk
    a_arena = (a if a.dtype == plan.dtype else a.astype(plan.dtype))._arena
    b_arena = (b if b.dtype == plan.dtype else b.astype(plan.dtype))._arena
    if sk is None:
        dev.check(L.tpa_gemm_chain(code, plan.cfg, plan.tasks_dev.data_ptr(), links.data_ptr(), plan.tiles_dev.data_ptr(), plan.n_tiles,
                                   a_arena.data_ptr(), b_arena.data_ptr(), res._arena.data_ptr(), dev.stream()), "gemm_chain")
    else:       # split-K: partial blocks into a scratch arena, then the plan's reduction pass
        part = dev.scratch('gemm_split_k', sk.total, plan.dtype)
        dev.check(L.tpa_gemm_chain(code, plan.cfg, sk.tasks_dev.data_ptr(), sk_links.data_ptr(), sk.tiles_dev.data_ptr(), sk.n_tiles,
                                   a_arena.data_ptr(), b_arena.data_ptr(), part.data_ptr(), dev.stream()), "gemm_chain")
        dev.check(L.tpa_lincomb_batch(code, sk.jobs_dev.data_ptr(), sk.n_jobs, sk.terms_dev.data_ptr(), sk.max_elems, part.data_ptr(),
                                      res._arena.data_ptr(), dev.stream()), "lincomb_batch")
    return res


def _close(contr, Id, out, k):
    """The value of a row set behind the last site -- ``take_slice(IdR)`` and the trace over the one-dimensional outer bond: one
    element of the arena -- into ``out[k]`` on the device."""
    if contr is None:
        return
    where = [leg.get_qindex(i) for leg, i in zip(contr.legs, [0] + [Id] * (contr.rank - 2) + [0])]
    row = np.nonzero(np.all(contr._qdata == np.array([b for b, _ in where]), axis=1))[0]
    if len(row) == 0:
        return
    pos = 0
    for (_, at), size in zip(where, contr._block_shapes()[row[0]]):
        pos = pos * int(size) + int(at)
    off = int(contr._offsets[row[0]]) + pos
    out[k:k + 1].copy_(contr._arena[off:off + 1])


def device_mpo_moments(psi, H, order, first=True):
    """``(<psi|H|psi>, <psi|H^2|psi>)`` (``order`` 1: ``(<psi|H|psi>, None)``) of a finite chain from one walk, as complex host
    numbers; the caller has asked ``decline_reason``.  ``first=False`` leaves the single-layer rows out (``variance`` with a given
    ``exp_val``): ``(None, <psi|H^2|psi>)``."""
    assert order in (1, 2) and (first or order == 2)
    moments_stats['walks'] += 1
    dtype = np.dtype(np.result_type(psi.dtype, H.dtype))
    n_ws = ([1] if first else []) + ([2] if order == 2 else [])
    th0 = psi.get_theta(0, n=1).replace_label('p0', 'p')
    leg_w = H.get_W(0).get_leg('wL').conj()
    rows = {n_w: _boundary(th0.get_leg('vL'), leg_w, _Id(H, 0, True), n_w, dtype) for n_w in n_ws}
    for i in range(psi.L):
        B = _std(th0 if i == 0 else psi.get_B(i, form='B'))
        if B.dtype != dtype:
            B = B.astype(dtype)
        Bc, W = _conj_view(B), H.get_W(i)
        for n_w in n_ws:
            if rows[n_w] is not None:
                rows[n_w] = _advance(rows[n_w], B, Bc, W, n_w)
    out = dev.zeros(2, dtype)
    IdR = _Id(H, H.L - 1, False)
    for n_w in n_ws:
        _close(rows[n_w], IdR, out, n_w - 1)
    host = np.asarray(dev.to_host(out)).astype(np.complex128)
    moments_stats['d2h'] += 1
    return (host[0] if first else None), (host[1] if order == 2 else None)


# ---- the reference's statements, for the stand-alone classes (under ``install`` a decline runs the reference's own method) -------------

def expectation_value_generic(psi, H):
    """``MPOEnvironment(psi, H).full_contraction(0)`` (reference mpo.py:1169-1171; handles ``explicit_plus_hc``)."""
    from .mpo import MPOEnvironment
    return np.real_if_close(MPOEnvironment(psi, H).full_contraction(0))


def variance_generic(psi, H, exp_val):
    """The statements of the reference's ``MPO.variance`` (mpo.py:1328-1342)."""
    th = psi.get_theta(0, n=1)
    W = H.get_W(0).take_slice(_Id(H, 0, True), 'wL')
    contr = npc.tensordot(th, W.replace_label('wR', 'wR1'), axes=['p0', 'p*'])
    contr = npc.tensordot(contr, W.replace_label('wR', 'wR2'), axes=['p', 'p*'])
    contr = npc.tensordot(th.conj(), contr, axes=[['vL*', 'p0*'], ['vL', 'p']])
    for i in range(1, H.L):
        B = psi.get_B(i, form='B')
        W = H.get_W(i)
        contr = npc.tensordot(contr, B, axes=['vR', 'vL'])
        contr = npc.tensordot(contr, W.replace_label('wR', 'wR1'), axes=[['wR1', 'p'], ['wL', 'p*']])
        contr = npc.tensordot(contr, W.replace_label('wR', 'wR2'), axes=[['wR2', 'p'], ['wL', 'p*']])
        contr = npc.tensordot(contr, B.conj(), axes=[['vR*', 'p'], ['vL*', 'p*']])
    contr = contr.take_slice([_Id(H, H.L - 1, False)] * 2, ['wR1', 'wR2'])
    contr = npc.trace(contr, 'vR', 'vR*')
    return np.real_if_close(contr - exp_val**2)


# ---- the two calls, for the stand-alone ``MPO`` and the wrappers of ``module_form`` ------------------------------------------------------

def expectation_value(psi, H, generic, init_env_data=None):
    """``(<psi|H|psi>, why)``: from the walk (``why`` is ``None``), or -- with the counted reason ``why`` -- from ``generic()``."""
    why = decline_reason(psi, H, 1, init_env_data)
    if why is not None:
        _count_why(why)
        return generic(), why
    moments_stats['device'] += 1
    return np.real_if_close(device_mpo_moments(psi, H, 1)[0]), None


def variance(psi, H, exp_val, generic):
    """``(<psi|H^2|psi> - exp_val^2, why)`` (``exp_val=None``: ``<psi|H|psi>`` from the same walk): from the walk (``why`` is ``None``),
    or -- with the counted reason ``why`` -- from ``generic()``.  The caller has made the reference's argument checks."""
    why = decline_reason(psi, H, 2)
    if why is not None:
        _count_why(why)
        return generic(), why
    moments_stats['device'] += 1
    h1, h2 = device_mpo_moments(psi, H, 2, first=exp_val is None)
    if exp_val is None:
        exp_val = np.real_if_close(h1)
    return np.real_if_close(h2 - exp_val**2), None
