"""Measurement on the device: one-site expectation values and two-point correlation functions of a finite MPS.

The reference's ``MPS.correlation_function`` (networks/mps.py:680-887) takes its rows from ``_corr_up_diag`` (:1289-1323): for every
start site i it walks the chain again -- ``C . B_r``, ``op2 . C``, ``inner``, ``B_r^dagger . C`` -- with one host read per (i, j).
All rows see the same ``B_r`` at site r, so ``device_corr_up`` walks the chain ONCE and carries the started rows as a stack: ``Cstack``
has the legs ``'vR*', 's', 'vR'`` with a charge-neutral stack leg ``'s'``, one ``npc.tensordot`` pair advances every row, one
``tpa_site_inner_batch`` launch (``SiteInnerPlan``) closes every row against ``B_r^dagger op2`` into a row of a device matrix, and one
device-to-host copy ends the walk.

``TPA_MEASURE=0`` switches the stacked route off (the callers then run the row-by-row statements, ``corr_up_generic``).  The default
follows ``profiles/measure.txt`` (``scripts/measure_bench.py``).
"""
import os
from hashlib import blake2b

import numpy as np

from .._lib import MPO_APPLY_MAXD
from ..linalg import _device as dev
from ..linalg import np_conserved as npc
from ..linalg.charges import LegCharge

__all__ = ['MEASURE', 'measure_stats', 'SiteInnerPlan', 'device_corr_up', 'corr_up', 'corr_up_generic', 'device_expectation_value', 'expectation_values', 'decline_reason',
           'as_site_op', 'clear_caches', 'reset_stats']

# profiles/measure.txt (L = 100, chi = 2048-shaped chain on the MI355X): the stacked walk takes a third of the time of the row-by-row
# statements, far outside the run-to-run spread, so it is on by default
MEASURE = os.environ.get('TPA_MEASURE', '1') != '0'

measure_stats = {}


def reset_stats():
    """Counters of the stacked route: ``walks``, ``kernel_launches`` (``tpa_site_inner_batch``), ``transfer_steps`` and
    ``transfer_tensordots``, ``start_tensordots``, ``opstr_tensordots``, ``closing_tensordots`` (the X of the last site), ``d2h`` (result copies), ``op_reads`` (operators given as
    device Arrays, read once per call each), ``slot_copies`` / ``slot_adds`` (rows that joined the stack by a copy into their slot / by an
    addition over the whole stack), ``filled`` / ``capacity`` (stack slots summed over the products with B_r: the flops spent on empty
    slots are ``1 - filled / capacity`` of the transfer flops), ``device`` / ``generic`` (calls served by either route) and ``why``
    (decline reasons)."""
    measure_stats.clear()
    measure_stats.update(walks=0, kernel_launches=0, transfer_steps=0, transfer_tensordots=0, start_tensordots=0, opstr_tensordots=0, closing_tensordots=0,
                         d2h=0, op_reads=0, slot_copies=0, slot_adds=0, filled=0, capacity=0, device=0, generic=0, why={})


reset_stats()


def clear_caches():
    SiteInnerPlan._cache.clear()


def _count_why(reason):
    measure_stats['why'][reason] = measure_stats['why'].get(reason, 0) + 1


def _budget():
    """Bytes the stacks of one walk may take: the free-memory helper of the batched TEBD work areas and the warm-start cache."""
    return dev.memory_budget('TPA_MEASURE_STACK_GB', 1. / 6., 8.)


def as_site_op(op, leg, hosts=None):
    """A one-site operator as a device Array ``['p', 'p*']`` on ``leg``.  Dense host matrices are uploaded with their charge detected
    and entered in ``hosts`` (see ``_host``), so that they are never read back; device Arrays are returned as they are."""
    if isinstance(op, npc.Array):
        return op
    host = np.asarray(op)
    res = npc.Array.from_ndarray(host, [leg, leg.conj()], labels=['p', 'p*'])
    if hosts is not None:
        hosts[id(res)] = (res, host)
    return res


def _host(op, hosts):
    """The dense host copy ``[p, p*]`` of the operator ``op`` (what ``SiteInnerPlan`` makes its coefficient blocks from).  ``hosts`` is
    the table of ONE call, ``id(op) -> (op, copy)``: an operator is read from the device once per call and never across calls -- nothing
    is kept on the Array, whose copies and in-place writers (``2 * op``, ``op.conj()``, ``iscale_prefactor`` ...) would carry a stale
    matrix along."""
    ent = hosts.get(id(op))
    if ent is None:
        ent = hosts[id(op)] = (op, np.asarray(op.copy(deep=False).itranspose(['p', 'p*']).to_ndarray()))
        measure_stats['op_reads'] += 1
    return ent[1]


def _same_leg(a, b):
    return a.qconj == b.qconj and np.array_equal(a.slices, b.slices) and np.array_equal(a.charges, b.charges)


class SiteInnerPlan:
    """Job table of one ``tpa_site_inner_batch`` launch: ``out[s, k] = <B| ops[k] |X_s>`` for the bra tensor ``B`` ``['vL', 'p', 'vR']``,
    the stack ``X`` (``[row, 's', 'p', 'vR']`` or ``['s', row, 'p', 'vR']``; without a stack leg ``[row, 'p', 'vR']``, one slot) and dense
    host operators ``[p, p*]`` (charged or complex ones included).  A job is one pair of blocks of B and X with equal row and column
    sectors, ``coeff`` the (p', p) sector block of the operator (blocks that are exactly zero are left out), ``out_col`` the operator.
    Cached by the structure keys of B and X and the operators' bytes."""
    _cache = {}
    CACHE_MAX = 4096

    @classmethod
    def get(cls, B, X, ops_host):
        h = blake2b(digest_size=16)
        for o in ops_host:
            o = np.ascontiguousarray(o)
            h.update(o.dtype.str.encode())
            h.update(o.tobytes())
        key = (B._struct_key(), X._struct_key(), tuple(X._labels), np.dtype(X.dtype).char, len(ops_host), h.digest())
        plan = cls._cache.get(key)
        if plan is None:
            if len(cls._cache) >= cls.CACHE_MAX:
                cls._cache.clear()
            plan = cls._cache[key] = cls(B, X, ops_host)
        return plan

    def __init__(self, B, X, ops_host):
        if list(B._labels) != ['vL', 'p', 'vR']:
            raise ValueError("SiteInnerPlan: the bra tensor needs the legs 'vL', 'p', 'vR' in this order")
        xl = list(X._labels)
        has_stack = 's' in xl
        if xl[-2:] != ['p', 'vR'] or X.rank != (4 if has_stack else 3):
            raise ValueError("SiteInnerPlan: X needs the legs [row, 's', 'p', 'vR'] or ['s', row, 'p', 'vR'], got %r" % (xl,))
        ax_s = xl.index('s') if has_stack else None
        ax_row = [a for a in range(X.rank - 2) if a != ax_s][0]
        ax_p, ax_c = X.rank - 2, X.rank - 1
        if has_stack and X.legs[ax_s].block_number != 1:
            raise ValueError("SiteInnerPlan: the stack leg must be one block")
        if not (_same_leg(X.legs[ax_row], B.legs[0]) and _same_leg(X.legs[ax_p], B.legs[1]) and _same_leg(X.legs[ax_c], B.legs[2])):
            raise ValueError("SiteInnerPlan: the legs of X and of the bra tensor differ")
        self.dtype = np.dtype(X.dtype)
        if np.dtype(B.dtype) != self.dtype:
            raise ValueError("SiteInnerPlan: B and X differ in dtype")
        self.n_stack = X.legs[ax_s].ind_len if has_stack else 1
        # a complex operator on real tensors takes two output columns (its real and its imaginary part): ``cols[k]`` = (re, im or None)
        split, self.cols = [], []
        for op in ops_host:
            op = np.asarray(op)
            if self.dtype.kind != 'c' and np.iscomplexobj(op):
                im = np.any(op.imag != 0)
                self.cols.append((len(split), len(split) + 1 if im else None))
                split += [op.real, op.imag] if im else [op.real]
            else:
                self.cols.append((len(split), None))
                split.append(op)
        ops_host = split
        self.n_out = len(ops_host)
        p_leg = B.legs[1]
        psl = np.asarray(p_leg.slices, dtype=np.int64)
        self.max_d = int(np.max(p_leg.get_block_sizes()))
        if self.max_d > MPO_APPLY_MAXD:
            raise ValueError("SiteInnerPlan: a physical sector is wider than %d" % MPO_APPLY_MAXD)
        xs, bs = X._block_shapes(), B._block_shapes()
        b_of = {}
        for n, (qa, qp, qc) in enumerate(B._qdata.tolist()):
            b_of.setdefault((qa, qc), []).append((qp, n))
        jobs, coeff, c_len = [], [], 0
        blocks = {}         # (operator, p' sector, p sector) -> offset of the coefficient block
        for nx, q in enumerate(X._qdata.tolist()):
            qa, qp, qc = q[ax_row], q[ax_p], q[ax_c]
            pre, d_x, post = int(xs[nx, ax_row]), int(xs[nx, ax_p]), int(xs[nx, ax_c])
            if not has_stack:
                x_ld, x_ss = d_x * post, 0
            elif ax_s == 1:
                x_ss = d_x * post
                x_ld = self.n_stack * x_ss
            else:
                x_ld = d_x * post
                x_ss = pre * x_ld
            for qo, nb in b_of.get((qa, qc), ()):
                d_b = int(bs[nb, 1])
                for k, op in enumerate(ops_host):
                    c_off = blocks.get((k, qo, qp))
                    if c_off is None:
                        blk = np.asarray(op)[psl[qo]:psl[qo + 1], psl[qp]:psl[qp + 1]]
                        if np.any(blk != 0):
                            c_off = c_len
                            coeff.append(np.ascontiguousarray(blk, dtype=self.dtype).reshape(-1))
                            c_len += blk.size
                        else:
                            c_off = -1
                        blocks[(k, qo, qp)] = c_off
                    if c_off >= 0:
                        jobs.append([int(B._offsets[nb]), d_b * post, d_b, int(X._offsets[nx]), x_ld, x_ss, d_x, pre, post, c_off, k, 0])
        self.jobs_host = np.array(jobs, dtype=np.int64).reshape(-1, 12)
        self.coeff_host = np.concatenate(coeff) if coeff else np.zeros(1, dtype=self.dtype)
        self.n_jobs = len(jobs)
        if self.n_jobs > 60000:
            raise ValueError("SiteInnerPlan: %d jobs for one launch" % self.n_jobs)
        self.max_cols = int(np.max(self.jobs_host[:, 7] * self.jobs_host[:, 8])) if jobs else 1
        self.jobs_dev, self.coeff_dev = dev.to_device_packed(self.jobs_host if jobs else np.zeros((1, 12), np.int64), self.coeff_host)
        j = self.jobs_host
        isz = self.dtype.itemsize
        self.bytes = int(isz * np.sum(j[:, 7] * j[:, 8] * (self.n_stack * j[:, 6] + -(-self.n_stack // 8) * j[:, 2]))) if jobs else 0

    def launch(self, B, X, out_ptr, n_stack=None):
        """Write ``2 n_stack n_out`` doubles at ``out_ptr`` (``n_stack`` <= the size of the stack leg: the filled slots)."""
        L = dev.lib()
        n_stack = self.n_stack if n_stack is None else int(n_stack)
        need = int(L.tpa_site_inner_work(self.n_jobs, n_stack, self.n_out, self.max_cols))
        work = dev.scratch('site_inner', need, np.float64)
        dev.check(L.tpa_site_inner_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.coeff_dev.data_ptr(), self.max_d,
                                         n_stack, self.n_out, self.max_cols, B._arena.data_ptr(), X._arena.data_ptr(), out_ptr,
                                         work.data_ptr(), dev.stream()), "site_inner")
        measure_stats['kernel_launches'] += 1

    def values(self, host):
        """The complex values ``[n_stack, operators]`` out of the doubles ``host[0 : 2 n_stack n_out]`` a launch wrote."""
        n_stack = len(host) // (2 * self.n_out)
        v = host[:2 * n_stack * self.n_out].reshape(n_stack, self.n_out, 2)
        v = v[:, :, 0] + 1j * v[:, :, 1]
        return np.stack([v[:, a] if b is None else v[:, a] + 1j * v[:, b] for a, b in self.cols], axis=1)


def _capacity(filled):
    """Stack slots for ``filled`` started rows: at most a fifth of them empty."""
    return filled + filled // 4


def _stack_leg(chinfo, n):
    return LegCharge.from_trivial(n, chinfo, 1)


def _regrow(stack, leg):
    """The stack with the longer stack leg ``leg``: the old slots in front, zeros behind (one strided copy launch)."""
    ax = stack.get_leg_index('s')
    legs = list(stack.legs)
    legs[ax] = leg
    res = npc.Array(legs, stack.dtype, stack.qtotal, list(stack._labels))
    if stack.stored_blocks == 0:
        return res
    sizes = stack._block_sizes_flat()
    shapes = stack._block_shapes()
    res._set_blocks(stack._qdata.copy(), zero=True, qdata_sorted=stack._qdata_sorted)
    outer = np.prod(shapes[:, :ax], axis=1)
    inner = np.prod(shapes[:, ax + 1:], axis=1)
    old, new = shapes[:, ax], leg.ind_len
    M = npc.COPY_MAXDIM
    jobs = np.zeros((len(sizes), 4 + 3 * M), dtype=np.int64)
    jobs[:, 0], jobs[:, 1], jobs[:, 2] = res._offsets, stack._offsets, 3
    jobs[:, 4], jobs[:, 5], jobs[:, 6] = outer, old, inner
    jobs[:, 4 + M], jobs[:, 5 + M], jobs[:, 6 + M] = new * inner, inner, 1
    jobs[:, 4 + 2 * M], jobs[:, 5 + 2 * M], jobs[:, 6 + 2 * M] = old * inner, inner, 1
    npc._run_copy(stack.dtype, jobs, int(np.max(sizes)), stack._arena, res._arena)
    return res


def _slot_jobs(stack, C, slot):
    """Copy jobs that write the blocks of ``C`` (``'vR*', 'vR'``) into slot ``slot`` of the blocks of ``stack`` (``'vR*', 's', 'vR'``), or
    ``None`` when the stack lacks one of these blocks."""
    where = {(qa, qc): n for n, (qa, _, qc) in enumerate(stack._qdata.tolist())}
    idx = [where.get((qa, qc)) for qa, qc in C._qdata.tolist()]
    if any(n is None for n in idx):
        return None
    idx = np.array(idx, dtype=np.int64)
    shapes = C._block_shapes()
    cap = stack.get_leg('s').ind_len
    M = npc.COPY_MAXDIM
    jobs = np.zeros((len(idx), 4 + 3 * M), dtype=np.int64)
    jobs[:, 0], jobs[:, 1], jobs[:, 2] = stack._offsets[idx] + slot * shapes[:, 1], C._offsets, 2
    jobs[:, 4], jobs[:, 5] = shapes[:, 0], shapes[:, 1]
    jobs[:, 4 + M], jobs[:, 5 + M] = cap * shapes[:, 1], 1
    jobs[:, 4 + 2 * M], jobs[:, 5 + 2 * M] = shapes[:, 1], 1
    return jobs


def _push(stack, C, filled):
    """The stack with the start matrix ``C`` (``'vR*', 'vR'``) in slot ``filled``: one strided copy of C's blocks into the (empty, zero)
    slot.  Only where the stack has no block for one of them is C embedded in an Array of the stack's size and added."""
    if stack is None:
        return C.add_leg(_stack_leg(C.chinfo, _capacity(1)), 0, axis=1, label='s')
    leg = stack.get_leg('s')
    if filled >= leg.ind_len:
        leg = _stack_leg(C.chinfo, _capacity(filled + 1))
        stack = _regrow(stack, leg)
    if list(stack._labels) == ['vR*', 's', 'vR'] and list(C._labels) == ['vR*', 'vR'] and stack.dtype == C.dtype and C.stored_blocks:
        jobs = _slot_jobs(stack, C, filled)
        if jobs is not None:
            stack._own_arena()
            npc._run_copy(stack.dtype, jobs, int(np.max(C._block_sizes_flat())), C._arena, stack._arena)
            measure_stats['slot_copies'] += 1
            return stack
    measure_stats['slot_adds'] += 1
    return stack.iadd_prefactor_other(1., C.add_leg(leg, filled, axis=1, label='s'))


def _start_op(ops1, opstr, i, str_on_first, apply_opstr_first):
    op1 = ops1[i % len(ops1)]
    opstr1 = opstr[i % len(opstr)] if opstr is not None else None
    if opstr1 is not None and str_on_first:
        op1 = npc.tensordot(op1, opstr1, axes=['p*', 'p'] if apply_opstr_first else ['p', 'p*'])
    return op1


def _start_matrix(psi, op1, i, bra=None):
    """``theta_i^dagger op1 theta_i`` with the legs ``'vR*', 'vR'`` (reference mps.py:1297-1302)."""
    theta = psi.get_B(i, 'Th')
    C = npc.tensordot(op1, theta, axes=['p*', 'p'])
    theta_bra = theta if bra is None else bra.get_B(i, 'Th')
    return npc.tensordot(theta_bra.conj(), C, axes=[['vL*', 'p*'], ['vL', 'p']])


def corr_up_generic(psi, ops1, ops2, i, j_gtr, opstr, str_on_first, apply_opstr_first, bra=None):
    """The row-by-row statements (reference ``_corr_up_diag``, mps.py:1289-1323): the values for fixed ``i`` and every j of ``j_gtr``
    (ascending, all > i), one host read each."""
    C = _start_matrix(psi, _start_op(ops1, opstr, i, str_on_first, apply_opstr_first), i, bra)
    js = list(j_gtr[::-1])
    res = []
    for r in range(i + 1, js[0] + 1):
        B = psi.get_B(r, 'B')
        B_bra = B if bra is None else bra.get_B(r, 'B')
        C = npc.tensordot(C, B, axes=['vR', 'vL'])
        if r == js[-1]:
            Cij = npc.tensordot(ops2[r % len(ops2)], C, axes=['p*', 'p'])
            Cij.ireplace_labels(['vR*'], ['vL'])
            res.append(npc.inner(B_bra, Cij, axes='labels', do_conj=True))
            js.pop()
        if len(js) > 0:
            op = opstr[r % len(opstr)] if opstr is not None else None
            if op is not None:
                C = npc.tensordot(op, C, axes=['p*', 'p'])
            C = npc.tensordot(B_bra.conj(), C, axes=[['vL*', 'p*'], ['vR*', 'p']])
    return res


def corr_up(psi, ops1, ops2, sites1, sites2, opstr, str_on_first, apply_opstr_first, bra=None, why=False, hosts=None):
    """The values above the diagonal (``sites2[y] > sites1[x]``; zeros elsewhere) as a complex matrix ``[len(sites1), len(sites2)]``:
    from the stacked walk, or -- with the reason ``why`` (default: ``decline_reason``; counted in ``measure_stats``) -- row by row."""
    if why is False:
        why = decline_reason(psi, ops1, ops2, opstr, bra)
    if why is None:
        measure_stats['device'] += 1
        return device_corr_up(psi, ops1, ops2, sites1, sites2, opstr, str_on_first, apply_opstr_first, hosts)
    measure_stats['generic'] += 1
    _count_why(why)
    s2 = np.asarray(sites2, dtype=np.int64)
    out = np.zeros((len(sites1), len(s2)), dtype=np.complex128)
    for x, i in enumerate(sites1):
        gtr = s2 > i
        if np.any(gtr):
            out[x, gtr] = corr_up_generic(psi, ops1, ops2, int(i), [int(j) for j in s2[gtr]], opstr, str_on_first, apply_opstr_first, bra)
    return out


def decline_reason(psi, ops1, ops2, opstr=None, bra=None):
    """``None`` when the stacked route serves the call, else the reason it goes to the generic statements (counted by the callers in
    ``measure_stats['why']``).  The operators are device Arrays ``['p', 'p*']``."""
    if not MEASURE:
        return 'switched_off'
    if not dev.lib_provides('tpa_site_inner_batch'):
        return 'no_kernel'
    if getattr(psi, 'bc', 'finite') != 'finite' or not getattr(psi, 'finite', True):
        return 'infinite'
    if bra is not None and bra is not psi:
        return 'bra_ne_ket'
    if list(getattr(psi, '_p_label', ['p'])) != ['p'] or set(psi.get_B(0, None).get_leg_labels()) != {'vL', 'p', 'vR'}:
        return 'p_label'
    for ops in (ops1, ops2):
        if any(o.rank != 2 or set(o.get_leg_labels()) != {'p', 'p*'} for o in ops):
            return 'p_label'
        if any(np.any(o.qtotal != ops[0].qtotal) for o in ops[1:]):
            return 'op_charges'
    if opstr is not None and any(o is not None and np.any(o.qtotal != 0) for o in opstr):
        return 'op_charges'
    if max(int(np.max(psi.get_B(i, None).get_leg('p').get_block_sizes())) for i in range(psi.L)) > MPO_APPLY_MAXD:
        return 'wide_sector'
    return None


def _std(B):
    return B if list(B._labels) == ['vL', 'p', 'vR'] else B.transpose(['vL', 'p', 'vR'])


def _row_bytes(psi, lo, hi):
    """Upper estimate of the stack memory per started row between the sites ``lo`` and ``hi``: the stack before and after a transfer
    step and X between them (dense bond dimensions), twice -- a regrown stack lives beside the old one for a moment, and the
    allocator keeps the blocks of the previous site."""
    isz = 16 if np.dtype(psi.dtype).kind == 'c' else 8
    worst = 1
    for r in range(lo, hi + 1):
        B = psi.get_B(r, None)
        vl, d, vr = (B.get_leg(l).ind_len for l in ('vL', 'p', 'vR'))
        worst = max(worst, vl * vl + vl * d * vr + vr * vr)
    return 2 * isz * worst


def device_corr_up(psi, ops1, ops2, sites1, sites2, opstr, str_on_first, apply_opstr_first, hosts=None):
    """All values ``<psi| op1_i (opstr_{i..j-1}) op2_j |psi>`` with j > i of ``_corr_up_diag`` for i in ``sites1`` and j in ``sites2``
    (both ascending) as a complex host matrix ``[len(sites1), len(sites2)]`` (zeros where j <= i): one walk from min(sites1) to
    max(sites2) that carries the started rows as a stack -- or several walks over parts of ``sites1`` where the stacks of one would not
    fit the memory budget.  ``ops1`` / ``ops2`` / ``opstr`` are lists of device Arrays ``['p', 'p*']`` (from ``as_site_op``), indexed
    with the site modulo their length; entries of ``opstr`` (or all of it) may be ``None``.  ``hosts``: the host copies of operators
    that came as dense matrices (``as_site_op``); the others are read once in this call."""
    hosts = {} if hosts is None else hosts
    sites1, sites2 = [int(i) for i in sites1], [int(j) for j in sites2]
    res = np.zeros((len(sites1), len(sites2)), dtype=np.complex128)
    if not sites2:
        return res
    jmax = max(sites2)
    rows = sorted(((x, i) for x, i in enumerate(sites1) if i < jmax), key=lambda xi: xi[1])
    if not rows:
        return res
    per_walk = max(1, int(_budget() // _row_bytes(psi, rows[0][1], jmax)))
    for at in range(0, len(rows), per_walk):
        _walk(psi, ops1, ops2, rows[at:at + per_walk], sites2, opstr, str_on_first, apply_opstr_first, res, hosts)
    return res


def _walk(psi, ops1, ops2, rows, sites2, opstr, str_on_first, apply_opstr_first, res, hosts):
    measure_stats['walks'] += 1
    i0, jmax = rows[0][1], max(sites2)
    start = {i: x for x, i in rows}
    closing = [(y, j) for y, j in enumerate(sites2) if j > i0]
    close_at = {j: k for k, (_, j) in enumerate(closing)}
    n_rows = len(rows)
    out = dev.zeros(4 * len(closing) * n_rows, np.float64)       # row k: the values of closing site k for the slots 0 .. filled - 1
    stack, filled, slot_x, closed = None, 0, [], {}
    for r in range(i0, jmax + 1):
        if stack is not None:
            B = _std(psi.get_B(r, 'B'))
            X = npc.tensordot(stack, B, axes=['vR', 'vL'])          # 'vR*', 's', 'p', 'vR'
            measure_stats['filled'] += filled
            measure_stats['capacity'] += stack.get_leg('s').ind_len
            if r in close_at:
                Bk = B if B.dtype == X.dtype else B.astype(X.dtype)
                plan = SiteInnerPlan.get(Bk, X, [_host(ops2[r % len(ops2)], hosts)])
                plan.launch(Bk, X, out.data_ptr() + 32 * close_at[r] * n_rows, n_stack=filled)
                closed[close_at[r]] = (plan, filled)
            if r < jmax:
                op = opstr[r % len(opstr)] if opstr is not None else None
                if op is not None:
                    X = npc.tensordot(op, X, axes=['p*', 'p'])
                    measure_stats['opstr_tensordots'] += 1
                stack = npc.tensordot(B.conj(), X, axes=[['vL*', 'p*'], ['vR*', 'p']])      # 'vR*', 's', 'vR'
                measure_stats['transfer_steps'] += 1
                measure_stats['transfer_tensordots'] += 2
            else:
                measure_stats['closing_tensordots'] += 1        # (the last site only closes)
        if r in start and r < jmax:
            C = _start_matrix(psi, _start_op(ops1, opstr, r, str_on_first, apply_opstr_first), r)
            measure_stats['start_tensordots'] += 2
            stack = _push(stack, C, filled)
            slot_x.append(start[r])
            filled += 1
    host = dev.to_host(out).reshape(len(closing), 4 * n_rows)
    measure_stats['d2h'] += 1
    for k, (y, j) in enumerate(closing):
        plan, n = closed[k]
        vals = plan.values(host[k, :2 * n * plan.n_out])[:, 0]
        for s in range(n):
            res[slot_x[s], y] = vals[s]


def device_expectation_value(psi, ops, sites, hosts=None):
    """``<psi| op_k |psi>`` at every site of ``sites`` for every operator of ``ops`` (device Arrays from ``as_site_op``, or a list of
    them per site: ``ops[k][i % len]``) as a complex host matrix ``[len(sites), len(ops)]``: one ``tpa_site_inner_batch`` launch per
    site for all operators (theta against itself, no stack) and one device-to-host copy for the whole call."""
    hosts = {} if hosts is None else hosts
    sites = [int(i) for i in sites]
    K = len(ops)
    out = dev.zeros(4 * max(len(sites), 1) * K, np.float64)
    plans = []
    for n, i in enumerate(sites):
        th = _std(psi.get_B(i, 'Th'))
        here = [(o[i % len(o)] if isinstance(o, (list, tuple)) else o) for o in ops]
        plans.append(SiteInnerPlan.get(th, th, [_host(o, hosts) for o in here]))
        plans[-1].launch(th, th, out.data_ptr() + 32 * n * K)
    host = dev.to_host(out).reshape(-1, 4 * K)
    measure_stats['d2h'] += 1
    res = np.zeros((len(sites), K), dtype=np.complex128)
    for n, plan in enumerate(plans):
        res[n] = plan.values(host[n, :2 * plan.n_out])[0]
    return res


def expectation_values(psi, ops, sites, hosts=None, why=False):
    """``device_expectation_value`` where the route serves the call, else -- with a counted reason -- the generic statements (one
    ``tensordot`` and one ``inner`` with its host read per site and operator).  ``ops[k]`` is one device Array per site."""
    if why is False:
        why = None
        for o in ops:
            why = why or decline_reason(psi, o, o)
    if why is None:
        measure_stats['device'] += 1
        return device_expectation_value(psi, ops, sites, hosts)
    measure_stats['generic'] += 1
    _count_why(why)
    res = np.zeros((len(sites), len(ops)), dtype=np.complex128)
    for n, i in enumerate(sites):
        th = psi.get_B(int(i), 'Th')
        for k, o in enumerate(ops):
            res[n, k] = npc.inner(th, npc.tensordot(o[int(i) % len(o)], th, axes=['p*', 'p']), axes='labels', do_conj=True)
    return res
