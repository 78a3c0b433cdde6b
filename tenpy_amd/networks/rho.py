"""Two-site density matrices and the two-site mutual information of a finite MPS on the device.

The reference's ``MPS.mutinf_two_site`` (networks/mps.py:4180-4233) walks the chain again for every start site i and, per pair (i, j),
issues three ``tensordot`` s on a ``[p0, p0*, vR*, vR]`` tensor, a ``combine_legs``, a block ``eigvalsh`` and one host read.  All rows
that are open at site j see the same ``B_j`` -- the situation ``networks/measure.py`` exploits for correlation functions -- so
``device_two_site_rho`` walks the chain ONCE and carries the open rows as stacks:

* row i carries the slots (a, b), a >= b, of ``C_ab = theta_i[:, b, :]^dagger theta_i[:, a, :]`` (legs ``'vR*', 'vR'``:
  ``measure._start_matrix`` with the matrix unit ``|b><a|``) -- d (d + 1) / 2 slots instead of d^2; the other half of rho follows on the
  host from ``rho[(b, p1'), (a, p1)] = conj rho[(a, p1), (b, p1')]``;
* one stack per charge difference q(a) - q(b): the charge sits in the stack's ``qtotal``, the stack leg ``'s'`` stays charge-neutral,
  and ``measure._push`` serves as it is;
* per site and stack: one ``tensordot`` with ``B_j``, one ``tpa_site_rho_batch`` launch (``SiteRhoPlan``) that closes every row with the
  physical index pair of site j left open into its slice of one device buffer, one ``tensordot`` with ``B_j^*`` while a row stays open;
* a row whose last partner was site j (j - i = max_range) leaves: its slots are zeroed and overwritten by the row that starts next (a
  ring), so a stack holds ``min(max_range, L - 1)`` rows, not L;
* one device-to-host copy ends a walk; the rows are dealt over several walks where the stacks of one would exceed ``measure._budget()``.

``mutinf_two_site`` takes the entropies from host eigenvalues, per charge block of the combined leg (the zero pattern of the result is
exact, so this is the reference's block ``eigvalsh`` on inputs that differ by rounding).

``TPA_MUTINF=0`` switches the stacked route off (``mutinf_generic``: the reference's statement sequence on ``npc``).
"""
import os

import numpy as np

from .._lib import SITE_RHO_MAXD
from ..linalg import _device as dev
from ..linalg import np_conserved as npc
from . import measure
from .measure import _same_leg, _std

__all__ = ['MUTINF', 'rho_stats', 'SiteRhoPlan', 'device_two_site_rho', 'device_one_site_rho', 'mutinf_two_site', 'mutinf_generic',
           'two_site_rho_generic', 'one_site_rho_generic', 'decline_reason', 'entropy', 'clear_caches', 'reset_stats']

# profiles/mutinf.txt (scripts/mutinf_bench.py; L = 100, chi = 2048-shaped chain on the MI355X): the stacked walk takes 0.31 s against
# 11.4 s of the pair-by-pair statements at max_range = 8 and 0.98 s against 36.6 s at 32, far outside the run-to-run spread (2.2 % between
# the stacked runs, 0.6 % between the pair-by-pair ones), so it is on by default
MUTINF = os.environ.get('TPA_MUTINF', '1') != '0'

rho_stats = {}


def reset_stats():
    """Counters of the stacked route: ``walks``, ``kernel_launches`` (``tpa_site_rho_batch``), ``transfer_steps`` (products with
    ``B_j^*``), ``start_tensordots``, ``slots`` / ``slots_full`` (stack slots the started rows took / what d^2 slots per row would have
    been), ``ring_rows`` (the most rows a stack was built for), ``d2h`` (result copies: one per walk) and ``d2h_one_site`` (the one read of
    ``device_one_site_rho``), ``device`` / ``generic`` (calls served by
    either route) and ``why`` (decline reasons)."""
    rho_stats.clear()
    rho_stats.update(walks=0, kernel_launches=0, transfer_steps=0, start_tensordots=0, slots=0, slots_full=0, ring_rows=0, d2h=0, d2h_one_site=0,
                     device=0, generic=0, why={})


reset_stats()


def clear_caches():
    SiteRhoPlan._cache.clear()


def _count_why(reason):
    rho_stats['why'][reason] = rho_stats['why'].get(reason, 0) + 1


class SiteRhoPlan:
    """Job table of one ``tpa_site_rho_batch`` launch: ``out[s, p', p] = sum conj(B[., p', .]) X_s[., p, .]`` for the bra tensor ``B``
    ``['vL', 'p', 'vR']`` and the stack ``X`` (``[row, 's', 'p', 'vR']`` or ``['s', row, 'p', 'vR']``; without a stack leg
    ``[row, 'p', 'vR']``, one slot).  A job is one pair of blocks of B and X with equal row and column sectors; its tile lies at the
    first states of the two physical sectors inside the d x d matrix of a slot.  Cached by the structure keys of B and X and the dtype."""
    _cache = {}
    CACHE_MAX = 4096
    MAX_JOBS = 60000

    @classmethod
    def get(cls, B, X):
        key = (B._struct_key(), X._struct_key(), tuple(X._labels), np.dtype(X.dtype).char)
        plan = cls._cache.get(key)
        if plan is None:
            if len(cls._cache) >= cls.CACHE_MAX:
                cls._cache.clear()
            plan = cls._cache[key] = cls(B, X)
        return plan

    def __init__(self, B, X):
        if list(B._labels) != ['vL', 'p', 'vR']:
            raise ValueError("SiteRhoPlan: the bra tensor needs the legs 'vL', 'p', 'vR' in this order")
        xl = list(X._labels)
        has_stack = 's' in xl
        if xl[-2:] != ['p', 'vR'] or X.rank != (4 if has_stack else 3):
            raise ValueError("SiteRhoPlan: X needs the legs [row, 's', 'p', 'vR'] or ['s', row, 'p', 'vR'], got %r" % (xl,))
        ax_s = xl.index('s') if has_stack else None
        ax_row = [a for a in range(X.rank - 2) if a != ax_s][0]
        ax_p, ax_c = X.rank - 2, X.rank - 1
        if has_stack and X.legs[ax_s].block_number != 1:
            raise ValueError("SiteRhoPlan: the stack leg must be one block")
        if not (_same_leg(X.legs[ax_row], B.legs[0]) and _same_leg(X.legs[ax_p], B.legs[1]) and _same_leg(X.legs[ax_c], B.legs[2])):
            raise ValueError("SiteRhoPlan: the legs of X and of the bra tensor differ")
        self.dtype = np.dtype(X.dtype)
        if np.dtype(B.dtype) != self.dtype:
            raise ValueError("SiteRhoPlan: B and X differ in dtype")
        self.n_stack = X.legs[ax_s].ind_len if has_stack else 1
        p_leg = B.legs[1]
        psl = np.asarray(p_leg.slices, dtype=np.int64)
        self.d = int(p_leg.ind_len)
        self.out_size = self.d * self.d
        self.max_d = int(np.max(p_leg.get_block_sizes()))
        if self.max_d > SITE_RHO_MAXD:
            raise ValueError("SiteRhoPlan: a physical sector is wider than %d" % SITE_RHO_MAXD)
        xs, bs = X._block_shapes(), B._block_shapes()
        b_of = {}
        for n, (qa, qp, qc) in enumerate(B._qdata.tolist()):
            b_of.setdefault((qa, qc), []).append((qp, n))
        jobs = []
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
                jobs.append([int(B._offsets[nb]), d_b * post, d_b, int(X._offsets[nx]), x_ld, x_ss, d_x, pre, post,
                             int(psl[qo]) * self.d + int(psl[qp]), self.d, 0])
        self.n_jobs = len(jobs)
        if self.n_jobs > self.MAX_JOBS:
            raise ValueError("SiteRhoPlan: %d jobs for one launch" % self.n_jobs)
        self.jobs_host = np.array(jobs, dtype=np.int64).reshape(-1, 12)
        self.max_cols = int(np.max(self.jobs_host[:, 7] * self.jobs_host[:, 8])) if jobs else 1
        self.jobs_dev = dev.to_device(self.jobs_host if jobs else np.zeros((1, 12), np.int64))
        j = self.jobs_host
        group = {1: 8, 2: 4}.get(self.max_d, 2)        # stack slots per pass over b (csrc/tpa_site_rho.hip)
        self.bytes = int(self.dtype.itemsize * np.sum(j[:, 7] * j[:, 8] * (self.n_stack * j[:, 6] + -(-self.n_stack // group) * j[:, 2]))) if jobs else 0

    def launch(self, B, X, out_ptr, n_stack=None):
        """Write ``2 n_stack d d`` doubles at ``out_ptr`` (``n_stack`` <= the size of the stack leg)."""
        L = dev.lib()
        n_stack = self.n_stack if n_stack is None else int(n_stack)
        need = int(L.tpa_site_rho_work(self.n_jobs, n_stack, self.out_size, self.max_cols))
        work = dev.scratch('site_rho', need, np.float64)
        b_ptr, x_ptr = (a._arena.data_ptr() if a.stored_blocks else None for a in (B, X))      # (no block: no job reads it)
        dev.check(L.tpa_site_rho_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.max_d, n_stack, self.out_size,
                                       self.max_cols, b_ptr, x_ptr, out_ptr, work.data_ptr(), dev.stream()), "site_rho")
        rho_stats['kernel_launches'] += 1

    def values(self, host, n_stack=None):
        """The complex matrices ``[n_stack, p', p]`` out of the doubles a launch wrote."""
        n_stack = self.n_stack if n_stack is None else int(n_stack)
        v = host[:2 * n_stack * self.out_size].reshape(n_stack, self.d, self.d, 2)
        return v[..., 0] + 1j * v[..., 1]


def decline_reason(psi, plain=None):
    """``None`` when the stacked route serves ``psi``, else the reason the call goes to the generic statements (counted by the callers
    in ``rho_stats['why']``).  ``plain``: the class whose subclasses have methods of their own and are declined as ``'infinite'``."""
    if not MUTINF:
        return 'switched_off'
    if not dev.lib_provides('tpa_site_rho_batch'):
        return 'no_kernel'
    if getattr(psi, 'bc', 'finite') != 'finite' or not getattr(psi, 'finite', True) or (plain is not None and type(psi) is not plain):
        return 'infinite'
    if list(getattr(psi, '_p_label', ['p'])) != ['p'] or set(psi.get_B(0, None).get_leg_labels()) != {'vL', 'p', 'vR'}:
        return 'p_label'
    if max(int(np.max(psi.get_B(i, None).get_leg('p').get_block_sizes())) for i in range(psi.L)) > SITE_RHO_MAXD:
        return 'wide_sector'
    return None


def _flat_charges(leg):
    """The charge of every state of a physical leg as the stack sees it (``qconj`` applied)."""
    return leg.chinfo.make_valid(np.asarray(leg.to_qflat()) * leg.qconj)


def _row_slots(leg):
    """The slots (a, b), a >= b, of a row that starts at a site with the physical leg ``leg``, per charge difference:
    ``{key: [(a, b), ...]}``."""
    q = _flat_charges(leg)
    out = {}
    for a in range(leg.ind_len):
        for b in range(a + 1):
            key = tuple(int(v) for v in leg.chinfo.make_valid(q[b] - q[a]))
            out.setdefault(key, []).append((a, b))
    return out


def _unit(leg, a, b, made):
    """The matrix unit ``|b><a|`` on ``leg`` as a device Array ``['p', 'p*']`` (one upload per leg and slot and call)."""
    key = (id(leg), a, b)
    if key not in made:
        E = np.zeros((leg.ind_len, leg.ind_len))
        E[b, a] = 1.
        made[key] = (leg, npc.Array.from_ndarray(E, [leg, leg.conj()], labels=['p', 'p*']))
    return made[key][1]


def _pairs(L, max_range):
    return [(i, j) for i in range(L) for j in range(i + 1, min(i + max_range + 1, L))]


def device_two_site_rho(psi, max_range=None):
    """``(coords, rhos)``: ``coords`` the int array ``[n, 2]`` of the pairs in the reference's order (``for i in range(L): for j in
    range(i + 1, min(i + max_range + 1, L))``; ``max_range=None``: L), ``rhos[k]`` the reduced density matrix of the pair as a host
    array ``[p0, p1, p0*, p1*]`` (the index order of ``get_rho_segment([i, j])``).  One left-to-right walk with the open rows as
    stacks, or several over parts of the start sites where the stacks of one would not fit ``measure._budget()``."""
    L = psi.L
    max_range = L if max_range is None else int(max_range)
    pairs = _pairs(L, max_range)
    coords = np.array(pairs, dtype=np.int64).reshape(-1, 2)
    if not pairs:
        return coords, []
    legs = [psi.get_B(i, None).get_leg('p') for i in range(L)]
    slots = [_row_slots(leg) for leg in legs]
    width = {}                                   # slots per row of every stack: the most any site asks for
    for sl in slots[:L - 1]:
        for key, lst in sl.items():
            width[key] = max(width.get(key, 0), len(lst))
    starts = list(range(L - 1))
    ring = min(max_range, L - 1)
    fit = max(1, int(measure._budget() // (measure._row_bytes(psi, 0, L - 1) * sum(width.values()))))
    per_walk = len(starts) if fit >= ring else fit
    res = {}
    for at in range(0, len(starts), per_walk):
        _walk(psi, legs, slots, width, starts[at:at + per_walk], max_range, res)
    return coords, [res[p] for p in pairs]


def _walk(psi, legs, slots, width, rows, max_range, res):
    rho_stats['walks'] += 1
    L = psi.L
    lo, hi = rows[0], rows[-1] + 1
    jmax = min(hi - 1 + max_range, L - 1)
    cap = min(max_range, len(rows))              # rows a stack holds at a time
    rho_stats['ring_rows'] = max(rho_stats['ring_rows'], cap)
    keys = sorted(width)
    n_slots = {key: cap * width[key] for key in keys}
    d = [leg.ind_len for leg in legs]
    # the result buffer: per closing site and stack 2 n_slots d_j^2 doubles
    at, total = {}, 0
    for r in range(lo + 1, jmax + 1):
        for key in keys:
            at[(r, key)] = total
            total += 2 * n_slots[key] * d[r] * d[r]
    out = dev.zeros(total, np.float64)
    stacks, plans, made = {}, {}, {}
    for r in range(lo, jmax + 1):
        is_open = [i for i in range(max(lo, r - max_range), min(hi, r))]
        if is_open:
            B = _std(psi.get_B(r, 'B'))
            stay = r < jmax and any(i + max_range > r for i in is_open)
            Bc = B.conj() if stay else None
            for key, stack in list(stacks.items()):
                X = npc.tensordot(stack, B, axes=['vR', 'vL'])          # 'vR*', 's', 'p', 'vR'
                Bk = B if B.dtype == X.dtype else B.astype(X.dtype)
                plan = plans[(r, key)] = SiteRhoPlan.get(Bk, X)
                plan.launch(Bk, X, out.data_ptr() + 8 * at[(r, key)])
                if stay:
                    stacks[key] = npc.tensordot(Bc, X, axes=[['vL*', 'p*'], ['vR*', 'p']])      # 'vR*', 's', 'vR'
                    rho_stats['transfer_steps'] += 1
            if not stay:
                # every open row has left (max_range = 1, or the last site): the stacks still stand on the bond left of site r and
                # must not take the row that starts here -- it begins new ones on the bond right of it
                stacks.clear()
        if lo <= r < hi:
            pos = (r - lo) % cap
            reused = r - lo >= cap
            rho_stats['slots_full'] += d[r] * d[r]
            for key, lst in slots[r].items():
                stack = stacks.get(key)
                if reused and stack is not None:    # the row that sat here has left: its slots are overwritten, not added to
                    keep = np.ones(n_slots[key])
                    keep[pos * width[key]:(pos + 1) * width[key]] = 0.
                    stack = stack.iscale_axis(keep, 's')
                for k, (a, b) in enumerate(lst):
                    C = measure._start_matrix(psi, _unit(legs[r], a, b, made), r)
                    rho_stats['start_tensordots'] += 2
                    rho_stats['slots'] += 1
                    slot = pos * width[key] + k
                    if stack is None:
                        stack = C.add_leg(measure._stack_leg(C.chinfo, n_slots[key]), slot, axis=1, label='s')
                    else:
                        stack = measure._push(stack, C, slot)
                stacks[key] = stack
    host = dev.to_host(out)
    rho_stats['d2h'] += 1
    for (r, key), plan in plans.items():
        vals = plan.values(host[at[(r, key)]:], n_slots[key])          # [slot, p1*, p1]
        for i in range(max(lo, r - max_range), min(hi, r)):
            lst = slots[i].get(key)
            if not lst:
                continue
            rho = res.get((i, r))
            if rho is None:
                rho = res[(i, r)] = np.zeros((d[i], d[r], d[i], d[r]), dtype=np.complex128 if psi.dtype.kind == 'c' else np.float64)
            base = ((i - lo) % cap) * width[key]
            for k, (a, b) in enumerate(lst):
                v = vals[base + k]
                if rho.dtype.kind != 'c':
                    v = v.real
                rho[a, :, b, :] = v.T                   # rho[p0 = a, p1, p0* = b, p1*] = out[p1*, p1]
                if a != b:
                    rho[b, :, a, :] = v.conj()          # rho[(b, p1'), (a, p1)] = conj rho[(a, p1), (b, p1')]


def device_one_site_rho(psi):
    """The one-site density matrices ``[p0, p0*]`` of all sites as host arrays: one ``tpa_site_rho_batch`` launch per site (theta
    against itself, no stack) and one host read for all of them."""
    L = psi.L
    ths = [_std(psi.get_B(i, 'Th')) for i in range(L)]
    d = [th.get_leg('p').ind_len for th in ths]
    at = np.concatenate([[0], np.cumsum([2 * k * k for k in d])])
    out = dev.zeros(int(at[-1]), np.float64)
    plans = []
    for i, th in enumerate(ths):
        plans.append(SiteRhoPlan.get(th, th))
        plans[-1].launch(th, th, out.data_ptr() + 8 * int(at[i]))
    host = dev.to_host(out)
    rho_stats['d2h_one_site'] += 1
    res = []
    for i, plan in enumerate(plans):
        v = plan.values(host[int(at[i]):], 1)[0].T       # out[p', p] = rho[p, p']
        res.append(v if psi.dtype.kind == 'c' else np.ascontiguousarray(v.real))
    return res


def one_site_rho_generic(psi):
    """The statements of the reference's ``get_rho_segment([i])`` (mps.py:4003-4004), one host read per site."""
    res = []
    for i in range(psi.L):
        th = psi.get_B(i, 'Th')
        rho = npc.tensordot(th, th.conj(), axes=(['vL', 'vR'], ['vL*', 'vR*']))
        res.append(np.asarray(rho.itranspose(['p', 'p*']).to_ndarray()))
    return res


def _generic_rows(psi, max_range):
    """The reference's statement sequence (mps.py:4217-4232) up to ``rho_ij``, as a generator of ``(i, j, rho_ij)`` with the legs
    ``'p0', 'p0*', 'p1', 'p1*'`` of ``rho_ij`` in the order the contractions leave them."""
    L = psi.L
    for i in range(L):
        th = psi.get_B(i, 'Th').replace_label('p', 'p0')
        rho = npc.tensordot(th, th.conj(), axes=('vL', 'vL*'))
        jmax = min(i + max_range + 1, L)
        for j in range(i + 1, jmax):
            B = psi.get_B(j, 'B').replace_label('p', 'p1')
            rho = npc.tensordot(rho, B, axes=['vR', 'vL'])
            rho_ij = npc.tensordot(rho, B.conj(), axes=(['vR*', 'vR'], ['vL*', 'vR*']))
            yield i, j, rho_ij
            if j + 1 < jmax:
                rho = npc.tensordot(rho, B.conj(), axes=(['vR*', 'p1'], ['vL*', 'p1*']))


def two_site_rho_generic(psi, max_range=None):
    """``device_two_site_rho`` from the reference's statements, one host read per pair."""
    max_range = psi.L if max_range is None else int(max_range)
    coords, rhos = [], []
    for i, j, rho_ij in _generic_rows(psi, max_range):
        coords.append((i, j))
        rhos.append(np.asarray(rho_ij.itranspose(['p0', 'p1', 'p0*', 'p1*']).to_ndarray()))
    return np.array(coords, dtype=np.int64).reshape(-1, 2), rhos


def entropy(p, n=1):
    """The reference's ``tools.math.entropy``: values ``<= 1e-30`` are dropped; von Neumann for n = 1, ``-log max p`` for n = inf, Renyi
    otherwise."""
    p = np.asarray(p)
    p = p[p > 1.e-30]
    if n == 1:
        return -np.inner(np.log(p), p)
    if n == np.inf:
        return -np.log(np.max(p))
    return np.log(np.sum(p**n)) / (1. - n)


def mutinf_generic(psi, max_range=None, n=1):
    """``(coords, mutinf)`` from the reference's statement sequence on ``npc`` (mps.py:4206-4233): per pair three ``tensordot`` s, a
    ``combine_legs``, a block ``eigvalsh`` and its host read.  The route of declined calls; it uses no entry point of the stacked
    route."""
    max_range = psi.L if max_range is None else int(max_range)
    S_i = []
    for i in range(psi.L):
        th = psi.get_B(i, 'Th')
        rho = npc.tensordot(th, th.conj(), axes=(['vL', 'vR'], ['vL*', 'vR*']))
        S_i.append(entropy(npc.eigvalsh(rho.itranspose(['p', 'p*'])), n))
    coords, mi = [], []
    for i, j, rho_ij in _generic_rows(psi, max_range):
        rho_ij = rho_ij.combine_legs([['p0', 'p1'], ['p0*', 'p1*']], qconj=[+1, -1])
        coords.append((i, j))
        mi.append(S_i[i] + S_i[j] - entropy(npc.eigvalsh(rho_ij), n))
    return np.array(coords, dtype=np.int64).reshape(-1, 2), np.array(mi)


def _block_eigenvalues(mat, charges):
    """Eigenvalues of the Hermitian host matrix ``mat`` whose entries between states of different ``charges`` (one row per state) are
    exact zeros: ``numpy.linalg.eigvalsh`` per charge block (the lower triangle, as the reference reads it)."""
    if charges.shape[1] == 0:
        return np.linalg.eigvalsh(mat)
    _, inverse = np.unique(charges, axis=0, return_inverse=True)
    inverse = np.asarray(inverse).reshape(-1)
    return np.concatenate([np.linalg.eigvalsh(mat[np.ix_(idx, idx)]) for idx in (np.nonzero(inverse == g)[0] for g in range(inverse.max() + 1))])


def entropies(psi, coords, rhos, rho1, n=1):
    """``S_i + S_j - S_ij`` for the pairs ``coords`` from the host matrices ``rhos`` / ``rho1``."""
    chinfo = psi.get_B(0, None).chinfo
    q = [_flat_charges(psi.get_B(i, None).get_leg('p')) for i in range(psi.L)]
    S_i = [entropy(_block_eigenvalues(r, q[i]), n) for i, r in enumerate(rho1)]
    mi = []
    for (i, j), rho in zip(coords.tolist(), rhos):
        di, dj = rho.shape[0], rho.shape[1]
        qij = chinfo.make_valid((q[i][:, None, :] + q[j][None, :, :]).reshape(di * dj, -1))
        mi.append(S_i[i] + S_i[j] - entropy(_block_eigenvalues(rho.reshape(di * dj, di * dj), qij), n))
    return np.array(mi)


def mutinf_two_site(psi, max_range=None, n=1, why=False, generic=None):
    """``(coords, mutinf)`` with ``mutinf[k] = S_i + S_j - S_ij`` for ``i, j = coords[k]`` (reference ``MPS.mutinf_two_site``): from the
    stacked walk and host eigenvalues, or -- with the reason ``why`` (default: ``decline_reason``; counted in ``rho_stats``) -- from
    ``generic()`` (default: ``mutinf_generic``)."""
    if why is False:
        why = decline_reason(psi)
    if why is not None:
        rho_stats['generic'] += 1
        _count_why(why)
        return mutinf_generic(psi, max_range, n) if generic is None else generic()
    rho_stats['device'] += 1
    rho1 = device_one_site_rho(psi)
    coords, rhos = device_two_site_rho(psi, max_range)
    return coords, entropies(psi, coords, rhos, rho1, n)
