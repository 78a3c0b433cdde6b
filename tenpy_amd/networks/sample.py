"""Projective sampling of a finite MPS on the device, a whole batch of samples per walk.

The reference's ``MPS.sample_measurements`` (networks/mps.py:4349-4442) draws ONE string per call: per site a ``tensordot`` of a single
vector with ``B``, ``tensordot(theta.conj(), theta)``, a host read of the diagonal, ``rng.choice``, ``take_slice``, ``norm`` (a host
read) and a division.  All samples see the same ``B_i`` at site i, so ``device_sample`` carries n samples as a block-diagonal stack
``V`` (``['s', 'vR']``, qtotal 0: the stack leg ``'s'`` has one sector per occupied sector of the bond, block q of shape n_q x chi_q).
One site is three device steps -- ``X = tensordot(V, B_i)`` (one grouped GEMM), ``tpa_sample_select_batch`` (``SamplePlan``: Born
probabilities and the outcome of every row) and ``tpa_sample_gather_batch`` (the chosen, normalised slices written into the next
stack, the rows re-sorted by their new sector) -- and one device-to-host copy of n x 32 bytes.

The uniform numbers come from the caller's numpy generator (``rng.random((n, n_sites))``, filled in the order of n consecutive
reference calls), which is what makes the route reproducible against the reference: ``Generator.choice(dim, p=p)`` draws one
``random()`` and takes ``cdf.searchsorted(u, side='right')``.

``TPA_SAMPLE=0`` switches the route off (every call then runs the sample-by-sample statements, ``sample_generic``);
``TPA_SAMPLE_SINGLE=0`` does so for single-sample calls (``n_samples=None``) only.  The defaults follow ``profiles/sample.txt``
(``scripts/sample_bench.py``).
"""
import os

import numpy as np

from .._lib import SAMPLE_MAX_DIM
from ..linalg import _device as dev
from ..linalg import np_conserved as npc
from ..linalg.charges import LegCharge
from .measure import _std, as_site_op

__all__ = ['SAMPLE', 'SINGLE', 'sample_stats', 'SamplePlan', 'device_sample', 'sample_generic', 'sample_measurements', 'decline_reason',
           'clear_caches', 'reset_stats']

# profiles/sample.txt (100 sites of a chi = 2048-shaped chain on the MI355X): a batch of 64 takes 19 ms against 1.9 s sample by sample, so
# the route is on by default; a walk with ONE sample takes 17 ms against 31 - 33 ms for the statements, outside the run-to-run spread
# (below 5 %), so a single-sample call (n_samples=None) takes it by default as well
SAMPLE = os.environ.get('TPA_SAMPLE', '1') != '0'
SINGLE = os.environ.get('TPA_SAMPLE_SINGLE', '1') != '0'

sample_stats = {}


def reset_stats():
    """Counters of the batched route: ``walks``, ``select_launches`` / ``gather_launches`` (the two entry points), ``tensordots`` (the
    products ``V . B_i`` and the rotations of site tensors into the eigenbasis of an operator), ``d2h`` (device-to-host copies),
    ``uploads`` (tables and uniforms, one per launch pair), ``device`` / ``generic`` (calls served by either route) and ``why``
    (decline reasons)."""
    sample_stats.clear()
    sample_stats.update(walks=0, select_launches=0, gather_launches=0, tensordots=0, d2h=0, uploads=0, device=0, generic=0, why={})


reset_stats()


def clear_caches():
    SamplePlan._cache.clear()


def _count_why(reason):
    sample_stats['why'][reason] = sample_stats['why'].get(reason, 0) + 1


def _budget():
    """Bytes the stacks of one walk may take (the free-memory helper of ``measure._budget``)."""
    return dev.memory_budget('TPA_SAMPLE_STACK_GB', 1. / 6., 8.)


class SamplePlan:
    """Seg and group tables of one ``tpa_sample_select_batch`` launch for the structure of ``X`` (``['s', 'p', 'vR']``): a seg is one
    charge block (rows, d, post) of X, a group the segs of one sector of the stack leg, ascending in ``sigma0``.  Cached by
    ``X._struct_key()``.  Host side: ``seg_of[g, sigma]`` is the seg that covers the outcome ``sigma`` for the rows of group g (-1:
    none) and ``seg_q[seg]`` the sector of the 'vR' leg the rows land in."""
    _cache = {}
    CACHE_MAX = 4096

    @classmethod
    def get(cls, X):
        key = (X._struct_key(), np.dtype(X.dtype).char)
        plan = cls._cache.get(key)
        if plan is None:
            if len(cls._cache) >= cls.CACHE_MAX:
                cls._cache.clear()
            plan = cls._cache[key] = cls(X)
        return plan

    def __init__(self, X):
        if list(X._labels) != ['s', 'p', 'vR']:
            raise ValueError("SamplePlan: X needs the legs 's', 'p', 'vR' in this order, got %r" % (list(X._labels),))
        s_leg, p_leg = X.legs[0], X.legs[1]
        self.dtype = np.dtype(X.dtype)
        self.dim = int(p_leg.ind_len)
        if not 1 <= self.dim <= SAMPLE_MAX_DIM:
            raise ValueError("SamplePlan: site dimension %d outside [1, %d]" % (self.dim, SAMPLE_MAX_DIM))
        self.n_rows = int(s_leg.ind_len)
        shapes = X._block_shapes()
        psl = np.asarray(p_leg.slices, dtype=np.int64)
        ssl = np.asarray(s_leg.slices, dtype=np.int64)
        qd = np.asarray(X._qdata, dtype=np.int64).reshape(-1, 3)
        order = np.lexsort((psl[qd[:, 1]], qd[:, 0])) if len(qd) else np.zeros(0, dtype=np.int64)       # by stack sector, then sigma0
        segs = np.zeros((max(len(qd), 1), 8), dtype=np.int64)
        self.seg_q = np.zeros(max(len(qd), 1), dtype=np.int64)
        n_groups = s_leg.block_number
        groups = np.zeros((max(n_groups, 1), 4), dtype=np.int64)
        groups[:n_groups, 2] = ssl[:-1]
        groups[:n_groups, 3] = ssl[1:] - ssl[:-1]
        self.seg_of = np.full((max(n_groups, 1), self.dim), -1, dtype=np.int64)
        for k, n in enumerate(order.tolist()):
            g, qp, qv = qd[n].tolist()
            d, post = int(shapes[n, 1]), int(shapes[n, 2])
            segs[k, :5] = (int(X._offsets[n]), d * post, d, post, psl[qp])
            self.seg_q[k] = qv
            if groups[g, 1] == 0:
                groups[g, 0] = k
            groups[g, 1] += 1
            self.seg_of[g, psl[qp]:psl[qp] + d] = k
        self.n_segs, self.n_groups = len(qd), n_groups
        self.segs_host, self.groups_host = segs, groups
        self.row_group = np.repeat(np.arange(n_groups, dtype=np.int64), groups[:n_groups, 3])      # row -> group
        self.bytes = int(self.dtype.itemsize * np.sum(shapes[:, 0] * shapes[:, 1] * shapes[:, 2])) if len(qd) else 0
        self.segs_dev, self.groups_dev = dev.to_device_packed(segs, groups)

    def launch(self, X, u_dev, out):
        """Write the rows ``{sigma, w, total, 0}`` of all ``n_rows`` rows of X to the device doubles ``out``."""
        dev.check(dev.lib().tpa_sample_select_batch(dev.code(self.dtype), self.segs_dev.data_ptr(), self.n_segs, self.groups_dev.data_ptr(),
                                                    self.n_groups, self.dim, self.n_rows, X._arena.data_ptr(), u_dev.data_ptr(),
                                                    out.data_ptr(), dev.stream()), "sample_select")
        sample_stats['select_launches'] += 1


def _is_plain_finite(psi):
    if getattr(psi, 'bc', 'finite') != 'finite' or not getattr(psi, 'finite', True):
        return False
    from .mps import MPS
    if type(psi) is MPS:
        return True
    # the reference's classes on the mirror: MPS itself, no subclass (UniformMPS reaches the wrapper through super(); PurificationMPS
    # overrides the method)
    return type(psi).__name__ == 'MPS' and type(psi).__module__.endswith('networks.mps')


def decline_reason(psi, first_site=0, last_site=None, n_samples=None):
    """``None`` when the batched route serves the call, else the reason it goes to the sample-by-sample statements (counted by the
    callers in ``sample_stats['why']``)."""
    if not SAMPLE:
        return 'switched_off'
    if n_samples is None and not SINGLE:
        return 'single_sample'
    if not _is_plain_finite(psi):
        return 'not_plain_finite'
    if tuple(getattr(psi, '_p_label', ('p',))) != ('p',):
        return 'p_label'
    last_site = psi.L - 1 if last_site is None else last_site
    if not 0 <= first_site <= last_site < psi.L:
        return 'site_range'
    if psi.get_B(first_site, None).get_leg('vL').ind_len != 1:
        return 'first_site'
    if max(psi.get_B(i, None).get_leg('p').ind_len for i in range(first_site, last_site + 1)) > SAMPLE_MAX_DIM:
        return 'site_dim'
    if not (dev.lib_provides('tpa_sample_select_batch') and dev.lib_provides('tpa_sample_gather_batch')):
        return 'no_kernel'
    return None


def _measure_op(psi, op, i):
    """The one-site operator ``op`` of site ``i`` as a device Array ``['p', 'p*']``: a name of the site class (the reference's MPS),
    a dense host matrix or a device Array (the stand-alone MPS)."""
    if isinstance(op, str):
        return psi.sites[i].get_op(op).transpose(['p', 'p*'])
    if isinstance(op, npc.Array):
        return op.transpose(['p', 'p*'])
    return as_site_op(op, psi.get_B(i, None).get_leg('p'))


def _eig_basis(psi, ops, i, first_site, cache):
    """``(W, V)`` of the operator measured at site ``i`` (reference mps.py:4408-4412), once per distinct operator and leg."""
    op = ops[(i - first_site) % len(ops)]
    leg = psi.get_B(i, None).get_leg('p')
    key = (op if isinstance(op, str) else id(op), id(leg))
    if key not in cache:
        O = _measure_op(psi, op, i)
        if npc.norm(O - O.conj().transpose()) > 1.e-13:
            raise ValueError('measurement operator %r not hermitian' % (op if isinstance(op, str) else (i - first_site) % len(ops),))
        W, V = npc.eigh(O)
        cache[key] = (np.asarray(W), V, op)          # (``op`` is kept so that its id is not given to another object during the call)
    return cache[key][:2]


def _rotated(B, V):
    """The site tensor in the eigenbasis of the measured operator: ``tensordot(V.conj(), B)`` (reference mps.py:4413), as
    ``'vL', 'p', 'vR'``."""
    sample_stats['tensordots'] += 1
    return npc.tensordot(V.conj(), B, axes=['p*', 'p']).replace_label('eig*', 'p').transpose(['vL', 'p', 'vR'])


def _stack_leg(vleg, sectors, counts):
    """The stack leg for rows in the sectors ``sectors`` (ascending block indices of ``vleg``, the 'vR' leg of the stack), ``counts``
    rows each: qconj +1 and the charges that make the blocks (k, sectors[k]) the ones of a tensor with qtotal 0."""
    chinfo = vleg.chinfo
    charges = chinfo.make_valid(-vleg.qconj * np.asarray(vleg.charges)[sectors].reshape(len(sectors), chinfo.qnumber))
    slices = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return LegCharge.from_qind(chinfo, slices, charges, qconj=1)


def _new_stack(vleg, sectors, counts, dtype):
    V = npc.Array([_stack_leg(vleg, sectors, counts), vleg], dtype, labels=['s', 'vR'])
    V._set_blocks(np.stack([np.arange(len(sectors)), sectors], axis=1), qdata_sorted=True)
    return V


def _sample_bytes(psi, first_site, last_site):
    """Upper estimate of the stack memory per sample: V before and after a site and X between them (dense bond dimensions), twice --
    the allocator keeps the blocks of the previous site."""
    worst = 1
    for i in range(first_site, last_site + 1):
        B = psi.get_B(i, None)
        vl, d, vr = (B.get_leg(l).ind_len for l in ('vL', 'p', 'vR'))
        worst = max(worst, vl + d * vr + vr)
    return 2 * 16 * worst + 64


def device_sample(psi, n_samples, last_site, u, ops=None, norm_tol=1.e-12, first_site=0):
    """``n_samples`` projective samples of the sites ``first_site .. last_site`` (``first_site`` with a 'vL' leg of width 1) from the
    uniforms ``u[sample, site]``: ``(sigma, W, w, phase)`` -- the outcomes as indices ``[n, n_sites]``, the eigenvalues per site (or
    ``None`` without ``ops``), the norms of the chosen slices ``[n, n_sites]`` and, for a whole chain, the remaining 1 x 1 entry
    ``theta_00 / w`` of every sample (else ``None``).  One walk, or several over parts of the batch where the
    stacks of one would not fit the memory budget."""
    n_sites = last_site - first_site + 1
    u = np.asarray(u, dtype=np.float64).reshape(n_samples, n_sites)
    sigma = np.zeros((n_samples, n_sites), dtype=np.int64)
    w = np.zeros((n_samples, n_sites), dtype=np.float64)
    closes = first_site == 0 and last_site == psi.L - 1 and psi.get_B(last_site, None).get_leg('vR').ind_len == 1
    phase = np.zeros(n_samples, dtype=np.complex128) if closes else None
    eig, Ws = {}, None
    if ops is not None:
        Ws = [_eig_basis(psi, ops, i, first_site, eig)[0] for i in range(first_site, last_site + 1)]
    per_walk = max(1, int(_budget() // _sample_bytes(psi, first_site, last_site)))
    for at in range(0, n_samples, per_walk):
        sl = slice(at, min(at + per_walk, n_samples))
        kind = _walk(psi, first_site, last_site, u[sl], ops, eig, norm_tol, sigma[sl], w[sl], None if phase is None else phase[sl])
    if phase is not None and kind != 'c':
        phase = phase.real
    return sigma, Ws, w, phase


def _gather(X, rows_dev, n_rows, out, Vn):
    """The chosen slices of ``X``, divided by the norms in ``out``, into the arena of the next stack ``Vn``."""
    dev.check(dev.lib().tpa_sample_gather_batch(dev.code(X.dtype), rows_dev.data_ptr(), n_rows, X._arena.data_ptr(), out.data_ptr(),
                                                Vn._arena.data_ptr(), dev.stream()), "sample_gather")
    sample_stats['gather_launches'] += 1


def _walk(psi, first_site, last_site, u, ops, eig, norm_tol, sigma, w, phase):
    sample_stats['walks'] += 1
    n = len(u)
    B = _std(psi.get_B(first_site, 'Th'))
    vleg = B.get_leg('vL').conj()
    V = npc.Array.from_ndarray(np.ones((n, 1), dtype=np.float64), [_stack_leg(vleg, np.zeros(1, dtype=np.int64), [n]), vleg], labels=['s', 'vR'])
    slot = np.arange(n)                 # sample number of every row of the stack
    u_dev = dev.to_device(np.ascontiguousarray(u[:, 0]))
    sample_stats['uploads'] += 1
    out = dev.empty(4 * n, np.float64)
    for k, i in enumerate(range(first_site, last_site + 1)):
        if k > 0:
            B = _std(psi.get_B(i, 'B'))
        if ops is not None:
            B = _rotated(B, _eig_basis(psi, ops, i, first_site, eig)[1])
        X = npc.tensordot(V, B, axes=['vR', 'vL'])          # 's', 'p', 'vR'
        sample_stats['tensordots'] += 1
        if X.stored_blocks == 0:
            raise ValueError('not normalized to `norm_tol`')
        plan = SamplePlan.get(X)
        plan.launch(X, u_dev, out)
        host = dev.to_host(out).reshape(n, 4)
        sample_stats['d2h'] += 1
        if np.any(host[:, 0] < 0) or not np.all(np.abs(host[:, 2] - 1.) <= norm_tol):
            raise ValueError('not normalized to `norm_tol`')
        sig = host[:, 0].astype(np.int64)
        sigma[slot, k], w[slot, k] = sig, host[:, 1]
        last = i == last_site
        if last and phase is None:
            break
        # the rows of the next stack: sorted stably by their new sector, then by sample number
        seg = plan.seg_of[plan.row_group, sig]
        newq = plan.seg_q[seg]
        order = np.lexsort((slot, newq))
        sectors, counts = np.unique(newq, return_counts=True)
        Vn = _new_stack(X.get_leg('vR'), sectors, counts, X.dtype)
        S = plan.segs_host[seg[order]]
        local = np.arange(n)[order] - plan.groups_host[plan.row_group[order], 2]
        post = S[:, 3]
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        which = np.searchsorted(sectors, newq[order])
        rows = np.zeros((n, 4), dtype=np.int64)
        rows[:, 0] = S[:, 0] + local * S[:, 1] + (sig[order] - S[:, 4]) * post
        rows[:, 1] = post
        rows[:, 2] = Vn._offsets[which] + (np.arange(n) - starts[which]) * post
        rows[:, 3] = np.arange(n)[order]
        slot = slot[order]
        if last:
            rows_dev, = dev.to_device_packed(rows)
        else:
            rows_dev, u_dev = dev.to_device_packed(rows, np.ascontiguousarray(u[slot, k + 1]))
        sample_stats['uploads'] += 1
        _gather(X, rows_dev, n, out, Vn)
        V = Vn
    if phase is not None:       # the 1 x 1 rows that are left carry the phase (reference mps.py:4435-4438)
        phase[slot] = dev.to_host(V._arena).reshape(-1)[:n]
        sample_stats['d2h'] += 1
    return np.dtype(V.dtype).kind


def sample_generic(psi, first_site=0, last_site=None, ops=None, rng=None, norm_tol=1.e-12, complex_amplitude=True, u=None,
                   margins=None):
    """ONE sample with the reference's statements (networks/mps.py:4394-4442) on the Arrays of ``psi``: the declined route and the
    comparator.  With ``u`` (one uniform number per site) ``rng.choice`` is replaced by what it computes from its one ``random()``,
    ``cdf.searchsorted(u, side='right')``; ``margins`` (a list) then receives the distance of every u from the nearest cdf edge."""
    if tuple(getattr(psi, '_p_label', ('p',))) != ('p',):
        raise NotImplementedError("Only works for a single physical 'p' leg")
    if last_site is None:
        last_site = psi.L - 1
    if rng is None and u is None:
        rng = np.random.default_rng()
    sigmas = []
    total_weight = 1.
    eig = {}
    theta = psi.get_theta(first_site, n=1).replace_label('p0', 'p')
    for i in range(first_site, last_site + 1):
        dim = theta.get_leg('p').ind_len
        if ops is not None:
            W, V = _eig_basis(psi, ops, i, first_site, eig)
            theta = npc.tensordot(V.conj(), theta, axes=['p*', 'p']).replace_label('eig*', 'p')
        else:
            W = np.arange(dim)
        rho = npc.tensordot(theta.conj(), theta, [['vL*', 'vR*'], ['vL', 'vR']])
        rho_diag = np.abs(np.diag(rho.to_ndarray()))
        if abs(np.sum(rho_diag) - 1.) > norm_tol:
            raise ValueError('not normalized to `norm_tol`')
        rho_diag /= np.sum(rho_diag)
        if u is None:
            sigma = rng.choice(dim, p=rho_diag)
        else:
            cdf = rho_diag.cumsum()
            cdf /= cdf[-1]
            uu = u[i - first_site]
            sigma = int(cdf.searchsorted(uu, side='right'))
            if margins is not None:
                margins.append(float(np.min(np.abs(np.concatenate([[0.], cdf]) - uu))))
        sigmas.append(W[sigma])
        theta = theta.take_slice(sigma, 'p')
        weight = npc.norm(theta)
        total_weight *= weight
        if i != last_site:
            theta = theta / npc.norm(theta)
            theta = npc.tensordot(theta, psi.get_B(i + 1, 'B'), axes=['vR', 'vL'])
        elif psi.bc == 'finite' and first_site == 0 and last_site == psi.L - 1:
            assert theta.shape == (1, 1)
            total_weight = total_weight * theta.to_ndarray()[0, 0] / weight
        if not complex_amplitude:
            total_weight = np.abs(total_weight)**2
    return sigmas, total_weight


def _weights(w, phase, full, complex_amplitude):
    """The reference's bookkeeping of ``total_weight`` (mps.py:4428, :4438-4441) for all samples at once, site by site."""
    n, n_sites = w.shape
    tw = np.ones(n, dtype=np.float64)
    for k in range(n_sites):
        tw = tw * w[:, k]
        if k == n_sites - 1 and full:
            tw = tw * phase         # (theta_00 / w: the gather launch has divided already)
        if not complex_amplitude:
            tw = np.abs(tw)**2
    return tw


def sample_measurements(psi, first_site=0, last_site=None, ops=None, rng=None, norm_tol=1.e-12, complex_amplitude=True, n_samples=None,
                        why=False, generic=None):
    """``MPS.sample_measurements`` with the extra keyword ``n_samples``: ``None`` returns what the reference returns for one sample (a
    list and a scalar), n returns ``(ndarray (n, n_sites), ndarray (n,))`` -- outcome for outcome what n consecutive reference calls on
    the same generator return.  From the batched walk, or -- with the reason ``why`` (default: ``decline_reason``; counted in
    ``sample_stats``) -- sample by sample from ``generic`` (default: ``sample_generic``, which raises the reference's
    ``NotImplementedError`` for a state with several physical legs)."""
    if last_site is None:
        last_site = psi.L - 1
    if rng is None:
        rng = np.random.default_rng()
    if why is False:
        why = decline_reason(psi, first_site, last_site, n_samples)
    n = 1 if n_samples is None else int(n_samples)
    n_sites = last_site - first_site + 1
    if why is not None:
        sample_stats['generic'] += 1
        _count_why(why)
        if generic is None:
            def generic():
                return sample_generic(psi, first_site, last_site, ops, rng, norm_tol, complex_amplitude)
        if n_samples is None:
            return generic()
        res = [generic() for _ in range(n)]
        weights = np.array([r[1] for r in res])
        return np.array([r[0] for r in res]).reshape(n, n_sites), weights
    sample_stats['device'] += 1
    u = rng.random((n, n_sites))
    sigma, Ws, w, phase = device_sample(psi, n, last_site, u, ops, norm_tol, first_site)
    full = psi.bc == 'finite' and first_site == 0 and last_site == psi.L - 1
    weights = _weights(w, phase, full, complex_amplitude)
    if Ws is None:
        outcomes = sigma
    else:
        outcomes = np.stack([np.asarray(Ws[k])[sigma[:, k]] for k in range(n_sites)], axis=1)
    if n_samples is None:
        return list(outcomes[0]), weights[0]
    return outcomes, weights
