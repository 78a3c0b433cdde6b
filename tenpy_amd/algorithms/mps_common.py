"""Effective Hamiltonians: the Lanczos matvec of the hot path (``TwoSiteH``; ``OneSiteH`` / ``ZeroSiteH`` of TDVP at the end of the file).

Mirrors ``TwoSiteH`` of ``tenpy/algorithms/mps_common.py`` (:1245; ``matvec`` :1321-1348, ``combine_Heff``
:1350, ``combine_theta`` :1374, ``update_LP`` :1421, ``update_RP`` :1430) for ``combine=True``:

    |theta'> = LHeff . theta . RHeff          (two block-sparse tensordots)

MI355X-first differences:
* the leg order of ``RHeff`` is chosen so that NEITHER tensordot of the matvec needs a transpose
  (the reference calls ``itranspose`` inside ``matvec`` :1339): LHeff = [(vR*.p0), wR, (vR.p0*)],
  RHeff = [wL, (p1*.vL), (p1.vL*)];
* both contraction plans are built once per bond and replayed for every Lanczos step: one matvec is
  exactly two grouped-GEMM launches, no host planning, no allocation besides the result arena;
* ``factored`` mode (default when every block of W0, W1 is a single number, or a small matrix on the physical index between 1-wide
  blocks of the MPO bond legs -- sites with several states per charge sector --, or, entry by entry, any block structure of a
  charged MPO: sorted and bunched MPO bond legs, wide sectors, ``MpoEntryApplyPlan``): the same operator applied as
  ``LP . theta . (W0 W1) . RP`` -- two GEMM launches with a factor d fewer flops (the physical legs are not fused into
  the contracted index) plus one block-level linear combination for the two MPO tensors; LHeff / RHeff are then only
  built on demand (mixer, tests).  theta stays in its un-fused form (vL, p0, p1, vR) during the Lanczos iteration and
  is fused once for the SVD (``prepare_svd``).  Same result as the fused path to rounding (tests/test_heff.py).
"""
import numpy as np

from ..linalg import _device as dev
from ..linalg import np_conserved as npc

__all__ = ['TwoSiteH', 'OneSiteH', 'ZeroSiteH']


FUSED_HEFF = True     # tuning / test hook: False forces the generic tensordot + combine_legs construction
import os as _os
FACTORED_MATVEC = _os.environ.get('TPA_FACTORED_MATVEC', '1') != '0'   # tuning / test hook: False = always LHeff . theta . RHeff (the reference's combine=True form)
# The factored form trades d times fewer flops for more and smaller GEMMs plus one extra pass: it pays when the GEMMs are
# compute bound (Heisenberg chi=2048: 0.80 vs 1.37 ms per matvec) and loses when they are launch bound (chi=256: 0.75 vs
# 0.54 s per sweep; Hubbard ladder chi=1024 with sectors <= 100 wide: 3.7 vs 1.5 s).  Automatic choice: largest bond sector.
FACTORED_MIN_SECTOR = 200
# MPO tensors whose physical charge sectors hold several states (MPO bond legs still 1-wide): the MPO step of the factored forms as
# small dense matrices on the physical index (``MpoBlockApplyPlan``, tpa_mpo_apply_batch).  A/B knob: '0' = the routing without it.
BLOCK_APPLY = _os.environ.get('TPA_MPO_BLOCK_APPLY', '1') != '0'
from .._lib import MPO_APPLY_MAXD      # noqa: E402  (TPA_MPO_APPLY_MAXD)
# MPO tensors neither of the two plans above serves -- MPO bond legs with blocks wider than 1 (sorted and bunched bond legs), physical
# sectors wider than ``TPA_MPO_APPLY_MAXD`` (two sites: their product): the MPO step entry by entry (``MpoEntryApplyPlan``,
# tpa_mpo_entry_apply_batch).  0 = the routing without it, 1 = MPOs with a conserved charge, 2 = also MPOs without one.  2 is not the
# default: tests/test_onesite_heff.py::test_generic_route_without_charges states the reference's contractions as the route of a
# charge-free MPO on both backends, and nothing has been measured that would justify moving it.
ENTRY_APPLY = int(_os.environ.get('TPA_MPO_ENTRY_APPLY', '1'))
# The launch program of the factored two-site matvec without the work nobody reads (``TwoSiteH._skip_program``): blocks of
# T1 that no term of the MPO step reads are not computed, and a block of T3 that is one term ``alpha . block of T1`` is read from T1 by
# a scaled link of ``tpa_gemm_chain_ex`` instead of being written and read back.  The bits of the full program.  A/B knob: '0' = off.
MATVEC_SKIP = _os.environ.get('TPA_MATVEC_UNIT', '1') != '0'

# ---------------------------------------------------------------------------------------------------------------------
# Fused construction of LHeff / RHeff:  LP.W0 (resp. W1.RP) + combine_legs in ONE kernel launch.
# When every charge block of the MPO tensor is a single number (all charges resolved: spin-1/2 with Sz, Hubbard with
# (N, Sz), parity-conserving TFI ...), ``tensordot(LP, W0, 'wR'-'wL')`` is a sum of scaled copies of the LP[:, w, :]
# blocks -- as a GEMM it has inner dimension 1 per link (64072 almost empty 64 x 64 tiles for a chi = 2048 Heisenberg
# bond, 1.4 ms) and is followed by a 131 MB repacking copy (combine_legs, 0.2 ms).  ``tpa_lincomb_batch`` writes every
# (w', p, p*) slab of the fused tensor directly at its place inside the pipe blocks.
def _env_set_LP(env, i, LP):
    """``env.set_LP`` with the age (number of physical sites in the part) of the reference (mps_common.py:1427)."""
    if hasattr(env, 'get_LP_age'):
        env.set_LP(i, LP, age=(env.get_LP_age(i - 1) or 0) + 1)
    else:
        env.set_LP(i, LP)


def _env_set_RP(env, i, RP):
    if hasattr(env, 'get_RP_age'):
        env.set_RP(i, RP, age=(env.get_RP_age(i + 1) or 0) + 1)
    else:
        env.set_RP(i, RP)


def _mpo_entries(W):
    """(qdata, values) of an MPO tensor whose stored blocks are all 1 x 1 x 1 x 1, else ``None`` (cached on W)."""
    ent = getattr(W, '_tpa_entries', False)
    if ent is False:
        if all(np.all(leg.get_block_sizes() == 1) for leg in W.legs) and W.stored_blocks > 0:
            vals = np.array([np.asarray(b).reshape(-1)[0] for b in W._data])
            ent = (np.array(W._qdata), vals)
        else:
            ent = None
        W._tpa_entries = ent
    return ent


def _mpo_blocks(W):
    """(qdata, host copies of the stored blocks) of an MPO tensor whose two MPO bond legs have 1-wide blocks and whose physical charge
    sectors are at most ``TPA_MPO_APPLY_MAXD`` wide, else ``None`` (cached on W like ``_tpa_entries``).  Wider bond blocks or sectors
    go entry by entry (``_mpo_coo`` / ``MpoEntryApplyPlan``), and so do MPOs without a conserved charge -- one dense block, no charge
    rule to select the terms -- where ``ENTRY_APPLY`` is 2; by default they keep the reference's contractions."""
    blk = getattr(W, '_tpa_blocks', False)
    if blk is False:
        labels = list(W.get_leg_labels())
        blk = None
        if W.rank == 4 and 'wL' in labels and 'wR' in labels and W.stored_blocks > 0 and W.chinfo.qnumber > 0:
            phys = [a for a in range(4) if labels[a] not in ('wL', 'wR')]
            if all(np.all(W.get_leg(l).get_block_sizes() == 1) for l in ('wL', 'wR')) and \
                    all(int(np.max(W.legs[a].get_block_sizes())) <= MPO_APPLY_MAXD for a in phys):
                blk = (np.array(W._qdata), [np.array(b) for b in W._data])
        W._tpa_blocks = blk
    return blk


def _share_mpo_tables(W_new, W):
    """Hand the host tables cached on the MPO's own tensor ``W`` to its relabelled copy ``W_new`` (one D2H read per site and run)."""
    W_new._tpa_entries = _mpo_entries(W)
    if W_new._tpa_entries is None and BLOCK_APPLY and dev.lib_provides('tpa_mpo_apply_batch'):
        W_new._tpa_blocks = _mpo_blocks(W)
    W_new._tpa_origin = W       # (``_mpo_coo`` reads and caches its table there when a plan first asks for it)


def _mpo_coo(W):
    """(global indices int64[n, 4] in the stored leg order, values) of the nonzero entries of an MPO tensor with legs ``wL``, ``wR``
    and two physical legs, whatever the widths of its blocks; ``None`` for anything else (cached on W like ``_tpa_entries``)."""
    coo = getattr(W, '_tpa_coo', False)
    if coo is False and getattr(W, '_tpa_origin', None) is not None:      # a relabelled copy: the table of the MPO's own tensor
        coo = W._tpa_coo = _mpo_coo(W._tpa_origin)
    if coo is False:
        labels = list(W.get_leg_labels())
        coo = None
        if W.rank == 4 and 'wL' in labels and 'wR' in labels and W.stored_blocks > 0:
            idx, vals = [], []
            for q, b in zip(np.array(W._qdata).tolist(), W._data):
                b = np.array(b)
                nz = np.nonzero(b)
                idx.append(np.stack([nz[a] + int(W.legs[a].slices[q[a]]) for a in range(4)], axis=1))
                vals.append(b[nz])
            coo = (np.concatenate(idx).astype(np.int64).reshape(-1, 4), np.concatenate(vals))
        W._tpa_coo = coo
    return coo


def _pack_alpha(terms, alpha):
    """The coefficients ``alpha`` as the bits of their real and imaginary parts in columns 2 and 3 of the int64 table ``terms``."""
    alpha = np.asarray(alpha, dtype=np.complex128)
    terms[:, 2] = np.ascontiguousarray(alpha.real).view(np.int64)
    terms[:, 3] = np.ascontiguousarray(alpha.imag).view(np.int64)


def _lincomb_into(dst, src, jobs, terms, max_elems):
    if len(jobs) == 0:
        return
    L = dev.lib()
    terms_d = dev.table(terms)
    for s0 in range(0, len(jobs), 60000):
        jd = dev.table(jobs[s0:s0 + 60000])
        dev.check(L.tpa_lincomb_batch(dev.code(dst.dtype), jd.data_ptr(), len(jobs[s0:s0 + 60000]), terms_d.data_ptr(),
                                      int(max_elems), src._arena.data_ptr(), dst._arena.data_ptr(), dev.stream()), "lincomb")


def _rank_rows(q):
    """The distinct rows of ``q`` in the order of a sorted ``_qdata`` (last column most significant), and for every row of ``q`` its
    number in that order."""
    uq, inv = np.unique(q, axis=0, return_inverse=True)
    order = np.lexsort(uq.T)
    rank_of = np.empty(len(order), dtype=np.int64)
    rank_of[order] = np.arange(len(order))
    return uq[order], rank_of[inv.reshape(-1)]


def _group_terms(dst):
    """Terms grouped by their destination ``dst`` (a block number or an offset), in a fixed order: the sorting permutation and, in the
    sorted order, the first term and the number of terms of every destination (one job each)."""
    key = np.lexsort((np.arange(len(dst)), dst))
    d_sorted = dst[key]
    starts = np.nonzero(np.concatenate([[True], d_sorted[1:] != d_sorted[:-1]]))[0]
    return key, starts, np.diff(np.concatenate([starts, [len(key)]]))


from collections import OrderedDict as _OrderedDict
_heff_plans = _OrderedDict()
_skip_table_cache = _OrderedDict()      # ids of the three plans -> (the plans, tables of `TwoSiteH._skip_program`)


def _fused_heff(env_t, W, left):
    """``left``: LHeff [(vR*.p0), wR, (vR.p0*)] from LP [vR*, wR, vR] and W0 [wL, wR, p0, p0*];
    else RHeff [wL, (p1*.vL), (p1.vL*)] from RP [wL, vL, vL*] and W1 [wL, wR, p1, p1*].
    Returns (Heff, pipe) or ``None`` when the fast path does not apply (generic tensordot + combine_legs then)."""
    from ..linalg.charges import LegPipe
    ent = _mpo_entries(W)
    pl = 'p0' if left else 'p1'
    want_env = ['vR*', 'wR', 'vR'] if left else ['wL', 'vL', 'vL*']
    if ent is None or list(env_t.get_leg_labels()) != want_env or list(W.get_leg_labels()) != ['wL', 'wR', pl, pl + '*'] \
            or env_t.dtype != np.result_type(env_t.dtype, W.dtype) or env_t.stored_blocks == 0:
        return None
    wq, wv = ent
    w_axis_env = 1 if left else 0
    if not np.all(env_t.legs[w_axis_env].get_block_sizes() == 1):
        return None
    # Everything below except the two launches is integer bookkeeping that depends on the block structure and the sector charges of
    # the environment tensor and on the MPO tensor: planned once per (bond, direction), replayed on every later visit.
    pkey = (left, env_t._struct_key(), env_t.dtype.str, id(ent), env_t.qtotal.tobytes(),
            tuple((l.charges.tobytes(), int(l.qconj)) for l in env_t.legs))
    plan = _heff_plans.get(pkey)
    if plan is not None and plan['ent'] is ent:
        try:
            _heff_plans.move_to_end(pkey)
        except KeyError:      # evicted by another thread in between (the reference's `+ h.c.` worker contracts concurrently)
            pass
        res = npc.Array(plan['legs'], env_t.dtype, plan['qtotal'], plan['labels'])
        res._adopt_blocks(plan['qdata'], plan['offsets'], dev.zeros(plan['total'], env_t.dtype), True)
        dev.check(dev.lib().tpa_lincomb_batch(dev.code(env_t.dtype), plan['jobs'].data_ptr(), plan['n_jobs'], plan['terms'].data_ptr(),
                                              plan['max_elems'], env_t._arena.data_ptr(), res._arena.data_ptr(), dev.stream()), "lincomb")
        return res, plan['pipe']
    eq = env_t._qdata
    shapes = env_t._block_shapes()
    if left:
        pipe = LegPipe([env_t.get_leg('vR*'), W.get_leg('p0')], qconj=+1)
        legs = [pipe, W.get_leg('wR'), pipe.conj()]
        labels = ['(vR*.p0)', 'wR', '(vR.p0*)']
    else:
        pipe = LegPipe([W.get_leg('p1'), env_t.get_leg('vL*')], qconj=-1)
        legs = [W.get_leg('wL'), pipe.conj(), pipe]
        labels = ['wL', '(p1*.vL)', '(p1.vL*)']
    qm = pipe.q_map
    n0, n1 = pipe.legs[0].block_number, pipe.legs[1].block_number
    row_of = np.full((n0, n1), -1, dtype=np.int64)
    row_of[qm[:, 3], qm[:, 4]] = np.arange(len(qm))
    psz = pipe.get_block_sizes()
    # all (env block, W entry) pairs that share the contracted MPO index
    wc = wq[:, 0] if left else wq[:, 1]            # W index contracted with the environment
    ie, iw = np.nonzero(eq[:, w_axis_env][:, None] == wc[None, :])
    if len(ie) == 0:
        return None
    if left:      # rows (vR*, p0), cols (vR, p0*)
        r_row = row_of[eq[ie, 0], wq[iw, 2]]
        c_row = row_of[eq[ie, 2], wq[iw, 3]]
        w_out = wq[iw, 1]
        rows, cols = shapes[ie, 0], shapes[ie, 2]
    else:         # rows (p1*, vL), cols (p1, vL*)
        r_row = row_of[wq[iw, 3], eq[ie, 1]]
        c_row = row_of[wq[iw, 2], eq[ie, 2]]
        w_out = wq[iw, 0]
        rows, cols = shapes[ie, 1], shapes[ie, 2]
    Qr, Qc = qm[r_row, 2], qm[c_row, 2]
    r0, c0 = qm[r_row, 0], qm[c_row, 0]
    bq = np.stack([Qr, w_out, Qc], axis=1) if left else np.stack([w_out, Qr, Qc], axis=1)
    ubq, blk = _rank_rows(bq)
    res = npc.Array(legs, env_t.dtype, env_t.chinfo.make_valid(env_t.qtotal + W.qtotal), labels)
    res._set_blocks(ubq, zero=True, qdata_sorted=True)
    ld = psz[Qc]
    dst_off = res._offsets[blk] + r0 * ld + c0
    # one job per destination slab, its terms = all contributions landing there (deterministic order)
    perm, starts, counts = _group_terms(dst_off)
    jobs = np.zeros((len(starts), 8), dtype=np.int64)
    pf = perm[starts]
    jobs[:, 0], jobs[:, 1], jobs[:, 2], jobs[:, 3] = dst_off[pf], rows[pf], cols[pf], ld[pf]
    jobs[:, 4], jobs[:, 5] = starts, counts
    terms = np.zeros((len(perm), 4), dtype=np.int64)
    terms[:, 0] = env_t._offsets[ie[perm]]
    terms[:, 1] = shapes[ie[perm], 2]
    _pack_alpha(terms, wv[iw[perm]])
    _lincomb_into(res, env_t, jobs, terms, int(np.max(rows * cols)))
    if 0 < len(jobs) <= 60000:
        for arr in (res._qdata, res._offsets):
            arr.setflags(write=False)
        _heff_plans[pkey] = dict(ent=ent, legs=legs, labels=labels, qtotal=res.qtotal.copy(), qdata=res._qdata, offsets=res._offsets,
                                 total=int(res._arena.numel()), jobs=dev.table(jobs), terms=dev.table(terms), n_jobs=len(jobs),
                                 max_elems=int(np.max(rows * cols)), pipe=pipe)
        if len(_heff_plans) > 8192:
            _heff_plans.popitem(last=False)
    return res, pipe


def _reverse_columns(U):
    """Rank-2 ``U`` with the columns of every block in reversed order (one strided slab copy per column, one launch)."""
    res = npc.Array(U.legs, U.dtype, U.qtotal, list(U._labels))
    res._set_blocks(U._qdata, zero=False, qdata_sorted=U._qdata_sorted)
    if U.stored_blocks == 0:
        return res
    shapes = U._block_shapes()
    m, k = shapes[:, 0], shapes[:, 1]
    blk = np.repeat(np.arange(len(k)), k)
    col = np.arange(len(blk)) - np.repeat(np.cumsum(k) - k, k)
    jobs = np.zeros((len(blk), 8), dtype=np.int64)
    jobs[:, 0] = res._offsets[blk] + col
    jobs[:, 1], jobs[:, 2], jobs[:, 3] = m[blk], 1, k[blk]
    jobs[:, 4], jobs[:, 5] = np.arange(len(blk)), 1
    terms = np.zeros((len(blk), 4), dtype=np.int64)
    terms[:, 0] = U._offsets[blk] + (k[blk] - 1 - col)
    terms[:, 1] = k[blk]
    terms[:, 2] = np.array([1.0]).view(np.int64)[0]
    _lincomb_into(res, U, jobs, terms, int(np.max(m)))
    return res


def _relabel_view(A, labels):
    """``A`` with its legs in the order ``labels`` WITHOUT moving data: allowed when only legs with 1-wide blocks change
    their position relative to the others (the memory layout of every block is then unchanged); bookkeeping only."""
    perm = [A.get_leg_index(l) for l in labels]
    if perm == list(range(A.rank)):
        return A
    big = [a for a in range(A.rank) if not np.all(A.legs[a].get_block_sizes() == 1)]
    assert [a for a in perm if a in big] == big, "only legs with 1-wide blocks may be moved"
    B = A.copy(deep=False)
    B.legs = [A.legs[a] for a in perm]
    B._set_shape()
    B._labels = [A._labels[a] for a in perm]
    B._qdata = np.ascontiguousarray(A._qdata[:, perm])
    B._offsets = A._offsets.copy()
    B._qdata_sorted = False
    B._skey = None
    B.isort_qdata()
    return B


class _MpoStepPlan:
    """What the three plans of the MPO step share -- ``MpoApplyPlan`` (scalar MPO blocks), ``MpoBlockApplyPlan`` (small matrices) and
    ``MpoEntryApplyPlan`` (entry by entry): the cached constructor, the bookkeeping of the result Y and ``apply``.  A subclass has a
    ``_cache`` dict of its own (``npc.clear_device_caches`` clears them by class), ``_table(W)``, the reader of the host table of an MPO
    tensor that its job tables are built from, ``_launch(X, res)``, the call of its kernel, and ``program_op``."""

    @classmethod
    def get(cls, X, W, *args, W2=None, **kwargs):
        """Cached constructor: the plan depends on the block structure of X and on the MPO tensors only."""
        t1, t2 = cls._table(W), (None if W2 is None else cls._table(W2))
        key = (X._struct_key(), str(X.dtype), id(t1), None if t2 is None else id(t2), args,
               tuple(sorted(kwargs.items())), tuple(X.get_leg_labels()))
        plan = cls._cache.get(key)
        if plan is None or plan._tables_alive[0] is not t1 or plan._tables_alive[1] is not t2:
            if len(cls._cache) > 4096:
                cls._cache.clear()
            plan = cls._cache[key] = cls(X, W, *args, W2=W2, **kwargs)
            # the key holds id()s: keep the host tables alive as long as the plan is cached, so that the id of a dead
            # MPO's table can never be handed to a new one (a stale plan would apply the OLD couplings)
            plan._tables_alive = (t1, t2)
        return plan

    @staticmethod
    def _match_blocks(X, keys, xa):
        """All (block of X, term) pairs for terms with the block indices ``keys`` = (w_in, w_out, p_out, p_in [, p2_out, p2_in]) that
        act on the legs ``xa`` of X: the block of X and the term of every pair, and its block indices in Y (in the leg order of X)."""
        xq = X._qdata
        match = xq[:, xa[0]][:, None] == keys[None, :, 0]
        for a, col in zip(xa[1:], (3, 5)):
            match &= xq[:, a][:, None] == keys[None, :, col]
        ib, ie = np.nonzero(match)
        oq = xq[ib].copy()
        for a, col in zip(xa, (1, 2, 4)):
            oq[:, a] = keys[ie, col]
        return ib, ie, oq

    def _set_output(self, X, W, W2, xa, w_out, p_out, p2_out, out_labels):
        """``dtype``, ``qtotal``, ``legs`` and ``labels`` of Y: those of X with the legs ``xa`` (MPO leg, physical leg [, second physical
        leg]) replaced by the open legs of W (, W2), in the order ``out_labels``.  Returns the legs in the order of X and ``perm``, the
        position in X of every leg of Y."""
        self.dtype = np.result_type(X.dtype, W.dtype) if W2 is None else np.result_type(X.dtype, W.dtype, W2.dtype)
        self.qtotal = X.chinfo.make_valid(X.qtotal + W.qtotal + (0 if W2 is None else W2.qtotal))
        legs, labels = list(X.legs), list(X.get_leg_labels())
        legs[xa[0]], labels[xa[0]] = (W if W2 is None else W2).get_leg(w_out), w_out
        legs[xa[1]], labels[xa[1]] = W.get_leg(p_out), p_out
        if W2 is not None:
            legs[xa[2]], labels[xa[2]] = W2.get_leg(p2_out), p2_out
        perm = [labels.index(l) for l in out_labels]
        self.legs = [legs[a] for a in perm]
        self.labels = list(out_labels)
        return legs, perm

    def _rank_blocks(self, oq):
        """``qdata``, ``offsets`` and ``total`` of Y from ``oq``, the block indices in Y of every (block of X, term of W) pair.  Returns
        the block number in Y of every pair and the block sizes of Y."""
        uq, blk = _rank_rows(oq)
        self.qdata = np.ascontiguousarray(uq, dtype=np.intp)
        proto = npc.Array(self.legs, self.dtype, self.qtotal, self.labels)
        sizes = proto._set_blocks(self.qdata, arena=dev.empty(0, self.dtype), qdata_sorted=True)
        self.offsets = proto._offsets
        self.total = int(np.sum(sizes))
        return blk, sizes

    def apply(self, X, launch=True):
        """Y as a new Array; ``launch=False``: its block structure and an unwritten arena only (a launch program is being assembled)."""
        res = npc.Array(self.legs, self.dtype, self.qtotal, self.labels)
        if self.empty:
            return res
        if X.dtype != self.dtype:
            X = X.astype(self.dtype)
        res._set_blocks(self.qdata, arena=dev.empty(self.total, self.dtype), qdata_sorted=True)
        if launch:
            self._launch(X, res)
        return res


class MpoApplyPlan(_MpoStepPlan):
    """``Y[.., w', p, ..] = sum_{w, p'} W[w, w', p, p'] X[.., w, p', ..]`` for an MPO tensor whose blocks are single
    numbers: every block of Y is a linear combination of whole blocks of X (the w and p legs of X have 1-wide blocks, so
    a block of X and the blocks of Y it feeds have the same memory layout).  One ``tpa_lincomb_batch`` launch; the job
    tables are built once from the block structure of X and replayed.  With ``W2`` the two neighbouring MPO tensors
    W W2 (summed over their common bond) are applied in the same single pass.

    ``x_w``, ``x_p`` (, ``x_p2``) : labels of X's MPO leg and physical leg(s) to be contracted.
    ``w_in`` / ``w_out``          : labels of the MPO legs contracted with X / left open ('wL', 'wR' when going left to right).
    ``p_out`` / ``p_in``          : labels of W's physical legs left open / contracted ('p0', 'p0*'); ``p2_out`` / ``p2_in`` for W2.
    ``out_labels``                : order of the legs of Y (must keep the relative order of X's non-trivial legs).
    """
    _cache = {}
    _table = staticmethod(_mpo_entries)

    def __init__(self, X, W, x_w, x_p, w_in, w_out, p_out, p_in, out_labels, W2=None, x_p2=None, p2_out=None, p2_in=None):
        ent = self._table(W)
        assert ent is not None
        wq, wv = ent
        wl = list(W.get_leg_labels())
        xa = [X.get_leg_index(l) for l in ((x_w, x_p) if W2 is None else (x_w, x_p, x_p2))]
        assert all(np.all(X.legs[a].get_block_sizes() == 1) for a in xa)
        # entry table: (w_in, w_out, p_out, p_in [, p2_out, p2_in]) -> value
        keys, vals = wq[:, [wl.index(l) for l in (w_in, w_out, p_out, p_in)]], np.asarray(wv)
        if W2 is not None:
            wq2, wv2 = self._table(W2)
            wl2 = list(W2.get_leg_labels())
            keys2 = wq2[:, [wl2.index(l) for l in (w_in, w_out, p2_out, p2_in)]]
            i1, i2 = np.nonzero(keys[:, 1][:, None] == keys2[:, 0][None, :])      # join over the common MPO bond
            joined = np.stack([keys[i1, 0], keys2[i2, 1], keys[i1, 2], keys[i1, 3], keys2[i2, 2], keys2[i2, 3]], axis=1)
            prod = vals[i1] * np.asarray(wv2)[i2]
            uk, inv = np.unique(joined, axis=0, return_inverse=True)
            tot = np.zeros(len(uk), dtype=prod.dtype)
            np.add.at(tot, inv.reshape(-1), prod)
            keys, vals = uk[tot != 0], tot[tot != 0]
        ib, ie, oq = self._match_blocks(X, keys, xa)
        legs, perm = self._set_output(X, W, W2, xa, w_out, p_out, p2_out, out_labels)
        big = [a for a in range(X.rank) if not np.all(legs[a].get_block_sizes() == 1)]
        assert [a for a in perm if a in big] == big, "out_labels must keep the order of the non-trivial legs"
        self.empty = len(ib) == 0
        if self.empty:
            return
        blk, sizes = self._rank_blocks(oq[:, perm])
        sizes_x = X._block_sizes_flat()
        key, starts, counts = _group_terms(blk)
        jobs = np.zeros((len(starts), 8), dtype=np.int64)
        sz = sizes[blk[key[starts]]]
        jobs[:, 0], jobs[:, 1], jobs[:, 2], jobs[:, 3] = self.offsets[blk[key[starts]]], 1, sz, sz
        jobs[:, 4], jobs[:, 5] = starts, counts
        terms = np.zeros((len(key), 4), dtype=np.int64)
        terms[:, 0] = X._offsets[ib[key]]
        terms[:, 1] = sizes_x[ib[key]]
        _pack_alpha(terms, vals[ie[key]])
        assert len(jobs) <= 60000
        self.jobs_host, self.terms_host, self.sizes = jobs, terms, sizes      # (row-restricted copies: algorithms/sharded.py)
        self.jobs_dev, self.terms_dev = dev.to_device(jobs), dev.to_device(terms)
        self.n_jobs, self.max_elems = len(jobs), int(np.max(sz))
        self.x_key = X._struct_key()
        self.bytes = 8 * (2 if self.dtype.kind == 'c' else 1) * (self.total + int(np.sum(sizes_x[ib])))

    def _launch(self, X, res):
        dev.check(dev.lib().tpa_lincomb_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.terms_dev.data_ptr(),
                                              self.max_elems, X._arena.data_ptr(), res._arena.data_ptr(), dev.stream()), "lincomb")

    def program_op(self, a_slot, c_slot):
        """The row of a ``tpa_lanczos_run`` program that applies this plan from slot ``a_slot`` into slot ``c_slot`` (kind 1)."""
        return [1, 0, self.jobs_dev.data_ptr(), self.terms_dev.data_ptr(), 0, self.n_jobs, a_slot, 0, c_slot, self.max_elems, 0, 0]


def _entry_route(chinfo):
    """Whether the entry-by-entry MPO step may serve tensors of this charge structure (switches and the installed library)."""
    return (ENTRY_APPLY > 0 and BLOCK_APPLY and (chinfo.qnumber > 0 or ENTRY_APPLY == 2) and
            dev.lib_provides('tpa_mpo_entry_apply_batch'))


_STANDARD_W_LABELS = (['wL', 'wR', 'p', 'p*'], ['wL', 'wR', 'p0', 'p0*'], ['wL', 'wR', 'p1', 'p1*'])


def _mpo_entry_plan_class(W, W2=None):
    """``MpoEntryApplyPlan`` where it may serve ``W`` (and ``W2``), else ``None``: asked only where the two older plans decline."""
    if not _entry_route(W.chinfo):
        return None
    for T in (W,) if W2 is None else (W, W2):
        if list(T.get_leg_labels()) not in _STANDARD_W_LABELS or _mpo_coo(T) is None:
            return None
    return MpoEntryApplyPlan


def _phys_width(W):
    return max(int(np.max(leg.get_block_sizes())) for leg, l in zip(W.legs, W.get_leg_labels()) if l not in ('wL', 'wR'))


def _mpo_plan_class(W, W2=None):
    """The plan class that applies the MPO tensor ``W`` (with ``W2``: both neighbours in one pass) to the blocks of a tensor:
    ``MpoApplyPlan`` when every stored block is a single number, ``MpoBlockApplyPlan`` when the MPO bond legs have 1-wide blocks and
    the physical sectors (two sites: their products) are at most ``TPA_MPO_APPLY_MAXD`` wide and the installed library provides
    ``tpa_mpo_apply_batch``; ``MpoEntryApplyPlan`` where both decline and the tensors carry the standard labels, the MPO has a
    conserved charge (or ``ENTRY_APPLY`` is 2) and the library provides ``tpa_mpo_entry_apply_batch``; ``None`` when there is no
    blockwise form.  ``BLOCK_APPLY`` off restores the routing before both of the younger plans."""
    if _mpo_entries(W) is not None and (W2 is None or _mpo_entries(W2) is not None):
        return MpoApplyPlan
    if not BLOCK_APPLY:
        return None
    if not dev.lib_provides('tpa_mpo_apply_batch'):
        return _mpo_entry_plan_class(W, W2)
    if _mpo_blocks(W) is None or (W2 is not None and _mpo_blocks(W2) is None):
        return _mpo_entry_plan_class(W, W2)
    if _phys_width(W) * (1 if W2 is None else _phys_width(W2)) > MPO_APPLY_MAXD:
        return _mpo_entry_plan_class(W, W2)
    return MpoBlockApplyPlan


class MpoBlockApplyPlan(_MpoStepPlan):
    """``MpoApplyPlan`` for MPO tensors whose physical charge sectors hold several states (MPO bond legs still with 1-wide blocks):
    only the 1-wide ``w`` leg changes its position, so a block of X ``(.., w, p [, p2], ..)`` is ``(pre, D_in, post)`` in memory and
    the block of Y it feeds is ``(pre, D_out, post)`` (two sites: ``D = d0 d1``) -- every block of Y is a sum of small dense matrices
    applied on the physical index of blocks of X.  One ``tpa_mpo_apply_batch`` launch.  With ``W2`` the matrix of a
    ``(w_in, w_out, sectors)`` term is ``sum_w'' W[w_in, w''] (x) W2[w'', w_out]``, formed once on the host; terms whose matrix is
    exactly zero are dropped.  Arguments and attributes: see ``MpoApplyPlan``."""
    _cache = {}
    _table = staticmethod(_mpo_blocks)

    @staticmethod
    def _entries(W, w_in, w_out, p_out, p_in):
        """keys (w_in, w_out, p_out sector, p_in sector) and the (d_out, d_in) matrices of the stored blocks of ``W``."""
        wq, blocks = _mpo_blocks(W)
        wl = list(W.get_leg_labels())
        ax = [wl.index(w_in), wl.index(w_out), wl.index(p_out), wl.index(p_in)]
        mats = [np.transpose(b, ax).reshape(b.shape[ax[2]], b.shape[ax[3]]) for b in blocks]
        return wq[:, ax], mats

    def __init__(self, X, W, x_w, x_p, w_in, w_out, p_out, p_in, out_labels, W2=None, x_p2=None, p2_out=None, p2_in=None):
        keys, mats = self._entries(W, w_in, w_out, p_out, p_in)
        xa = [X.get_leg_index(l) for l in ((x_w, x_p) if W2 is None else (x_w, x_p, x_p2))]
        xa_w, xa_p = xa[:2]
        assert np.all(X.legs[xa_w].get_block_sizes() == 1)
        rest = [a for a in range(X.rank) if a != xa_w]      # memory order of a block (the w leg has extent 1)
        if W2 is not None:
            assert rest.index(xa[2]) == rest.index(xa_p) + 1, "the two physical legs must be neighbours in memory"
            keys2, mats2 = self._entries(W2, w_in, w_out, p2_out, p2_in)
            joined = {}
            for k1, m1 in zip(keys.tolist(), mats):         # join over the common MPO bond, in table order
                for k2, m2 in zip(keys2.tolist(), mats2):
                    if k1[1] == k2[0]:
                        k = (k1[0], k2[1], k1[2], k1[3], k2[2], k2[3])
                        m = np.kron(m1, m2)
                        joined[k] = joined[k] + m if k in joined else m
            kept = sorted(k for k, m in joined.items() if np.any(m != 0))
            keys = np.array(kept, dtype=np.int64).reshape(-1, 6)
            mats = [joined[k] for k in kept]
        else:
            keep = [n for n, m in enumerate(mats) if np.any(m != 0)]
            keys, mats = keys[keep], [mats[n] for n in keep]
        _, perm = self._set_output(X, W, W2, xa, w_out, p_out, p2_out, out_labels)
        assert [a for a in perm if a != xa_w] == rest, "out_labels must keep the order of the legs other than the MPO leg"
        ib, ie, oq = self._match_blocks(X, keys, xa)        # (no surviving key: ``keys`` has no rows and there is no pair)
        self.empty = len(ib) == 0
        if self.empty:
            return
        blk, sizes = self._rank_blocks(oq[:, perm])
        # coefficient table: the matrices back to back, row-major (d_out, d_in)
        m_shape = np.array([m.shape for m in mats], dtype=np.int64)
        m_off = np.concatenate([[0], np.cumsum(m_shape[:, 0] * m_shape[:, 1])])
        coeff = np.concatenate([np.asarray(m, dtype=self.dtype).reshape(-1) for m in mats])
        shapes_x, sizes_x = X._block_shapes(), X._block_sizes_flat()
        lead = rest[:rest.index(xa_p)]
        pre = np.prod(shapes_x[:, lead], axis=1) if lead else np.ones(len(shapes_x), dtype=np.int64)
        d_in = m_shape[:, 1]
        post = sizes_x // (pre * shapes_x[:, xa_p] * (1 if W2 is None else shapes_x[:, xa[2]]))
        assert np.array_equal(pre[ib] * d_in[ie] * post[ib], sizes_x[ib])
        key, starts, counts = _group_terms(blk)             # one job per block of Y, its terms in a fixed order
        kf = key[starts]
        jobs = np.zeros((len(starts), 8), dtype=np.int64)
        jobs[:, 0], jobs[:, 1], jobs[:, 2], jobs[:, 3] = self.offsets[blk[kf]], pre[ib[kf]], m_shape[ie[kf], 0], post[ib[kf]]
        jobs[:, 4], jobs[:, 5] = starts, counts
        assert np.array_equal(jobs[:, 1] * jobs[:, 2] * jobs[:, 3], sizes[blk[kf]])
        terms = np.zeros((len(key), 4), dtype=np.int64)
        terms[:, 0], terms[:, 1], terms[:, 2] = X._offsets[ib[key]], d_in[ie[key]], m_off[ie[key]]
        assert len(jobs) <= 60000
        self.jobs_host, self.terms_host, self.coeff_host, self.sizes = jobs, terms, coeff, sizes
        self.jobs_dev, self.terms_dev, self.coeff_dev = dev.to_device(jobs), dev.to_device(terms), dev.to_device(coeff)
        self.n_jobs, self.max_elems = len(jobs), int(np.max(sizes[blk[kf]]))
        self.max_d = int(max(np.max(jobs[:, 2]), np.max(terms[:, 1])))
        assert self.max_d <= MPO_APPLY_MAXD
        self.x_key = X._struct_key()
        self.bytes = 8 * (2 if self.dtype.kind == 'c' else 1) * (self.total + int(np.sum(sizes_x[ib])))

    def _launch(self, X, res):
        dev.check(dev.lib().tpa_mpo_apply_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.terms_dev.data_ptr(),
                                                self.coeff_dev.data_ptr(), self.max_d, self.max_elems, X._arena.data_ptr(),
                                                res._arena.data_ptr(), dev.stream()), "mpo_apply")

    def program_op(self, a_slot, c_slot):
        """The row of a ``tpa_lanczos_run`` program that applies this plan from slot ``a_slot`` into slot ``c_slot`` (kind 5)."""
        return [5, 0, self.jobs_dev.data_ptr(), self.terms_dev.data_ptr(), self.coeff_dev.data_ptr(), self.n_jobs, a_slot, self.max_d,
                c_slot, self.max_elems, 0, 0]


def _leg_block_pos(leg, idx):
    """(block number, position inside the block) of the global indices ``idx`` of ``leg``."""
    sl = np.asarray(leg.slices, dtype=np.int64)
    b = np.searchsorted(sl, idx, side='right') - 1
    return b, idx - sl[b]


def _join_entries_blocks(X, mid, b_in, n_entries):
    """All (block of X, entry of W) pairs whose in-blocks agree on the legs ``mid`` of X -- ``b_in[a]``: the block of every entry on leg
    ``a`` --: a sorted join on the combined block number of these legs.  Returns the block and the entry of every pair, ordered by
    block, the entries of a block in table order."""
    xq = X._qdata
    key_e, key_x = np.zeros(n_entries, dtype=np.int64), np.zeros(len(xq), dtype=np.int64)
    for a in mid:
        n = X.legs[a].block_number
        key_e, key_x = key_e * n + b_in[a], key_x * n + xq[:, a]
    oe = np.argsort(key_e, kind='stable')
    lo, hi = np.searchsorted(key_e[oe], key_x, side='left'), np.searchsorted(key_e[oe], key_x, side='right')
    cnt = hi - lo
    ib = np.repeat(np.arange(len(xq)), cnt)
    ie = oe[np.arange(len(ib)) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)]
    return ib, ie


class MpoEntryApplyPlan(_MpoStepPlan):
    """``MpoApplyPlan`` for MPO tensors of any block structure -- MPO bond legs with blocks wider than 1, physical sectors wider than
    ``TPA_MPO_APPLY_MAXD``, no conserved charge -- entry by entry.  X has its two virtual legs first and last and the MPO and physical
    legs between them, so a block of X is ``(pre, M_in, post)`` in memory and the block of Y it feeds is ``(pre, M_out, post)`` with the
    middle legs in the order of ``out_labels``: a single entry of W (two sites: of ``sum_w'' W[w, w''] W2[w'', w']``, joined once on the
    host, exact zeros dropped) takes one middle row of a block of X to one middle row of a block of Y; the global indices map to
    (block, position inside the block) through the leg slices.  One ``tpa_mpo_entry_apply_batch`` launch with one job per block of Y,
    or -- calls with few blocks -- per range of its rows.  Arguments and attributes: see ``MpoApplyPlan``."""
    _cache = {}
    SPLIT_BELOW = 512       # calls with fewer blocks of Y than this split the rows of a block over several jobs
    _table = staticmethod(_mpo_coo)

    @staticmethod
    def _entries(W, w_in, w_out, p_out, p_in):
        """Global indices (w_in, w_out, p_out, p_in) and values of the nonzero entries of ``W``."""
        idx, vals = _mpo_coo(W)
        wl = list(W.get_leg_labels())
        return idx[:, [wl.index(w_in), wl.index(w_out), wl.index(p_out), wl.index(p_in)]], vals

    def __init__(self, X, W, x_w, x_p, w_in, w_out, p_out, p_in, out_labels, W2=None, x_p2=None, p2_out=None, p2_in=None):
        keys, vals = self._entries(W, w_in, w_out, p_out, p_in)
        if W2 is not None:              # join over the common MPO bond; equal keys are summed in a fixed order
            keys2, vals2 = self._entries(W2, w_in, w_out, p2_out, p2_in)
            o2 = np.argsort(keys2[:, 0], kind='stable')
            lo, hi = np.searchsorted(keys2[o2, 0], keys[:, 1], side='left'), np.searchsorted(keys2[o2, 0], keys[:, 1], side='right')
            i1 = np.repeat(np.arange(len(keys)), hi - lo)
            i2 = o2[np.arange(len(i1)) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo) + np.repeat(lo, hi - lo)]
            joined = np.stack([keys[i1, 0], keys2[i2, 1], keys[i1, 2], keys[i1, 3], keys2[i2, 2], keys2[i2, 3]], axis=1)
            uk, inv = np.unique(joined, axis=0, return_inverse=True)
            tot = np.zeros(len(uk), dtype=np.result_type(vals.dtype, vals2.dtype))
            np.add.at(tot, inv.reshape(-1), vals[i1] * vals2[i2])
            keep = tot != 0
            keys, vals = uk[keep], tot[keep]
        xa = [X.get_leg_index(l) for l in ((x_w, x_p) if W2 is None else (x_w, x_p, x_p2))]
        legs, perm = self._set_output(X, W, W2, xa, w_out, p_out, p2_out, out_labels)
        mid = list(range(1, X.rank - 1))
        assert sorted(xa) == mid and perm[0] == 0 and perm[-1] == X.rank - 1, "X: virtual legs first and last, the MPO step between them"
        # (block, position) of every entry on the legs of X (in) and of Y (out); columns of `keys`: w_in, w_out, p_out, p_in [, p2_out, p2_in]
        col_in, col_out = [0, 3, 5], [1, 2, 4]
        b_in, pos_in, b_out, pos_out = {}, {}, {}, {}
        for n, a in enumerate(xa):
            b_in[a], pos_in[a] = _leg_block_pos(X.legs[a], keys[:, col_in[n]])
            b_out[a], pos_out[a] = _leg_block_pos(legs[a], keys[:, col_out[n]])
        xq = X._qdata
        ib, ie = _join_entries_blocks(X, mid, b_in, len(keys))
        self.empty = len(ib) == 0
        if self.empty:
            return
        oq = xq[ib].copy()
        for a in mid:
            oq[:, a] = b_out[a][ie]
        blk, sizes = self._rank_blocks(oq[:, perm])
        # middle row of the source (order of X's legs) and of the destination (order of out_labels) of every pair
        shapes_x, sizes_x = X._block_shapes(), X._block_sizes_flat()
        c = np.zeros(len(ib), dtype=np.int64)
        for a in mid:
            c = c * shapes_x[ib, a] + pos_in[a][ie]
        out_bs = [np.asarray(leg.get_block_sizes(), dtype=np.int64) for leg in self.legs]
        o = np.zeros(len(ib), dtype=np.int64)
        for k in range(1, X.rank - 1):
            o = o * out_bs[k][self.qdata[blk, k]] + pos_out[perm[k]][ie]
        pre_y, post_y = out_bs[0][self.qdata[:, 0]], out_bs[-1][self.qdata[:, -1]]
        m_out = sizes // (pre_y * post_y)
        assert np.array_equal(pre_y * m_out * post_y, sizes)
        post_x = shapes_x[ib, -1]
        assert np.array_equal(shapes_x[ib, 0], pre_y[blk]) and np.array_equal(post_x, post_y[blk])
        m_in = sizes_x[ib] // (shapes_x[ib, 0] * post_x)
        assert np.all(c < m_in) and np.all(o < m_out[blk])
        # rows table: the terms of a destination row back to back, in the order of the pairs
        row_base = np.cumsum(m_out) - m_out
        row = row_base[blk] + o
        key = np.lexsort((np.arange(len(row)), row))
        n_rows = int(np.sum(m_out))
        counts = np.bincount(row, minlength=n_rows).astype(np.int64)
        rows = np.stack([np.cumsum(counts) - counts, counts], axis=1)
        terms = np.zeros((len(key), 4), dtype=np.int64)
        terms[:, 0] = X._offsets[ib[key]] + c[key] * post_x[key]
        terms[:, 1] = m_in[key] * post_x[key]
        _pack_alpha(terms, vals[ie[key]])
        # jobs: one per block of Y; with few blocks the rows of a block are split over several jobs (dst_ld = the whole block's rows)
        pieces = 1 if len(sizes) >= self.SPLIT_BELOW else -(-self.SPLIT_BELOW // len(sizes))
        per_job = np.maximum(1, -(-m_out // pieces))
        n_piece = -(-m_out // per_job)
        jb = np.repeat(np.arange(len(sizes)), n_piece)
        r0 = (np.arange(len(jb)) - np.repeat(np.cumsum(n_piece) - n_piece, n_piece)) * per_job[jb]
        jobs = np.zeros((len(jb), 8), dtype=np.int64)
        jobs[:, 0], jobs[:, 1], jobs[:, 2] = self.offsets[jb] + r0 * post_y[jb], pre_y[jb], np.minimum(per_job[jb], m_out[jb] - r0)
        jobs[:, 3], jobs[:, 4], jobs[:, 5] = post_y[jb], row_base[jb] + r0, m_out[jb] * post_y[jb]
        assert len(jobs) <= 60000 and int(np.sum(jobs[:, 1] * jobs[:, 2] * jobs[:, 3])) == self.total
        self.jobs_host, self.rows_host, self.terms_host, self.sizes = jobs, rows, terms, sizes
        self.jobs_dev, self.rows_dev, self.terms_dev = dev.to_device(jobs), dev.to_device(rows), dev.to_device(terms)
        self.n_jobs, self.max_cols = len(jobs), int(np.max(pre_y * post_y))
        self.x_key = X._struct_key()
        self.bytes = 8 * (2 if self.dtype.kind == 'c' else 1) * (self.total + int(np.sum(shapes_x[ib, 0] * post_x)))

    def _launch(self, X, res):
        dev.check(dev.lib().tpa_mpo_entry_apply_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.rows_dev.data_ptr(),
                                                      self.terms_dev.data_ptr(), self.max_cols, X._arena.data_ptr(), res._arena.data_ptr(),
                                                      dev.stream()), "mpo_entry_apply")

    def program_op(self, a_slot, c_slot):
        """The row of a ``tpa_lanczos_run`` program that applies this plan from slot ``a_slot`` into slot ``c_slot`` (kind 6)."""
        return [6, 0, self.jobs_dev.data_ptr(), self.rows_dev.data_ptr(), self.terms_dev.data_ptr(), self.n_jobs, a_slot, 0, c_slot,
                self.max_cols, 0, 0]


def _merged_w_leg(leg1, leg2):
    """The leg ``(w1, w2)`` of two MPO bond legs with the same ``qconj``: one block per pair of blocks, the first leg's block number the
    slow one, and inside a block the first leg's position the slow one -- which is how a block of a tensor with the neighbouring legs
    ``w1, w2`` lies in memory, so that merging them (``_with_w_legs``) moves no data."""
    from ..linalg.charges import LegCharge
    assert leg1.qconj == leg2.qconj
    chinfo = leg1.chinfo
    s1, s2 = np.asarray(leg1.get_block_sizes(), dtype=np.int64), np.asarray(leg2.get_block_sizes(), dtype=np.int64)
    slices = np.concatenate([[0], np.cumsum(np.outer(s1, s2).reshape(-1))])
    q1, q2 = np.asarray(leg1.charges).reshape(len(s1), -1), np.asarray(leg2.charges).reshape(len(s2), -1)
    charges = chinfo.make_valid((q1[:, None, :] + q2[None, :, :]).reshape(len(s1) * len(s2), -1))
    return LegCharge.from_qind(chinfo, slices, charges, leg1.qconj)


def _merged_w_index(leg1, leg2, merged, i1, i2):
    """The indices on ``merged = _merged_w_leg(leg1, leg2)`` of the index pairs ``(i1, i2)``."""
    (b1, p1), (b2, p2) = _leg_block_pos(leg1, i1), _leg_block_pos(leg2, i2)
    s2 = np.asarray(leg2.get_block_sizes(), dtype=np.int64)
    return np.asarray(merged.slices, dtype=np.int64)[b1 * leg2.block_number + b2] + p1 * s2[b2] + p2


def _array_from_entries(legs, labels, idx, vals, dtype, qtotal):
    """The Array with the entries ``vals`` at the global indices ``idx`` (int64[n, rank], no index twice) and nothing else stored:
    only the blocks that hold an entry exist -- nothing of the size of the dense tensor is formed."""
    where = [_leg_block_pos(leg, idx[:, a]) for a, leg in enumerate(legs)]
    uq, blk = _rank_rows(np.stack([b for b, _ in where], axis=1))
    res = npc.Array(legs, dtype, qtotal, labels)
    if len(idx) == 0:
        return res
    shapes = res._block_shapes(uq)
    sizes = np.prod(shapes, axis=1)
    offs = np.cumsum(sizes) - sizes
    pos = np.zeros(len(idx), dtype=np.int64)
    for a, (_, at) in enumerate(where):
        pos = pos * shapes[blk, a] + at
    flat = np.zeros(int(np.sum(sizes)), dtype=dtype)
    flat[offs[blk] + pos] = vals
    res._set_blocks(uq, arena=dev.to_device(flat), qdata_sorted=True)
    return res


def _with_w_legs(A, at, legs, labels):
    """``A`` with the MPO bond leg(s) that start at position ``at`` replaced by ``legs`` -- the two legs ``w1, w2`` by their merged leg
    (``_merged_w_leg``) or the merged leg by the two -- WITHOUT moving data: the blocks keep their places in the arena, only their
    numbers change."""
    n_old = 3 - len(legs)
    q = A._qdata
    if n_old == 2:
        mid = (q[:, at] * A.legs[at + 1].block_number + q[:, at + 1])[:, None]
    else:
        mid = np.stack(np.divmod(q[:, at], legs[1].block_number), axis=1)
    qdata = np.concatenate([q[:, :at], mid, q[:, at + n_old:]], axis=1)
    res = npc.Array(A.legs[:at] + list(legs) + A.legs[at + n_old:], A.dtype, A.qtotal, A._labels[:at] + list(labels) + A._labels[at + n_old:])
    order = np.lexsort(qdata.T)
    res._adopt_blocks(np.ascontiguousarray(qdata[order], dtype=np.intp), np.ascontiguousarray(A._offsets[order]), A._arena, True)
    return res


def _pair_tensors(W):
    """The host-multiplied tensors of the pair step of ``W`` (legs ``wL, wR, p, p*``), each an MPO tensor ``[wL, wR, p, p*]`` on merged
    bond legs ``(w1, w2)`` (cached on W like ``_tpa_entries``; the tables of the three plan families are then read from them):
    ``'prod'``: ``sum_p' W[w2, w2'][p'', p'] W[w1, w1'][p', p]``, the two layers of ``H^2`` in one tensor;
    ``'low'`` : ``W[w1, w1'] (x) 1[w2]``, layer 1 with the bond of layer 2 as a spectator; ``'up'``: ``1[w1'] (x) W[w2, w2']``, layer 2.
    All three come from the nonzero entries of W (``_mpo_coo``) -- the product by a sorted join over ``p'``, the way the ``W0 W1``
    tables are joined over their common bond -- and are stored entry by entry: the cost is the number of entries of the results
    (``nnz^2 / d`` and ``2 D nnz``), never the ``D^4`` of a dense tensor on the merged legs."""
    pair = getattr(W, '_tpa_pair', None)
    if pair is None:
        labels = ['wL', 'wR', 'p', 'p*']
        idx, vals = _mpo_coo(W)
        wl = list(W.get_leg_labels())
        a, b, s, t = (idx[:, wl.index(l)] for l in labels)
        wL, wR, p, pc = (W.get_leg(l) for l in labels)
        # layer 2 entry e2 on layer 1 entry e1: p' = p* of e2 = p of e1
        o1 = np.argsort(s, kind='stable')
        lo, hi = np.searchsorted(s[o1], t, side='left'), np.searchsorted(s[o1], t, side='right')
        e2 = np.repeat(np.arange(len(t)), hi - lo)
        e1 = o1[np.arange(len(e2)) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo) + np.repeat(lo, hi - lo)]
        n, c_in, c_out = len(vals), np.arange(wL.ind_len), np.arange(wR.ind_len)
        rep_in, rep_out = np.repeat(np.arange(n), len(c_in)), np.repeat(np.arange(n), len(c_out))
        # (w1, w2, w1', w2', p'', p, value), the legs of every bond pair, total charge in units of W's
        parts = dict(prod=((a[e1], a[e2], b[e1], b[e2], s[e2], t[e1], vals[e2] * vals[e1]), (wL, wL), (wR, wR), 2),
                     low=((a[rep_in], np.tile(c_in, n), b[rep_in], np.tile(c_in, n), s[rep_in], t[rep_in], vals[rep_in]),
                          (wL, wL), (wR, wL.conj()), 1),
                     up=((np.tile(c_out, n), a[rep_out], np.tile(c_out, n), b[rep_out], s[rep_out], t[rep_out], vals[rep_out]),
                         (wR.conj(), wL), (wR, wR), 1))
        pair = {}
        for name, ((w1, w2, w1o, w2o, po, pi, v), l_in, l_out, n_q) in parts.items():
            leg_in, leg_out = _merged_w_leg(*l_in), _merged_w_leg(*l_out)
            at = np.stack([_merged_w_index(*l_in, leg_in, w1, w2), _merged_w_index(*l_out, leg_out, w1o, w2o), po, pi], axis=1)
            uq, inv = np.unique(at, axis=0, return_inverse=True)         # equal indices are summed in a fixed order
            tot = np.zeros(len(uq), dtype=np.asarray(v).dtype)
            np.add.at(tot, inv.reshape(-1), v)
            pair[name] = _array_from_entries([leg_in, leg_out, p, pc], labels, uq[tot != 0], tot[tot != 0], W.dtype,
                                             W.chinfo.make_valid(n_q * W.qtotal))
        W._tpa_pair = pair
    return pair


class MpoPairPlan(_MpoStepPlan):
    """The MPO step of the second moment (``networks/moments.py``): both layers of ``H^2`` on one site,

        ``Y[vR*, p, wR1, wR2, vR] = sum_{w1, w2, p} C[(w1 -> w1'), (w2 -> w2'); p'', p] X[vR*, wR1, wR2, p, vR]``,
        ``C = sum_p' W[w2, w2'][p'', p'] W[w1, w1'][p', p]``

    with the physical leg of Y next to ``vR*`` (the GEMM that closes the site needs no transposed copy).  The bond legs ``wR1, wR2`` of X
    are neighbours, so X is -- without moving data -- a tensor ``[vR*, (w1.w2), p, vR]`` on their merged leg, and the step is the
    one-site step of the plan family that ``_mpo_plan_class`` selects for the MPO, applied to a host-multiplied tensor of
    ``_pair_tensors``: no kernel and no entry point of its own.  Two modes:

    * ``'product'``  one launch with the product table ``C``;
    * ``'two_pass'`` two launches, ``W (x) 1`` (layer 1, ``wR2`` a spectator) and ``1 (x) W`` (layer 2): fewer terms where the MPO bond
      is wide (about ``2 D nnz`` against ``nnz^2 / d``).

    ``two_pass=None`` takes the mode with fewer terms (``n_terms``; a tie goes to the single launch).  ``steps`` are the plans of the
    family, ``launches`` their number."""
    _cache = {}
    _table = staticmethod(_pair_tensors)
    X_LABELS = ('vR*', 'wR1', 'wR2', 'p', 'vR')
    Y_LABELS = ('vR*', 'p', 'wR1', 'wR2', 'vR')
    MAX_JOBS = 60000            # what the job tables of the three plan families take (one job per block of Y)
    # (blocks of X) x (terms of a table) per site that `modes_within_reach` accepts: the scalar and the block family match them as one
    # boolean matrix when a plan is built, 2.3 - 2.8 ns per cell (profiles/mpo_moments.txt: 9.8 s for the first `variance` call of an
    # L = 100 chain at D = 20, 46 s at D = 32, against 0.7 / 1.6 s of the reference's statements); 10^6 keeps the build of a site at
    # about 3 ms, what the Heisenberg chain (D = 5: 3 10^4 cells) pays several times over -- D up to about 8 for a spin chain
    MAX_MATCH = 10**6

    @staticmethod
    def family(W):
        """The plan class of the pair step of ``W``, ``None`` where there is no blockwise form (``_mpo_plan_class`` of every tensor of
        ``_pair_tensors``: the merged legs keep the widths' character, so this is the family of ``W`` itself)."""
        cls = _mpo_plan_class(W)
        if cls is None or any(_mpo_plan_class(T) is not cls for T in _pair_tensors(W).values()):
            return None
        return cls

    @classmethod
    def modes_within_reach(cls, W, n_blocks, two_pass=None):
        """The modes -- of both, or the one ``two_pass`` names -- whose plans can be built for an X of at most ``n_blocks`` blocks
        within ``MAX_MATCH``, from the entry counts of W alone (nothing is multiplied): the product table has
        ``sum_p' #(p* = p') #(p = p')`` terms, the two passes ``nnz D`` each.  The entry family joins sorted tables and has no such
        matrix."""
        modes = ['product', 'two_pass'] if two_pass is None else ['two_pass' if two_pass else 'product']
        if _mpo_plan_class(W) is MpoEntryApplyPlan:
            return modes
        idx, _ = _mpo_coo(W)
        wl = list(W.get_leg_labels())
        d = W.get_leg('p').ind_len
        n_in, n_out = (np.bincount(idx[:, wl.index(l)], minlength=d) for l in ('p*', 'p'))
        terms = {'product': int(np.sum(n_in * n_out)), 'two_pass': len(idx) * max(W.get_leg('wL').ind_len, W.get_leg('wR').ind_len)}
        return [m for m in modes if n_blocks * terms[m] <= cls.MAX_MATCH]

    @staticmethod
    def _one_step(cls, Xm, T, first):
        out = ('vR*', 'p', 'wR', 'vR') if first else ('vR*', 'wR', 'p', 'vR')
        return cls.get(Xm, T, 'wR', 'p', 'wL', 'wR', 'p', 'p*', out)

    def __init__(self, X, W, two_pass=None, W2=None):
        assert W2 is None and tuple(X.get_leg_labels()) == self.X_LABELS
        cls, pair = self.family(W), _pair_tensors(W)
        Xm = _with_w_legs(X, 1, [_merged_w_leg(X.legs[1], X.legs[2])], ['wR'])
        modes = {}          # (only the mode asked for, or both to compare them; what is worth building is the caller's question: `modes_within_reach`)
        for m in ['product', 'two_pass'] if two_pass is None else ['two_pass' if two_pass else 'product']:
            if m == 'product':
                modes[m] = [self._one_step(cls, Xm, pair['prod'], True)]
            else:
                low = self._one_step(cls, Xm, pair['low'], False)
                modes[m] = [low] if low.empty else [low, self._one_step(cls, low.apply(Xm, launch=False), pair['up'], True)]
        self.n_terms = {m: sum(0 if s.empty else len(s.terms_host) for s in steps) for m, steps in modes.items()}
        self.mode = min(modes, key=lambda m: (self.n_terms[m], m))          # (a tie goes to 'product', the single launch)
        self.steps = modes[self.mode]
        self.launches = len(self.steps)
        self.empty = any(s.empty for s in self.steps)
        self.dtype = np.result_type(X.dtype, W.dtype)
        self.x_key = X._struct_key()
        if self.empty:
            self.qtotal = X.chinfo.make_valid(X.qtotal + 2 * W.qtotal)
            wR = W.get_leg('wR')
            self.legs, self.labels = [X.legs[0], W.get_leg('p'), wR, wR, X.legs[4]], list(self.Y_LABELS)
            return
        Ym = self.steps[-1].apply(Xm, launch=False)             # (block structure only)
        wR = W.get_leg('wR')
        Y = _with_w_legs(Ym, 2, [wR, wR], ['wR1', 'wR2'])
        self.legs, self.labels, self.qtotal = Y.legs, list(Y.get_leg_labels()), Y.qtotal
        self.qdata, self.offsets, self.total = Y._qdata, Y._offsets, self.steps[-1].total
        self.bytes = sum(s.bytes for s in self.steps)

    def apply(self, X, launch=True):
        """Y as a new Array (the plans of ``steps`` read nothing of X but its arena)."""
        res = npc.Array(self.legs, self.dtype, self.qtotal, self.labels)
        if self.empty:
            return res
        T = X
        for step in self.steps:
            T = step.apply(T, launch=launch)
        res._adopt_blocks(self.qdata, self.offsets, T._arena, True)
        return res


class ExpandJobLimit(ValueError):
    """The expanded matrix has more cells than one ``tpa_mpo_expand_batch`` launch takes jobs."""


class MpoExpandPlan(_MpoStepPlan):
    """The matrix that the subspace expansion of single-site DMRG decomposes (reference ``SubspaceExpansion.mix_and_decompose_1site``,
    mps_common.py:2140-2164 and :2170-2194), written in ONE ``tpa_mpo_expand_batch`` launch from ``T1 = LP . theta`` (right move,
    legs ``vR*, wR, p0, vR``) or ``T1 = theta . RP`` (left move, legs ``vL, p0, wL, vL*``):

        right:  E[(vL.p0), (wR.vR)] = sum_{w, p*} mix[wR] W[w, wR, p0, p*] T1[vL, w, p*, vR]
        left :  E[(vL.wL), (p0.vR)] = sum_{w, p*} mix[wL] W[wL, w, p0, p*] T1[vL, p*, w, vR]

    entry by entry of W (``_mpo_coo``: every block structure of the MPO is served by the one form), straight into the charge blocks of
    the fused matrix: ``LHeff`` / ``RHeff``, the scaling pass and the ``combine_legs`` copy do not happen.  A job is one cell -- the
    slice of an incoming block pair of the row pipe times that of the column pipe -- of a stored charge block; a block is stored when
    one of its cells receives a term (whatever the weights: a sector that ``mix = 0`` wipes out holds zeros, as after the reference's
    ``iscale_axis``), every cell of a stored block is covered, and cells or rows without terms are written as zeros.

    ``move_right``: the direction.  ``zero``: bool per index of the outgoing MPO bond leg, True where the weight is exactly zero -- the
    terms of these rows are not read.  ``proj`` (with ``theta``, legs ``vL, p0, vR``): the stacked form of ``IdL`` / ``IdR`` = ``None``
    (:2146-2163 without the ``explicit_plus_hc`` part) -- the outgoing MPO leg is one trivial index, whose rows copy ``theta`` itself
    (the second source of the kernel), followed by the indices with ``proj`` True.  The weights are multiplied into the coefficients
    on the host when the plan is applied (one rounding each)."""
    _cache = {}
    _table = staticmethod(_mpo_coo)
    MAX_JOBS = 60000        # (the entry point takes 65535; the margin of the sibling plans)
    _P = ('p0', 'p0*')      # labels of the physical legs of W: the open one and the one contracted with T1
    _X_RIGHT = ['vR*', 'wR', 'p0', 'vR']        # labels of T1 moving right

    @classmethod
    def get(cls, X, W, move_right, zero, proj=None, theta=None, row_pipe=None):
        """Cached constructor: the plan depends on the block structure and the leg charges of ``X`` (and ``theta``), on the MPO tensor,
        the direction and the two masks."""
        t1 = cls._table(W)
        key = (X._struct_key(), str(X.dtype), id(t1), bool(move_right), np.asarray(zero, bool).tobytes(),
               None if proj is None else np.asarray(proj, bool).tobytes(), None if theta is None else theta._struct_key(),
               X.qtotal.tobytes(), tuple((l.charges.tobytes(), int(l.qconj)) for l in X.legs),
               None if row_pipe is None else row_pipe._content_key())
        plan = cls._cache.get(key)
        if plan is None or plan._tables_alive[0] is not t1:
            if len(cls._cache) > 4096:
                cls._cache.clear()
            plan = cls._cache[key] = cls(X, W, move_right, zero, proj, theta, row_pipe)
            plan._tables_alive = (t1, None)       # (the key holds its id(): see `_MpoStepPlan.get`)
        return plan

    def __init__(self, X, W, move_right, zero, proj=None, theta=None, row_pipe=None):
        from ..linalg.charges import LegCharge, LegPipe
        w_in, w_out = ('wL', 'wR') if move_right else ('wR', 'wL')
        p_out, p_in = self._P
        want = self._X_RIGHT if move_right else ['vL', 'p0', 'wL', 'vL*']
        assert list(X.get_leg_labels()) == want and list(W.get_leg_labels()) == ['wL', 'wR', p_out, p_in]
        ax_w, ax_p = (1, 2) if move_right else (2, 1)
        keys, vals = MpoEntryApplyPlan._entries(W, w_in, w_out, p_out, p_in)      # (w_in, w_out, p_out, p_in)
        wleg, pleg = W.get_leg(w_out), W.get_leg(p_out)
        zero = np.asarray(zero, bool)
        assert zero.shape == (wleg.ind_len,)
        w_new = keys[:, 1]
        self.stacked = proj is not None
        if self.stacked:       # the outgoing leg: [theta itself] + [the indices that survive the projection]
            proj = np.asarray(proj, bool)
            assert proj.shape == (wleg.ind_len,) and theta is not None and list(theta.get_leg_labels()) == ['vL', 'p0', 'vR']
            assert np.all(W.qtotal == 0), "the stacked form puts theta next to W . theta: they must carry the same charge"
            _, _, kept = wleg.project(proj)
            sizes = np.concatenate([[1], kept.get_block_sizes()])
            charges = np.concatenate([np.zeros((1, W.chinfo.qnumber), dtype=kept.charges.dtype), kept.charges], axis=0)
            wleg = LegCharge.from_qind(W.chinfo, np.append([0], np.cumsum(sizes)), charges, wleg.qconj)
            new_of_old = np.where(proj, np.cumsum(proj), -1)
            keep = new_of_old[keys[:, 1]] >= 0
            keys, vals = keys[keep], vals[keep]
            w_new = new_of_old[keys[:, 1]]
        self.dtype = np.result_type(X.dtype, W.dtype)
        self.qtotal = X.chinfo.make_valid(X.qtotal + W.qtotal)
        if move_right:
            self.row_pipe = row_pipe if row_pipe is not None else LegPipe([X.legs[0], pleg], qconj=+1)
            self.col_pipe = LegPipe([wleg, X.legs[3]], qconj=-1)
            self.labels = ['(vL.%s)' % p_out, '(wR.vR)']
        else:
            self.row_pipe = LegPipe([X.legs[0], wleg], qconj=+1)
            self.col_pipe = row_pipe if row_pipe is not None else LegPipe([pleg, X.legs[3]], qconj=-1)     # (the given pipe of theta)
            self.labels = ['(vL.wL)', '(p0.vR)']
        self.legs = [self.row_pipe, self.col_pipe]
        self.w_leg = wleg
        # ---- all (block of T1, entry of W) pairs: the join of `MpoEntryApplyPlan`
        xq = X._qdata
        b_in, pos_in = {}, {}
        b_in[ax_w], pos_in[ax_w] = _leg_block_pos(X.legs[ax_w], keys[:, 0])
        b_in[ax_p], pos_in[ax_p] = _leg_block_pos(X.legs[ax_p], keys[:, 3])
        ib, ie = _join_entries_blocks(X, [1, 2], b_in, len(keys))
        bw, pw = _leg_block_pos(wleg, w_new)
        bp, pp = _leg_block_pos(pleg, keys[:, 2])
        shapes_x = X._block_shapes()
        post_x = shapes_x[ib, 3]
        # per pair: blocks and positions on the four legs of the result, the source row, the value and the (old) outgoing index
        pr = dict(v0=xq[ib, 0], v1=xq[ib, 3], bw=bw[ie], pw=pw[ie], bp=bp[ie], pp=pp[ie],
                  off=X._offsets[ib] + (pos_in[1][ie] * shapes_x[ib, 2] + pos_in[2][ie]) * post_x,
                  ld=shapes_x[ib, 1] * shapes_x[ib, 2] * post_x, val=vals[ie].astype(np.complex128), w=keys[ie, 1],
                  sel=np.zeros(len(ib), np.int64), blk=ib)
        if self.stacked and theta.stored_blocks:       # the rows of theta: one term each, alpha = 1, read from the second source
            tq, ts = theta._qdata, theta._block_shapes()
            tb = np.repeat(np.arange(len(tq)), ts[:, 1])
            tp = np.arange(len(tb)) - np.repeat(np.cumsum(ts[:, 1]) - ts[:, 1], ts[:, 1])
            z = np.zeros(len(tb), np.int64)
            th = dict(v0=tq[tb, 0], v1=tq[tb, 2], bw=z, pw=z, bp=tq[tb, 1], pp=tp, off=theta._offsets[tb] + tp * ts[tb, 2],
                      ld=ts[tb, 1] * ts[tb, 2], val=np.ones(len(tb), np.complex128), w=z - 1, sel=z + 1, blk=tb)
            pr = {k: np.concatenate([pr[k], th[k]]) for k in pr}
            self.theta_key = theta._struct_key()
        self.empty = len(pr['off']) == 0
        if self.empty:
            return
        # ---- cells and charge blocks
        qr, qc = self.row_pipe.q_map, self.col_pipe.q_map
        if move_right:      # rows (vL, p0), columns (wR, vR)
            rc = self.row_pipe._map_incoming_qind(np.stack([pr['v0'], pr['bp']], axis=1))
            cc = self.col_pipe._map_incoming_qind(np.stack([pr['bw'], pr['v1']], axis=1))
            pos_r, pos_c = pr['pp'], pr['pw']
        else:               # rows (vL, wL), columns (p0, vR)
            rc = self.row_pipe._map_incoming_qind(np.stack([pr['v0'], pr['bw']], axis=1))
            cc = self.col_pipe._map_incoming_qind(np.stack([pr['bp'], pr['v1']], axis=1))
            pos_r, pos_c = pr['pw'], pr['pp']
        blk, sizes = self._rank_blocks(np.stack([qr[rc, 2], qc[cc, 2]], axis=1))
        ld_blk = self.col_pipe.get_block_sizes()[self.qdata[:, 1]]
        # one job per cell of a stored block
        jk, jr, jc = [], [], []
        for k, (Qr, Qc) in enumerate(self.qdata.tolist()):
            r_cells, c_cells = np.nonzero(qr[:, 2] == Qr)[0], np.nonzero(qc[:, 2] == Qc)[0]
            jk.append(np.full(len(r_cells) * len(c_cells), k))
            jr.append(np.repeat(r_cells, len(c_cells)))
            jc.append(np.tile(c_cells, len(r_cells)))
        jk, jr, jc = np.concatenate(jk), np.concatenate(jr), np.concatenate(jc)
        bs_r = [np.asarray(l.get_block_sizes(), dtype=np.int64) for l in self.row_pipe.legs]
        bs_c = [np.asarray(l.get_block_sizes(), dtype=np.int64) for l in self.col_pipe.legs]
        pre, n_r = bs_r[0][qr[jr, 3]], bs_r[1][qr[jr, 4]]
        n_c, post = bs_c[0][qc[jc, 3]], bs_c[1][qc[jc, 4]]
        ld = ld_blk[jk]
        n_rows = n_r * n_c
        row_begin = np.cumsum(n_rows) - n_rows
        jobs = np.zeros((len(jk), 8), dtype=np.int64)
        jobs[:, 0], jobs[:, 1], jobs[:, 2], jobs[:, 3] = self.offsets[jk] + qr[jr, 0] * ld, pre, n_rows, post
        jobs[:, 4], jobs[:, 5] = row_begin, n_r * ld
        if len(jobs) > self.MAX_JOBS:       # (one job per blockIdx.y; the caller takes the generic route)
            raise ExpandJobLimit("%d cells for one tpa_mpo_expand_batch launch" % len(jobs))
        assert int(np.sum(pre * n_rows * post)) == self.total
        # rows of a job: (position on the inner leg of the row pipe, position on the outer leg of the column pipe)
        rj = np.repeat(np.arange(len(jk)), n_rows)
        ro = np.arange(len(rj)) - row_begin[rj]
        rows = np.zeros((len(rj), 4), dtype=np.int64)
        rows[:, 2] = (ro // n_c[rj]) * ld[rj] + qc[jc[rj], 0] + (ro % n_c[rj]) * post[rj]
        # the job of every pair, then its row; terms grouped by row, in the order of the pairs
        n_cc = len(qc)
        cell_key = jr * n_cc + jc
        order = np.argsort(cell_key)
        job_of = order[np.searchsorted(cell_key[order], rc * n_cc + cc)]
        assert np.array_equal(cell_key[job_of], rc * n_cc + cc) and np.array_equal(jk[job_of], blk)
        assert np.array_equal(pre[job_of[:len(ib)]], shapes_x[ib, 0]) and np.array_equal(post[job_of[:len(ib)]], post_x)
        row = row_begin[job_of] + pos_r * n_c[job_of] + pos_c
        rows[row, 3] = pr['sel']
        live = ~zero[np.maximum(pr['w'], 0)] | (pr['w'] < 0)        # (rows of a zero weight: no terms, zeros are written)
        key = np.lexsort((np.arange(len(row)), row))
        key = key[live[key]]
        counts = np.bincount(row[key], minlength=len(rows)).astype(np.int64)
        rows[:, 0], rows[:, 1] = np.cumsum(counts) - counts, counts
        assert np.all(counts[rows[:, 3] == 1] == 1), "a row of theta has exactly one term"
        terms = np.zeros((max(len(key), 1), 4), dtype=np.int64)
        terms[:len(key), 0], terms[:len(key), 1] = pr['off'][key], pr['ld'][key]
        self.term_val, self.term_w = pr['val'][key], pr['w'][key]
        self.term_blk, self.term_row = pr['blk'][key], row[key]       # (block of the source and row of every term: the cell-dense form)
        if self.dtype.kind != 'c':
            assert np.all(self.term_val.imag == 0)
        self.jobs_host, self.rows_host, self.terms_host, self.sizes = jobs, rows, terms, sizes
        self.jobs_dev, self.rows_dev = dev.to_device(jobs), dev.to_device(rows)
        self.terms_dev = self._mix_host = None
        self.n_jobs, self.max_cols = len(jobs), int(np.max(pre * post))
        self.x_key = X._struct_key()
        cols_t = (pre * post)[job_of[key]]
        self.bytes = 8 * (2 if self.dtype.kind == 'c' else 1) * int(np.sum(cols_t) + np.sum((pre * post)[rj]))
        self.flops = (8 if self.dtype.kind == 'c' else 2) * int(np.sum(cols_t))

    def _set_weights(self, mix):
        """alpha = fl(mix[outgoing index] * W entry), 1 for the rows of theta; uploaded once per bond and amplitude."""
        mix = np.ascontiguousarray(mix, np.float64)
        if self._mix_host is None or not np.array_equal(self._mix_host, mix):
            alpha = np.where(self.term_w >= 0, mix[np.maximum(self.term_w, 0)] * self.term_val, self.term_val)
            _pack_alpha(self.terms_host[:len(alpha)], alpha)
            self.terms_dev, self._mix_host = dev.to_device(self.terms_host), mix.copy()

    def apply(self, X, mix, theta=None):
        """The expanded matrix as a new Array.  ``mix``: the real weight of every index of the outgoing MPO bond leg of W (the stacked
        form reads it at the indices it keeps)."""
        res = npc.Array(self.legs, self.dtype, self.qtotal, self.labels)
        if self.empty:
            return res
        assert X._struct_key() == self.x_key and X.dtype == self.dtype
        src2 = None
        if self.stacked:
            assert theta is not None and theta.dtype == self.dtype and theta._struct_key() == self.theta_key
            src2 = theta._arena.data_ptr()
        self._set_weights(mix)
        res._set_blocks(self.qdata, arena=dev.empty(self.total, self.dtype), qdata_sorted=True)
        dev.check(dev.lib().tpa_mpo_expand_batch(dev.code(self.dtype), self.jobs_dev.data_ptr(), self.n_jobs, self.rows_dev.data_ptr(),
                                                 self.terms_dev.data_ptr(), self.max_cols, X._arena.data_ptr(), src2,
                                                 res._arena.data_ptr(), dev.stream()), "mpo_expand")
        return res


# ---------------------------------------------------------------------------------------------------------------------
# Zip-up application of an MPO to an MPS (reference ``MPO.apply_zipup``, mpo.py:1679-1767).  At an interior site the reference decomposes
#     M[(vL.p), (wR.vR)] = sum_{w, p*} W[w, wR, p, p*] T1[vL, w, p*, vR],      T1 = VH_prev[vL, w, vR'] . B[vR', p*, vR]
# and gets it as tensordot(B, W) -- an intermediate of chi^2 D^2 d elements --, a tensordot over (w, vR') and ``combine_legs``.  It is the
# matrix of ``MpoExpandPlan`` moving right with ``VH_prev`` in the place of ``LP`` and all weights 1: one GEMM over chi and the MPO step.
# Time-evolution MPOs (U_I, U_II) are dense in the bond index: the rows of a cell share their source rows, and the cell-dense form
# (``tpa_mpo_cell_apply_batch``) loads each of them once.
from .._lib import MPO_CELL_MAXROWS    # noqa: E402  (TPA_MPO_CELL_MAXROWS)
# Which cells of a zip-up step take the cell-dense launch: 0 = none (the entry-by-entry launch of the subspace expansion alone), 1 = the
# cells ``MpoZipupPlan._cell_rule`` selects, 2 = every cell with a source.  The default follows profiles/mpo_zipup.txt: the forced
# cell-dense route is slower than the entry launch on the 4-wide nearest-neighbour structure, so it is 0.
MPO_CELL_DEFAULT = '0'


def mpo_cell_mode():
    return int(_os.environ.get('TPA_MPO_CELL', MPO_CELL_DEFAULT))


zipup_stats = {'device_steps': 0, 'declined': 0, 'why': {}, 'plans_built': 0, 'cell_launches': 0, 'entry_launches': 0}


def reset_zipup_stats():
    zipup_stats.update(device_steps=0, declined=0, why={}, plans_built=0, cell_launches=0, entry_launches=0)


class _ZipupRoute:
    """The launches of one ``MpoZipupPlan`` under one setting of ``TPA_MPO_CELL``: the jobs of the cell-dense launch and the jobs left to
    the entry-by-entry launch (disjoint destinations)."""

    def __init__(self, plan, cell):
        piece_cell = cell[plan.piece_job]
        cj, ej = plan.cell_jobs_host[piece_cell], plan.jobs_host[~cell]
        if len(cj) > plan.MAX_JOBS:
            raise ExpandJobLimit("%d jobs for one tpa_mpo_cell_apply_batch launch" % len(cj))
        if len(ej) > plan.MAX_JOBS:
            raise ExpandJobLimit("%d jobs for one tpa_mpo_expand_batch launch" % len(ej))
        self.n_cell, self.n_entry = len(cj), len(ej)
        self.cell_jobs_dev = dev.to_device(cj) if len(cj) else None
        self.entry_jobs_dev = (plan.jobs_dev if len(ej) == len(plan.jobs_host) else dev.to_device(ej)) if len(ej) else None
        self.max_rows = int(np.max(cj[:, 2])) if len(cj) else 0
        self.cell_cols = int(np.max(cj[:, 1] * cj[:, 3])) if len(cj) else 0
        self.entry_cols = int(np.max(ej[:, 1] * ej[:, 3])) if len(ej) else 0


class MpoZipupPlan(MpoExpandPlan):
    """``MpoExpandPlan`` moving right for the zip-up step -- ``X = T1 [vL, wR, p, vR]``, ``W [wL, wR, p, p*]``, all weights 1, result
    ``[(vL.p), (wR.vR)]`` with the pipes of the reference's ``combine_legs`` -- with a CELL-DENSE table form next to the entry tables:
    per cell the distinct source rows (ordered by block of T1 and position inside it: the order in which every row of the entry tables
    lists them, ``ordered``) and the ``n_rows x n_src`` coefficient matrix, zero where W has no entry, for
    ``tpa_mpo_cell_apply_batch``.  Cells with more than ``TPA_MPO_CELL_MAXROWS`` rows are split into jobs over the same source list.
    ``apply`` sends every cell to one of at most two launches (``TPA_MPO_CELL``); both sum the same chain of fused multiply-adds, so the
    choice does not change a bit of the result (a plan that is not ``ordered`` keeps to the entry launch)."""
    _cache = {}
    MAX_JOBS = 60000
    _P = ('p', 'p*')
    _X_RIGHT = ['vL', 'wR', 'p', 'vR']

    @classmethod
    def get(cls, X, W, row_pipe=None):
        return super().get(X, W, True, np.zeros(W.get_leg('wR').ind_len, bool), None, None, row_pipe)

    def __init__(self, X, W, move_right, zero, proj=None, theta=None, row_pipe=None):
        assert move_right and proj is None and not np.any(zero)
        super().__init__(X, W, True, zero, None, None, row_pipe)
        self._routes = {}
        if self.empty:
            return
        jobs, nt = self.jobs_host, len(self.term_val)
        n_rows, row_begin = jobs[:, 2], jobs[:, 4]
        t_row = self.term_row
        t_job = np.repeat(np.arange(len(jobs)), n_rows)[t_row]
        # the distinct sources of every cell, by (block of T1, offset)
        uq, inv = np.unique(np.stack([t_job, self.term_blk, self.terms_host[:nt, 0]], axis=1), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        n_src = np.bincount(uq[:, 0], minlength=len(jobs)).astype(np.int64)
        src_begin = np.cumsum(n_src) - n_src
        k = inv - src_begin[t_job]
        srcs = np.zeros((max(len(uq), 1), 2), dtype=np.int64)
        srcs[:len(uq), 0] = uq[:, 2]
        srcs[inv, 1] = self.terms_host[:nt, 1]
        same = t_row[1:] == t_row[:-1]
        self.ordered = bool(np.all(k[1:][same] > k[:-1][same]))      # every row lists its sources in the order of the cell
        # jobs of at most MPO_CELL_MAXROWS rows
        n_piece = -(-n_rows // MPO_CELL_MAXROWS)
        pj = np.repeat(np.arange(len(jobs)), n_piece)
        piece_begin = np.cumsum(n_piece) - n_piece
        r0 = (np.arange(len(pj)) - piece_begin[pj]) * MPO_CELL_MAXROWS
        p_rows = np.minimum(MPO_CELL_MAXROWS, n_rows[pj] - r0)
        c_size = p_rows * n_src[pj]
        c_off = np.cumsum(c_size) - c_size
        cj = np.zeros((len(pj), 10), dtype=np.int64)
        cj[:, 0], cj[:, 1], cj[:, 2], cj[:, 3], cj[:, 4] = jobs[pj, 0], jobs[pj, 1], p_rows, jobs[pj, 3], jobs[pj, 5]
        cj[:, 5], cj[:, 6], cj[:, 7], cj[:, 8] = row_begin[pj] + r0, src_begin[pj], n_src[pj], c_off
        o = t_row - row_begin[t_job]
        piece = piece_begin[t_job] + o // MPO_CELL_MAXROWS
        coeff = np.zeros(max(int(np.sum(c_size)), 1), dtype=self.dtype)
        val = self.term_val if self.dtype.kind == 'c' else self.term_val.real
        at = c_off[piece] + k * p_rows[piece] + o % MPO_CELL_MAXROWS
        assert len(np.unique(at)) == len(at), "a row lists one source twice"      # (an entry of W per (row, source): nothing to add up)
        coeff[at] = val
        self.cell_jobs_host, self.piece_job, self.srcs_host, self.coeff_host = cj, pj, srcs, coeff
        self.cell_n_src, self.cell_nnz = n_src, np.bincount(t_job, minlength=len(jobs)).astype(np.int64)
        self.cell_rows_dev = dev.to_device(np.ascontiguousarray(np.stack([self.rows_host[:, 2], np.zeros(len(self.rows_host), np.int64)], axis=1)))
        self.srcs_dev, self.coeff_dev = dev.to_device(srcs), dev.to_device(coeff)
        cols = jobs[:, 1] * jobs[:, 3]
        item = 8 * (2 if self.dtype.kind == 'c' else 1)
        self.cell_bytes = item * int(np.sum(cols * (n_src + n_rows)))      # every cell by the cell-dense launch

    @staticmethod
    def _cell_rule(n_src, n_rows, nnz):
        """The cells that the cell-dense launch takes under ``TPA_MPO_CELL=1``: the entry tables load ``nnz`` source rows per column
        item of the cell, the cell-dense form ``n_src`` -- it takes the cells where that halves the loads at least AND that have 6
        rows or more.  Measured (profiles/mpo_zipup.txt, chi = 1024, complex and real): cells of 6 and 12 rows over 9 and 18 sources
        run 2.2 to 2.6 times faster in the cell-dense form, cells of 12 and 24 rows over 18 and 36 sources (one launch on the
        32-accumulator kernel: the largest job of a launch selects it for all of them) 2.1 to 3 times; cells of 1 and 2 rows over at
        most 3 sources are served from the caches either way and the entry form is up to 10 % faster there.  Not measured: cells of 3
        to 5 rows (they stay where they were), and a launch that mixes a few cells above 16 rows with many small ones, which all run
        with 32 accumulators then."""
        return (n_src >= 1) & (n_rows >= 6) & (nnz >= 2 * n_src)

    def route(self, mode):
        r = self._routes.get(mode)
        if r is None:
            if mode == 0 or not self.ordered:      # (out of order the two launches would sum differently: the entry launch alone)
                cell = np.zeros(len(self.jobs_host), bool)
            elif mode == 2:
                cell = self.cell_n_src >= 1
            else:
                cell = self._cell_rule(self.cell_n_src, self.jobs_host[:, 2], self.cell_nnz)
            r = self._routes[mode] = _ZipupRoute(self, cell)
        return r

    def apply(self, X, mode=None):
        """M as a new Array: at most one cell-dense and one entry-by-entry launch (``mode``: ``TPA_MPO_CELL``)."""
        res = npc.Array(self.legs, self.dtype, self.qtotal, self.labels)
        if self.empty:
            return res
        assert X._struct_key() == self.x_key and X.dtype == self.dtype
        r = self.route(mpo_cell_mode() if mode is None else mode)
        res._set_blocks(self.qdata, arena=dev.empty(self.total, self.dtype), qdata_sorted=True)
        code, L = dev.code(self.dtype), dev.lib()
        if r.n_entry:
            self._set_weights(np.ones(self.w_leg.ind_len))
            dev.check(L.tpa_mpo_expand_batch(code, r.entry_jobs_dev.data_ptr(), r.n_entry, self.rows_dev.data_ptr(),
                                             self.terms_dev.data_ptr(), r.entry_cols, X._arena.data_ptr(), None,
                                             res._arena.data_ptr(), dev.stream()), "mpo_expand")
            zipup_stats['entry_launches'] += 1
        if r.n_cell:
            dev.check(L.tpa_mpo_cell_apply_batch(code, r.cell_jobs_dev.data_ptr(), r.n_cell, self.cell_rows_dev.data_ptr(),
                                                 self.srcs_dev.data_ptr(), self.coeff_dev.data_ptr(), r.max_rows, r.cell_cols,
                                                 X._arena.data_ptr(), res._arena.data_ptr(), dev.stream()), "mpo_cell")
            zipup_stats['cell_launches'] += 1
        return res


def zipup_enabled():
    return _os.environ.get('TPA_ZIPUP_DEVICE', '1') != '0'


def _zipup_declines(VH_prev, B, W, explicit_plus_hc, finite):
    """Why the device route of the zip-up step does not take this call (counted in ``zipup_stats['why']``), or ``None``."""
    if not zipup_enabled():
        return 'switched off'
    if explicit_plus_hc:
        return 'explicit_plus_hc'
    if not finite:
        return 'not finite'
    if not (dev.lib_provides('tpa_mpo_expand_batch') and dev.lib_provides('tpa_mpo_cell_apply_batch')):
        return 'entry point'      # an emulation that predates the entry points: never forwarded to the real library
    if VH_prev.stored_blocks == 0 or B.stored_blocks == 0 or W.stored_blocks == 0:
        return 'empty tensor'
    return None


def _zipup_decline(why):
    zipup_stats['declined'] += 1
    zipup_stats['why'][why] = zipup_stats['why'].get(why, 0) + 1


def device_zipup_step(VH_prev, B, W, explicit_plus_hc=False, finite=True):
    """The matrix that an interior step of ``MPO.apply_zipup`` hands to ``svd_theta`` (reference mpo.py:1733, :1756-1757), labels
    ``['(vL.p)', '(wR.vR)']`` with the pipes ``combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1])`` builds, so that the
    reference's ``U.split_legs()`` / ``VH.split_legs()`` work on the factors; or ``None`` where the route declines
    (``_zipup_declines``, too many jobs) and the caller runs the generic statements.  ``VH_prev``: ``[vL, wR, vR]`` (the split ``VH`` of
    the step before, scaled with S), ``B``: ``[vL, p, vR]``, ``W``: ``[wL, wR, p, p*]``.  One GEMM over chi (``T1 = VH_prev . B``, the
    plan cache of ``tensordot``) and the MPO step of ``MpoZipupPlan``; operands are converted to ``result_type(B, W)`` first (a real
    MPS meets a complex U on the first step)."""
    why = _zipup_declines(VH_prev, B, W, explicit_plus_hc, finite)
    if why is not None:
        _zipup_decline(why)
        return None
    dtype = np.result_type(VH_prev.dtype, B.dtype, W.dtype)
    VH_prev, B = (t if t.dtype == dtype else t.astype(dtype) for t in (VH_prev, B))
    if list(VH_prev.get_leg_labels()) != ['vL', 'wR', 'vR']:
        VH_prev = VH_prev.transpose(['vL', 'wR', 'vR'])
    if list(B.get_leg_labels()) != ['vL', 'p', 'vR']:
        B = B.transpose(['vL', 'p', 'vR'])
    if list(W.get_leg_labels()) != ['wL', 'wR', 'p', 'p*']:
        W = W.transpose(['wL', 'wR', 'p', 'p*'])
    T1 = npc.tensordot(VH_prev, B, axes=['vR', 'vL'])        # vL, wR, p, vR
    if T1.stored_blocks == 0:
        _zipup_decline('empty tensor')
        return None
    try:
        plan = MpoZipupPlan.get(T1, W)
        if plan.empty:
            _zipup_decline('empty tensor')
            return None
        if getattr(plan, '_counted', None) is None:
            zipup_stats['plans_built'] += 1
            plan._counted = True
        M = plan.apply(T1)
    except ExpandJobLimit:
        _zipup_decline('too many jobs')
        return None
    zipup_stats['device_steps'] += 1
    return M


def _envs_wide(LP, RP):
    """Whether an MPO bond leg of the environments has a block wider than 1."""
    return not (bool(np.all(LP.get_leg('wR').get_block_sizes() == 1)) and bool(np.all(RP.get_leg('wL').get_block_sizes() == 1)))


def _envs_factorable(LP, RP):
    """LP / RP as the factored forms contract them: the standard labels with the bra leg of LP before its ket leg and the ket leg of
    RP before its bra leg; MPO bond legs resolved into 1-wide blocks, or -- where the entry-by-entry MPO step is available
    (``_entry_route``) -- of any widths (``_env_form`` then makes one transposed copy unless the stored order is the standard one)."""
    lp, rp = list(LP.get_leg_labels()), list(RP.get_leg_labels())
    return (sorted(lp) == sorted(['vR*', 'wR', 'vR']) and lp.index('vR*') < lp.index('vR') and
            sorted(rp) == sorted(['wL', 'vL', 'vL*']) and rp.index('vL') < rp.index('vL*') and
            (not _envs_wide(LP, RP) or _entry_route(LP.chinfo)))


def _env_form(A, labels):
    """The environment tensor ``A`` with its legs in the order ``labels``: itself, a view when only 1-wide legs move
    (``_relabel_view``), else -- a wide MPO bond leg has to move -- one transposed copy."""
    if list(A.get_leg_labels()) == list(labels):
        return A
    w = 'wR' if 'wR' in labels else 'wL'
    if np.all(A.get_leg(w).get_block_sizes() == 1):
        return _relabel_view(A, labels)
    return A.transpose(labels)


def _factored_plan_class(LP, RP, W, W2=None):
    """The plan class of the MPO step (``_mpo_plan_class``) if the factored forms can run on these environments, else ``None``:
    the one acceptance rule of the stand-alone classes and of the module-form dispatch.  Environments with wide MPO bond blocks
    need the entry-by-entry step (the two older plans move a 1-wide MPO leg only)."""
    if not _envs_factorable(LP, RP):
        return None
    cls = _mpo_plan_class(W, W2)
    if cls is not MpoEntryApplyPlan and _envs_wide(LP, RP):
        return None
    return cls


def factored_matvec_possible(LP, RP, W0, W1):
    """Whether ``LP . theta . (W0 W1) . RP`` can run as GEMM / block linear combination / GEMM on the tensors as they are stored:
    every MPO block a single number -- or a small matrix on the physical index between 1-wide MPO bond blocks (``_mpo_plan_class``) --,
    MPO bond legs of the environments resolved into 1-wide blocks, leg orders that need no transposed copy.  ``W0`` / ``W1`` with
    labels ``p`` or ``p0`` / ``p1``."""
    w0, w1 = list(W0.get_leg_labels()), list(W1.get_leg_labels())
    return (_factored_plan_class(LP, RP, W0, W1) is not None and
            w0 in (['wL', 'wR', 'p0', 'p0*'], ['wL', 'wR', 'p', 'p*']) and w1 in (['wL', 'wR', 'p1', 'p1*'], ['wL', 'wR', 'p', 'p*']))


class _Program:
    """A launch program for ``tpa_lanczos_run`` (include/tenpy_amd.h) while it is put together: ``ops``, the rows ``(kind, cfg, p0, p1, p2,
    count, a_slot, b_slot, c_slot, max_elems, 0, 0)``, and ``bufs``, the device tensors that the non-negative slots number (operands
    first, then temporaries from the scratch pool, in the order they are asked for); slot -1 = input vector, -2 = output vector.
    Apart from ``program_op`` of the MPO-step plans nothing else writes a row."""

    def __init__(self, *operands):
        self.bufs = list(operands)
        self.ops = []

    def scratch(self, name, n, dtype):
        """The slot of a new temporary, the arena ``name`` of the scratch pool."""
        self.bufs.append(dev.scratch(name, n, dtype))
        return len(self.bufs) - 1

    def gemm(self, plan, a, b, c, scratch_name, tiles=None, links=None, jobs=None, a2=None, alphas=None):
        """One planned contraction: the grouped GEMM, or -- split-K plans, ``npc._split_k`` -- the GEMM of the partial blocks into a
        scratch arena followed by their reduction into ``c`` (cfg = 1: timed together with the GEMM it completes).  In place of the
        plan's own: ``tiles`` (fewer tiles), ``links``, ``jobs`` (the reduction of fewer blocks); with ``a2`` (a slot) and ``alphas``
        the GEMM is kind 7, ``tpa_gemm_chain_ex``."""
        sk = plan.sk
        t = plan if sk is None else sk
        tiles, n_tiles = (t.tiles_dev, t.n_tiles) if tiles is None else (tiles, len(tiles))
        out = c if sk is None else self.scratch(scratch_name, sk.total, plan.dtype)
        self.ops.append([0 if a2 is None else 7, plan.cfg, t.tasks_dev.data_ptr(), (t.links_dev if links is None else links).data_ptr(),
                         tiles.data_ptr(), n_tiles, a, b, out, 0 if a2 is None else a2, 0 if a2 is None else alphas.data_ptr(), 0])
        if sk is not None:
            jobs, n_jobs = (sk.jobs_dev, sk.n_jobs) if jobs is None else (jobs, len(jobs))
            self.lincomb(jobs, n_jobs, sk.terms_dev, sk.max_elems, out, c, cfg=1)

    def lincomb(self, jobs, n_jobs, terms, max_elems, a, c, cfg=0):
        self.ops.append([1, cfg, jobs.data_ptr(), terms.data_ptr(), 0, n_jobs, a, 0, c, max_elems, 0, 0])

    def mpo_step(self, plan, a, c):
        self.ops.append(plan.program_op(a, c))

    def copy(self, jobs, n_jobs, max_elems, a, c):
        self.ops.append([2, 0, jobs.data_ptr(), 0, 0, n_jobs, a, 0, c, max_elems, 0, 0])

    def collective(self, a, c):
        self.ops.append([3, 0, 0, 0, 0, 0, a, 0, c, 0, 0, 0])

    def finish(self, gemm_plans, collective=None):
        """``(ops, bufs, gemm_plans[, collective])``: what ``krylov_based._native_krylov`` takes."""
        res = (np.array(self.ops, dtype=np.int64), self.bufs, gemm_plans)
        return res if collective is None else res + (collective,)


# The labels of an MPO step -- x_w, x_p, w_in, w_out, p_out, p_in of ``MpoApplyPlan`` -- going left to right (W0 on the legs wR, p0 of
# X = LP . theta, wL -> wR) and going right to left (W1 on the legs wL, p1 of X = theta . RP, wR -> wL: ``update_RP``, the right mixer).
_STEP_LR = ('wR', 'p0', 'wL', 'wR', 'p0', 'p0*')
_STEP_RL = ('wL', 'p1', 'wR', 'wL', 'p1', 'p1*')


def _mpo_step_lr(X, W0, W1=None, *, out_labels):
    """The cached plan (``_mpo_plan_class``) that applies W0 -- with ``W1``: W0 W1 on the legs wR, p0, p1 in ONE pass -- to X from left
    to right, giving Y with the legs ``out_labels``."""
    two = {} if W1 is None else dict(W2=W1, x_p2='p1', p2_out='p1', p2_in='p1*')
    return _mpo_plan_class(W0, W1).get(X, W0, *_STEP_LR, tuple(out_labels), **two)


def _mpo_step_rl(X, W1, *, out_labels):
    """The cached plan that applies W1 to X from right to left."""
    return _mpo_plan_class(W1).get(X, W1, *_STEP_RL, tuple(out_labels))


def _factored_plans(LPf, RPf, theta, W0, W1=None, launch=False, old=None):
    """The plans of the factored forms as the dict that an operator keeps in ``_fplans`` and the drivers hand from visit to visit of a
    bond: ``p1`` (``LPf . theta``, GEMM), the MPO step (``a01`` for W0 W1, ``a0`` for W0 alone, ``None`` without a site), ``p2``
    (``. RPf``, GEMM chained over wR and the bond sector) and what they were made for: the structure keys ``key`` (theta), ``lkey``,
    ``rkey`` and ``dtype``.  Returns ``(plans, T1, T)``: ``old`` itself and no tensors if it was made for the same structures (the
    environments grow between visits), else new plans with the results of step 1 and of the MPO step.  ``launch``: these two steps
    run while the plans are built (``plans['p2'].apply(T, RPf)`` completes the matvec), a step that needs a transposed copy is an
    assertion failure and an empty step gives empty plans.  Without it nothing is launched (T1, T: block structure only), and a
    transposed copy or an empty step means that there are no plans: ``(None, None, None)``."""
    keys = dict(key=theta._struct_key(), dtype=theta.dtype, lkey=LPf._struct_key(), rkey=RPf._struct_key())
    if old is not None and all(old[k] == v for k, v in keys.items()):
        return old, None, None
    p1, l_use, t_use = npc.plan_tensordot(LPf, theta, axes=['vR', 'vL'])
    fits = l_use is LPf and t_use is theta
    assert fits or not launch, "factored matvec step 1 must not need a transpose"
    if not fits or (p1.empty and not launch):
        return None, None, None
    T = T1 = p1.apply(LPf, theta, launch=launch)                   # vR*, wR, [p0, [p1,]] vR
    a = None
    if W0 is not None:
        a = _mpo_step_lr(T1, W0, W1, out_labels=('vR*', 'p0', 'wR', 'vR') if W1 is None else ('vR*', 'p0', 'p1', 'wR', 'vR'))
        if a.empty and not launch:
            return None, None, None
        T = a.apply(T1, launch=launch)                             # vR*, p0, [p1,] wR, vR
    p2, t_use, r_use = npc.plan_tensordot(T, RPf, axes=(['wR', 'vR'], ['wL', 'vL']))
    fits = t_use is T and r_use is RPf
    assert fits or not launch, "factored matvec step 2 must not need a transpose"
    if not fits or (p2.empty and not launch):
        return None, None, None
    return dict(keys, p1=p1, p2=p2, **{'a0' if W1 is None else 'a01': a}), T1, T


class _DeviceEffectiveH:
    """What the device forms of the effective Hamiltonians share: the factored matvec over the plans of ``_factored_plans``, their
    hand-over between the visits of a bond, and the hand-over of a vector to ``tpa_lanczos_run``.  A subclass provides
    ``_build_program(theta)``."""

    def _apply_factored(self, fp, theta):
        """``LPf . theta`` (GEMM, contracted index = chi, not d chi), the MPO tensors applied blockwise (none without a site), ``. RPf``
        (GEMM, chain over wR and the bond sector), by the plans ``fp``."""
        T = fp['p1'].apply(self._LPf, theta)
        step = fp.get('a01', fp.get('a0'))
        if step is not None:
            T = step.apply(T)
        return fp['p2'].apply(T, self._RPf)

    def adopt_plans(self, plans):
        """Take the plans that :meth:`plans_to_keep` gave on the previous visit of this bond (used only while their keys match)."""
        if self.factored and plans is not None:
            self._fplans = plans

    def plans_to_keep(self):
        """The plans to hand to the next visit of this bond: a complete result of ``_factored_plans``, or ``None``."""
        fp = getattr(self, '_fplans', None)
        return fp if isinstance(fp, dict) and 'lkey' in fp else None

    def _set_counts(self, p1, p2, mpo_bytes=0):
        """The flop and byte counts of a matvec whose GEMM steps are ``p1`` and ``p2`` (they stay as they are where one is empty)."""
        if not p1.empty and not p2.empty:
            self.flops_per_matvec = p1.flops + p2.flops
            self.bytes_per_matvec = p1.bytes_min + p2.bytes_min + mpo_bytes
            self.gemm_shapes = (p1.gemm_shapes, p2.gemm_shapes)

    def matvec_program(self, theta):
        """The matvec as a replayable launch program for ``tpa_lanczos_run``: ``(ops, bufs, gemm_plans[, collective])`` (``_Program``).
        ``None`` when the matvec cannot be replayed on raw arenas: vector not in the operator's own leg order, no plans, mixed
        dtypes, or an output block structure different from the input's (the first steps from a product state, where H creates
        blocks).  ``_build_program(theta)`` of the subclass gives ``(program, last plan of the chain)`` or ``None``."""
        if list(theta.get_leg_labels()) != self.acts_on or theta.stored_blocks == 0 or not theta._is_packed():
            return None
        prog = self.__dict__.get('_program')
        if prog is not None and prog[0] == (theta._struct_key(), theta.dtype):
            return prog[1]
        return self._file_program(theta, *(self._build_program(theta) or (None, None)))

    @staticmethod
    def _closed(theta, last):
        """Whether the result of plan ``last`` has the block structure of ``theta``."""
        return (last.res_total == theta._arena.numel() and np.array_equal(last.res_qdata, theta._qdata)
                and np.array_equal(last.res_offsets, theta._offsets))

    @staticmethod
    def _replayable(theta, *parts):
        """Whether the operands and plans ``parts`` have the dtype of ``theta`` and no plan among them is an empty step."""
        return all(x.dtype == theta.dtype and not getattr(x, 'empty', False) for x in parts)

    def _file_program(self, theta, res, last):
        """Keep the program ``res`` of a contraction chain ending in plan ``last`` for ``theta``'s structure -- or, when the chain's
        output has another block structure than its input (no replay on raw arenas), that structure for :meth:`native_input`."""
        key = (theta._struct_key(), theta.dtype)
        self.__dict__['_program_out'] = None
        if res is not None and not self._closed(theta, last):
            self.__dict__['_program_out'] = (key, last.res_qdata, last.res_offsets, last.res_total)
            res = None
        self.__dict__['_program'] = (key, res)
        return res

    def native_input(self, theta, max_pad=2):
        """``(vector, program)`` for ``tpa_lanczos_run``: ``theta`` itself, or -- when H_eff creates blocks that ``theta`` does not
        store (tiny extreme charge sectors of a state grown from a product state: the first Krylov step of the step-by-step
        loop goes the generic way for them) -- ``theta`` embedded with zero blocks in the block structure of ``H_eff theta``,
        provided that structure is closed under another application.  ``None`` if no replayable program exists."""
        vec = theta
        for _ in range(max_pad + 1):
            prog = self.matvec_program(vec)
            if prog is not None:
                return vec, prog
            out = self.__dict__.get('_program_out')
            if out is None or out[0] != (vec._struct_key(), vec.dtype):
                return None
            _, qdata, offsets, total = out
            have = {tuple(r) for r in qdata.tolist()}
            if not all(tuple(r) in have for r in vec._qdata.tolist()):
                return None                      # H_eff theta lacks blocks of theta: not an embedding
            pad = npc.Array(vec.legs, vec.dtype, vec.qtotal, vec.get_leg_labels())
            pad._set_blocks(qdata, arena=dev.zeros(total, vec.dtype), qdata_sorted=True)
            if not np.array_equal(pad._offsets, offsets):
                return None
            npc._scatter_blocks(vec, pad, pad._arena)
            vec = pad
        return None


class TwoSiteH(_DeviceEffectiveH):
    length = 2
    acts_on = ['(vL.p0)', '(p1.vR)']

    def __init__(self, env, i0, combine=True, move_right=True, tensors=None, factored=None):
        if not combine:     # (TeNPy's own TwoSiteH runs combine=False on the mirror: tenpy_amd/install.py)
            raise NotImplementedError("tenpy_amd.TwoSiteH (stand-alone driver): only combine=True")
        self.i0 = i0
        self.combine = combine
        self.move_right = move_right
        if tensors is not None:      # explicit (LP, RP, W0, W1), e.g. replaying a dumped bond
            self.LP, self.RP, W0, W1 = tensors
            self.dtype = W0.dtype
        else:
            self.LP = env.get_LP(i0)
            self.RP = env.get_RP(i0 + 1)
            W0, W1 = env.H.get_W(i0), env.H.get_W(i0 + 1)
            self.dtype = env.H.dtype
        self.W0 = W0.replace_labels(['p', 'p*'], ['p0', 'p0*'])
        self.W1 = W1.replace_labels(['p', 'p*'], ['p1', 'p1*'])
        # the host copy of the MPO entries is cached on the MPO's own tensors (one D2H read per site for the whole run)
        _share_mpo_tables(self.W0, W0)
        _share_mpo_tables(self.W1, W1)
        self._env = env         # (with explicit tensors: None, or the holder of the caches of `plus_hc`)
        # `_skip_program` serves the operators the drivers build from an environment (explicit tensors, a half MPO with
        # `explicit_plus_hc` whose operator runs as `PlusHcH`, the sharded subclass: the full program)
        self._skip_ok = tensors is None and not getattr(env.H, 'explicit_plus_hc', False)
        self._LHeff = self._RHeff = None
        self._fused = None          # (p1, p2, structure key, dtype) of the LHeff . theta . RHeff form
        self._fplans = None
        if factored is None:
            want = FACTORED_MATVEC and int(np.max(self.LP.get_leg('vR').get_block_sizes())) >= FACTORED_MIN_SECTOR
        else:
            want = factored
        self.factored = bool(want) and self._factored_possible()
        if self.factored:       # pipes only (host bookkeeping); LHeff / RHeff are built on first access
            from ..linalg.charges import LegPipe
            self._LPf = _env_form(self.LP, ['vR*', 'wR', 'vR'])      # leg orders the two GEMM steps want (views; wide MPO bond legs: a copy)
            self._RPf = _env_form(self.RP, ['wL', 'vL', 'vL*'])
            self.pipeL = LegPipe([self.LP.get_leg('vR*'), self.W0.get_leg('p0')], qconj=+1)
            self.pipeR = LegPipe([self.W1.get_leg('p1'), self.RP.get_leg('vL*')], qconj=-1)
            self._LHeff = self._RHeff = None
            self.acts_on = ['vL', 'p0', 'p1', 'vR']
        else:
            self.combine_Heff(self._env)
        self.N = self.pipeL.ind_len * self.pipeR.ind_len
        self.flops_per_matvec = None
        self.bytes_per_matvec = None

    def _factored_possible(self):
        return factored_matvec_possible(self.LP, self.RP, self.W0, self.W1)

    # LHeff / RHeff: attributes in the fused mode, built lazily in the factored mode (mixer, tests)
    @property
    def LHeff(self):
        if self._LHeff is None:
            self._build_heff_lazily()
        return self._LHeff

    @LHeff.setter
    def LHeff(self, value):
        self._LHeff = value

    @property
    def RHeff(self):
        if self._RHeff is None:
            self._build_heff_lazily()
        return self._RHeff

    @RHeff.setter
    def RHeff(self, value):
        self._RHeff = value

    def _build_heff_lazily(self):
        pL, pR = self.pipeL, self.pipeR
        self.combine_Heff(self._env)
        pL.test_equal(self.pipeL)
        pR.test_equal(self.pipeR)
        self.pipeL, self.pipeR = pL, pR      # keep the pipe objects theta was fused with

    def combine_Heff(self, env=None):
        """LHeff = LP.W0 and RHeff = W1.RP with the (virtual, physical) legs fused into pipes.

        Reference: ``TwoSiteH.combine_Heff`` (mps_common.py:1350).  With an environment, the fused tensors are kept in
        ``env._heff_cache`` keyed by (side, site) and reused as long as the environment tensor they were built from is
        still the stored one: in a right-moving half sweep RHeff of a bond is exactly the one built when the previous
        left-moving half sweep optimised that bond (and vice versa), so only one of the two is rebuilt per update.
        All cached tensors stay in HBM (2 x 131 MB per bond at chi=2048, < 26 GB for L=100)."""
        cache = getattr(env, '_heff_cache', None) if env is not None else None
        hit = cache.get(('L', self.i0)) if cache is not None else None
        if hit is not None and hit[0] is self.LP:
            _, self.LHeff, self.pipeL = hit
        else:
            fused = _fused_heff(self.LP, self.W0, True) if FUSED_HEFF else None
            if fused is not None:
                self.LHeff, self.pipeL = fused
            else:
                LHeff = npc.tensordot(self.LP, self.W0, axes=['wR', 'wL'])        # vR*, vR, wR, p0, p0*
                self.pipeL = pipeL = LHeff.make_pipe(['vR*', 'p0'], qconj=+1)
                self.LHeff = LHeff.combine_legs([['vR*', 'p0'], ['vR', 'p0*']], pipes=[pipeL, pipeL.conj()],
                                                new_axes=[0, 2])                   # (vR*.p0), wR, (vR.p0*)
            if cache is not None:
                cache[('L', self.i0)] = (self.LP, self.LHeff, self.pipeL)
        hit = cache.get(('R', self.i0 + 1)) if cache is not None else None
        if hit is not None and hit[0] is self.RP:
            _, self.RHeff, self.pipeR = hit
        else:
            fused = _fused_heff(self.RP, self.W1, False) if FUSED_HEFF else None
            if fused is not None:
                self.RHeff, self.pipeR = fused
            else:
                RHeff = npc.tensordot(self.W1, self.RP, axes=['wR', 'wL'])        # wL, p1, p1*, vL, vL*
                self.pipeR = pipeR = RHeff.make_pipe(['p1', 'vL*'], qconj=-1)
                self.RHeff = RHeff.combine_legs([['p1*', 'vL'], ['p1', 'vL*']], pipes=[pipeR.conj(), pipeR],
                                                new_axes=[1, 2])                   # wL, (p1*.vL), (p1.vL*)
            if cache is not None:
                cache[('R', self.i0 + 1)] = (self.RP, self.RHeff, self.pipeR)

    def combine_theta(self, theta):
        """theta (vL, p0, p1, vR) -> the form the matvec acts on: the matrix [(vL.p0), (p1.vR)] (pipes of Heff), or --
        factored mode -- the un-fused tensor itself (an already fused theta is split)."""
        if self.factored:
            if theta.rank == 2:
                theta = theta.split_legs()
            return theta if list(theta.get_leg_labels()) == ['vL', 'p0', 'p1', 'vR'] else theta.transpose(['vL', 'p0', 'p1', 'vR'])
        return theta.combine_legs([['vL', 'p0'], ['p1', 'vR']], pipes=[self.pipeL, self.pipeR])

    def prepare_svd(self, theta):
        """The matrix [(vL.p0), (p1.vR)] that svd_theta / the mixer expect (fused once per bond in the factored mode)."""
        if theta.rank == 2:
            return theta
        return theta.combine_legs([['vL', 'p0'], ['p1', 'vR']], pipes=[self.pipeL, self.pipeR])

    def _matvec_factored(self, theta):
        """theta [vL, p0, p1, vR] -> LP . theta . W0 W1 . RP with the same legs (``_apply_factored``)."""
        fp, T3 = self._plans_for(theta, launch=True)      # (building the plans runs the first two steps)
        res = self._apply_factored(fp, theta) if T3 is None else fp['p2'].apply(T3, self._RPf)
        res.iset_leg_labels(['vL', 'p0', 'p1', 'vR'])
        return res

    def _plans_for(self, theta, launch):
        """``_factored_plans`` for ``theta``: the plans (``None``: there are none, and ``_fplans`` stays) and the result of the MPO
        step if they were built now; new plans are kept in ``_fplans`` with their flop and byte counts."""
        fp, _, T3 = _factored_plans(self._LPf, self._RPf, theta, self.W0, self.W1, launch, old=self._fplans)
        if fp is not None and fp is not self._fplans:
            self._fplans = fp
            self._set_counts(fp['p1'], fp['p2'], fp['a01'].bytes)
        return fp, T3

    def _fused_plans(self, theta, launch):
        """``(p1, p2, tmp)``: the plans of ``LHeff . theta`` and ``. RHeff`` as ``_fused`` keeps them, and the result of step 1 if they
        were built now (else ``None``).  ``launch`` as in ``_factored_plans``: step 1 runs while they are built and a transposed
        copy is an assertion failure; without it nothing is launched, and a transposed copy or an empty step means ``None``."""
        if self._fused is not None and self._fused[2:] == (theta._struct_key(), theta.dtype):
            return self._fused[0], self._fused[1], None
        p1, l_use, t_use = npc.plan_tensordot(self.LHeff, theta, axes=['(vR.p0*)', '(vL.p0)'])
        fits = l_use is self.LHeff and t_use is theta
        assert fits or not launch, "matvec step 1 must not need a transpose"
        if not fits or (p1.empty and not launch):
            return None
        tmp = p1.apply(self.LHeff, theta, launch=launch)
        p2, t2_use, r_use = npc.plan_tensordot(tmp, self.RHeff, axes=(['wR', '(p1.vR)'], ['wL', '(p1*.vL)']))
        fits = t2_use is tmp and r_use is self.RHeff
        assert fits or not launch, "matvec step 2 must not need a transpose"
        if not fits or (p2.empty and not launch):
            return None
        self._fused = (p1, p2, theta._struct_key(), theta.dtype)
        self._set_counts(p1, p2)
        return p1, p2, tmp

    def matvec(self, theta):
        """theta [(vL.p0), (p1.vR)] (fused mode) or [vL, p0, p1, vR] (factored mode) -> H_eff theta, same legs and labels."""
        if self.factored:
            if theta.rank == 2:      # a fused vector handed to a factored operator (tests, parity checks)
                return self.prepare_svd(self._matvec_factored(self.combine_theta(theta)))
            return self._matvec_factored(theta)
        p1, p2, tmp = self._fused_plans(theta, launch=True)
        res = p2.apply(p1.apply(self.LHeff, theta) if tmp is None else tmp, self.RHeff)
        res.iset_leg_labels(['(vL.p0)', '(p1.vR)'])
        return res

    def _build_program(self, theta):
        if self.factored:
            fp = self._plans_for(theta, launch=False)[0]
            if fp is None:
                return None
            p1, a01, p2 = fp['p1'], fp['a01'], fp['p2']
            if not self._replayable(theta, self._LPf, self._RPf, p1, a01, p2):
                return None
            res = self._skip_program(theta, fp)
            if res is None:
                prog = self._new_program(p1, a01)
                prog.gemm(p1, 0, -1, 2, 'lanczos_sk1')
                prog.mpo_step(a01, 2, 3)
                prog.gemm(p2, 3, 1, -2, 'lanczos_sk2')
                res = prog.finish((p1, p2))
            return res, p2
        plans = self._fused_plans(theta, launch=False)
        if plans is None or not self._replayable(theta, self.LHeff, self.RHeff, *plans[:2]):
            return None
        p1, p2 = plans[:2]
        prog = _Program(self.LHeff._arena, self.RHeff._arena)
        prog.scratch('lanczos_t1', p1.res_total, p1.dtype)
        prog.gemm(p1, 0, -1, 2, 'lanczos_sk1')
        prog.gemm(p2, 2, 1, -2, 'lanczos_sk2')
        return prog.finish((p1, p2)), p2

    def _new_program(self, p1, a01):
        """A program of the factored form: LP, RP, T1 and T3 in slots 0 to 3."""
        prog = _Program(self._LPf._arena, self._RPf._arena)
        prog.scratch('lanczos_t1', p1.res_total, p1.dtype)
        prog.scratch('lanczos_t3', a01.total, a01.dtype)
        return prog

    # ---- the launch program without the work nobody reads ----------------------------------------------------
    def _skip_program(self, theta, fp):
        """The program of the factored matvec with the bits of the full program and less work, or ``None`` (the caller then builds the
        full program):

        a (kind 0)  step 1 with the tiles of the blocks of T1 that some term of the MPO step reads (split-K as ``p1`` has it, with the
                    reduction jobs of these blocks).  All tiles stay where dropping some would move the launch to another kernel
                    (``tpa_gemm_kernel_id``);
        b (kind 1)  the MPO step for the blocks of T3 that have several terms;
        c (kind 7)  step 2 through ``tpa_gemm_chain_ex`` on the tables of ``p2`` (split-K: of its parts, then their reduction as today),
                    in which a link over a block of T3 that is ONE term ``alpha . block of T1`` reads that block of T1 as the second
                    source and scales it on its way into LDS -- the rounding of ``tpa_lincomb_batch``.

        Same chains, same order, same tile tables.  For operators of this very class built from an environment, float64,
        ``MpoApplyPlan``, a closed block structure and a library that provides ``tpa_gemm_chain_ex``.  Tables per block structure:
        ``_skip_table_cache``.  Counters: ``krylov_based.stats['n_skip_taken' / 'n_skip_declined']``, reasons in
        ``krylov_based.skip_declined``."""
        from ..linalg import krylov_based as kb
        p1, a01, p2 = fp['p1'], fp['a01'], fp['p2']
        if not MATVEC_SKIP or not self._closed(theta, p2):
            return None                     # (switched off; H creates blocks: `_file_program` keeps no program either way)

        def declined(reason):
            kb.stats['n_skip_declined'] += 1
            kb.skip_declined[reason] = kb.skip_declined.get(reason, 0) + 1
            return None
        if type(self) is not TwoSiteH or not self._skip_ok:
            return declined('operator')
        if type(a01) is not MpoApplyPlan:
            return declined('mpo_plan')
        if theta.dtype != np.float64:
            return declined('dtype')
        if not (dev.lib_provides('tpa_gemm_chain_ex') and hasattr(dev.lib(), 'tpa_gemm_kernel_id')):
            return declined('library')
        key = (id(p1), id(a01), id(p2))
        hit = _skip_table_cache.get(key)
        if hit is not None and hit[0] is p1 and hit[1] is a01 and hit[2] is p2:
            _skip_table_cache.move_to_end(key)
            et = hit[3]
        else:
            et = self._skip_tables(fp)
            _skip_table_cache[key] = (p1, a01, p2, et)          # (the plans stay alive with their ids)
            if len(_skip_table_cache) > 1024:
                _skip_table_cache.popitem(last=False)
        if isinstance(et, str):
            return declined(et)
        kb.stats['n_skip_taken'] += 1
        prog = self._new_program(p1, a01)
        prog.gemm(p1, 0, -1, 2, 'lanczos_sk1', tiles=et['a_tiles'], jobs=et['a_jobs'])
        if et['b_jobs'] is not None:
            prog.lincomb(et['b_jobs'], len(et['b_jobs']), a01.terms_dev, a01.max_elems, 2, 3)
        prog.gemm(p2, 3, 1, -2, 'lanczos_sk2', links=et['c_links'], a2=2, alphas=et['alphas'])
        self._set_counts(et['plan_a'], p2, et['b_bytes'])
        return prog.finish((et['plan_a'], p2))

    @staticmethod
    def _skip_tables(fp):
        """The tables of :meth:`_skip_program` (numpy only, no device read-back): a dict, or the reason (a string) why there is nothing
        to skip or to build."""
        p1, a01, p2 = fp['p1'], fp['a01'], fp['p2']
        jobs3, terms3 = a01.jobs_host, a01.terms_host
        t1_off = np.asarray(p1.res_offsets, dtype=np.int64)
        term_t1 = np.searchsorted(t1_off, terms3[:, 0])
        if not np.array_equal(t1_off[np.minimum(term_t1, len(t1_off) - 1)], terms3[:, 0]):
            return 'term_inside_block'
        # ---- step 2: a link over a single-term block of T3 reads the block of T1 (a split-K part: the same cut of it)
        order = np.argsort(jobs3[:, 0])
        j_off, j_size = jobs3[order, 0], jobs3[order, 1] * jobs3[order, 2]
        single, first_term = jobs3[order, 5] == 1, jobs3[order, 4]
        links = (p2.links_host if p2.sk is None else p2.sk.links_host).copy()
        lj = np.clip(np.searchsorted(j_off, links[:, 0], side='right') - 1, 0, len(j_off) - 1)
        inside = (links[:, 0] >= j_off[lj]) & (links[:, 0] < j_off[lj] + j_size[lj])
        if not np.all(inside | (links[:, 2] <= 0)):
            return 'link_outside_blocks'
        swap = inside & single[lj] & (links[:, 2] > 0)
        term = first_term[lj[swap]]
        if np.any(terms3[term, 1] != j_size[lj[swap]]):
            return 'term_shape'
        alpha = terms3[:, 2:4].copy().view(np.float64)[:, 0]
        ualpha, ai = np.unique(alpha[term], return_inverse=True)
        if len(ualpha) + 1 > 0xffff:
            return 'too_many_coefficients'
        alphas = np.zeros(2 * (len(ualpha) + 1), dtype=np.float64)
        alphas[0], alphas[2::2] = 1., ualpha
        links[swap, 0] = terms3[term, 0] + (links[swap, 0] - j_off[lj[swap]])
        links[swap, 7] = (links[swap, 7] & 3) | 4 | ((ai.reshape(-1) + 1) << 16)
        multi = np.sort(order[~single])
        et = dict(a_tiles=None, a_jobs=None, b_jobs=None)
        b_elems = 0
        if len(multi):
            in_multi = np.zeros(len(terms3), dtype=bool)
            starts, counts = jobs3[multi, 4], jobs3[multi, 5]
            in_multi[np.repeat(starts, counts) + np.arange(int(np.sum(counts))) - np.repeat(np.cumsum(counts) - counts, counts)] = True
            b_elems = int(np.sum(terms3[in_multi, 1]) + np.sum(jobs3[multi, 1] * jobs3[multi, 2]))
        # ---- step 1: the tiles of the blocks of T1 that are read
        need = np.zeros(len(t1_off), dtype=bool)
        need[term_t1] = True
        plan_a = p1
        if not np.all(need):
            sk, t1 = p1.sk, p1.tasks_host
            src = p1.tiles_host if sk is None else sk.tiles_host
            tile_task = src[:, 0] if sk is None else np.repeat(np.arange(len(t1_off)), sk.parts)[src[:, 0]]
            kept = np.ascontiguousarray(src[need[tile_task]])
            kernel = dev.lib().tpa_gemm_kernel_id
            if kernel(dev.code(p1.dtype), p1.cfg, len(kept)) == kernel(dev.code(p1.dtype), p1.cfg, len(src)):
                cnt = t1[need, 5]
                lk = np.repeat(t1[need, 4], cnt) + np.arange(int(np.sum(cnt))) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                mt, nt_, kk = np.repeat(t1[need, 1], cnt), np.repeat(t1[need, 2], cnt), p1.links_host[lk, 2]
                _, ua = np.unique(p1.links_host[lk, 0], return_index=True)
                _, ub = np.unique(p1.links_host[lk, 1], return_index=True)
                from types import SimpleNamespace
                plan_a = SimpleNamespace(empty=False, flops=int(2 * np.sum(mt * kk * nt_)), gemm_shapes=np.stack([mt, kk, nt_], axis=1),
                                         bytes_min=int(8 * (np.sum(mt[ua] * kk[ua]) + np.sum(kk[ub] * nt_[ub]) + np.sum(t1[need, 1] * t1[need, 2]))))
                if sk is None:
                    (et['a_tiles'],) = dev.to_device_packed(kept)
                else:
                    et['a_tiles'], et['a_jobs'] = dev.to_device_packed(kept, np.ascontiguousarray(sk.jobs_host[need]))
        if et['a_tiles'] is None and not np.any(swap):
            return 'nothing_to_skip'
        if len(multi):
            et['c_links'], et['alphas'], et['b_jobs'] = dev.to_device_packed(links, alphas, np.ascontiguousarray(jobs3[multi]))
        else:
            et['c_links'], et['alphas'] = dev.to_device_packed(links, alphas)
        et['plan_a'], et['b_bytes'], et['n_swapped'] = plan_a, 8 * b_elems, int(np.sum(swap))
        return et

    def update_LP(self, env, i, U=None):
        """LP(i0+1) = U^dagger LHeff U   (reference :1421)."""
        assert i == self.i0 + 1
        if self.factored:       # LP' = A^dagger (LP . A) W0 without LHeff (reference MPOEnvironment._contract_LP, mpo.py:3087)
            A = U.split_legs(['(vL.p0)'])                                        # vL, p0, vR
            cls = _mpo_plan_class(self.W0)
            X = npc.tensordot(self._LPf if cls is MpoEntryApplyPlan else self.LP, A, axes=['vR', 'vL'])     # vR*, wR, p0, vR
            X = _mpo_step_lr(X, self.W0, out_labels=('vR*', 'p0', 'wR', 'vR')).apply(X)
            LP = npc.tensordot(A.conj(), X, axes=(['vL*', 'p0*'], ['vR*', 'p0']))   # vR*, wR, vR
            LP = _env_form(LP, list(self.LP.get_leg_labels()))
            _env_set_LP(env, i, LP)
            return LP
        LP = npc.tensordot(self.LHeff, U, axes=['(vR.p0*)', '(vL.p0)'])
        LP = npc.tensordot(U.conj(), LP, axes=['(vL*.p0*)', '(vR*.p0)'])      # vR*, wR, vR
        _env_set_LP(env, i, LP)
        return LP

    def update_RP(self, env, i, VH=None):
        """RP(i0) = RHeff VH VH^dagger   (reference :1430)."""
        assert i == self.i0
        if self.factored:       # RP' = (B . RP) W1 B^dagger without RHeff (reference _contract_RP, mpo.py:3097)
            B = VH.split_legs(['(p1.vR)'])                                       # vL, p1, vR
            cls = _mpo_plan_class(self.W1)
            X = npc.tensordot(B, self._RPf if cls is MpoEntryApplyPlan else self.RP, axes=['vR', 'vL'])     # vL, p1, wL, vL*
            X = _mpo_step_rl(X, self.W1, out_labels=('vL', 'wL', 'p1', 'vL*')).apply(X)
            RP = npc.tensordot(X, B.conj(), axes=(['p1', 'vL*'], ['p1*', 'vR*']))   # vL, wL, vL*
            RP = _env_form(RP, list(self.RP.get_leg_labels()))
            _env_set_RP(env, i, RP)
            return RP
        RP = npc.tensordot(VH, self.RHeff, axes=['(p1.vR)', '(p1*.vL)'])      # vL, wL, (p1.vL*)
        RP = npc.tensordot(RP, VH.conj(), axes=['(p1.vL*)', '(p1*.vR*)'])     # vL, wL, vL*
        _env_set_RP(env, i, RP)
        return RP

    def adjoint(self):
        """The Hermitian conjugate as an operator of its own (``AdjointH``: the reference's contractions on the conjugated tensors)."""
        return AdjointH(self)

    def plus_hc(self):
        """``self + self.adjoint()`` as ONE operator of this class on the direct sum along the MPO bond (``PlusHcH``), or ``None`` where
        that form does not apply (``_plus_hc_operator``) -- the caller then sums the two operators itself."""
        return _plus_hc_operator(self)

    def to_matrix_array(self):
        """The effective Hamiltonian contracted to a device matrix with legs [(vL.p0.p1.vR)-like pipe, its conj]
        (reference ``TwoSiteH.to_matrix`` :1392) -- for the exact diagonalisation of small bonds (``full_diag_effH``)."""
        contr = npc.tensordot(self.LHeff, self.RHeff, axes=['wR', 'wL'])
        return contr.combine_legs([['(vR*.p0)', '(p1.vL*)'], ['(vR.p0*)', '(p1*.vL)']], qconj=[+1, -1])

    def to_matrix(self):
        """Dense effective Hamiltonian on the host (tests only)."""
        L, R = self.LHeff.to_ndarray(), self.RHeff.to_ndarray()
        full = np.tensordot(L, R, axes=([1], [0]))           # (vR*.p0), (vR.p0*), (p1*.vL), (p1.vL*)
        full = full.transpose(0, 3, 1, 2)                    # out_L, out_R, in_L, in_R
        n = full.shape[0] * full.shape[1]
        return full.reshape(n, n)


# ---------------------------------------------------------------------------------------------------------------------
# One- and zero-site effective Hamiltonians (TDVP: ``one_site_update`` after every two-site update, ``zero_site_update`` after
# every one-site update of the single-site algorithm), in the factored form of ``TwoSiteH``:
#     one site   theta [vL, p0, vR]:  T1 = LP . theta (grouped GEMM),  T2 = W0 applied blockwise (MpoApplyPlan / MpoBlockApplyPlan),
#                                     theta' = T2 . RP (grouped GEMM chained over wR and the bond sector)
#     zero sites theta [vL, vR]    :  T1 = LP . theta,  theta' = T1 . RP chained over (wR, vR)
# instead of three generic tensordots with transposed copies and a K = 1 GEMM per MPO entry (reference mps_common.py:1146-1149,
# :1512-1514).
class _LocalH(_DeviceEffectiveH):
    combine = False
    move_right = True
    _env = None             # the environment the tensors were taken from, where the constructor knows it (caches of `plus_hc`)

    def _setup(self, LP, W0, RP, i0, dtype):
        self.i0 = i0
        self.LP, self.RP = LP, RP
        self.W0 = None
        if W0 is not None:
            self.W0 = W0.replace_labels(['p', 'p*'], ['p0', 'p0*'])
            _share_mpo_tables(self.W0, W0)               # (host copy of the entries / blocks: cached on the MPO's own tensor)
        self.dtype = dtype
        self._fplans = None
        if W0 is None:
            self.factored = _envs_factorable(LP, RP)
        else:
            self.factored = (list(self.W0.get_leg_labels()) == ['wL', 'wR', 'p0', 'p0*'] and
                             _factored_plan_class(LP, RP, self.W0) is not None)
        if self.factored:
            self._LPf = _env_form(LP, ['vR*', 'wR', 'vR'])
            self._RPf = _env_form(RP, ['wL', 'vL', 'vL*'])
        n = LP.get_leg('vR').ind_len * RP.get_leg('vL').ind_len
        self.N = n if W0 is None else n * self.W0.get_leg('p0').ind_len

    def _plans(self, theta):
        """The cached plans of the three (two) steps for this ``theta`` -- rebuilt whenever the block structure of ``theta`` OR of an
        environment differs from the one they were made for (plans are handed from visit to visit of a site while the
        environments grow); ``None`` when a step would need a transposed copy or contributes nothing."""
        self._fplans = _factored_plans(self._LPf, self._RPf, theta, self.W0, old=self._fplans)[0]
        return self._fplans

    def matvec(self, theta):
        """``theta`` with the labels of ``acts_on`` (any order) -> ``H_eff theta``, same legs and labels."""
        labels = list(theta.get_leg_labels())
        if labels != self.acts_on:
            theta = theta.transpose(self.acts_on)
        fp = self._plans(theta) if (self.factored and theta.stored_blocks > 0) else None
        if fp is not None:
            res = self._apply_factored(fp, theta)
        else:               # the reference's contractions (no blockwise form of the MPO step -- `_mpo_plan_class` --, empty theta)
            res = npc.tensordot(self.LP, theta, axes=['vR', 'vL'])
            if self.W0 is not None:
                res = npc.tensordot(self.W0, res, axes=[['wL', 'p0*'], ['wR', 'p0']])
            res = npc.tensordot(res, self.RP, axes=[['wR', 'vR'], ['wL', 'vL']])
            res = res.replace_labels(['vR*', 'vL*'], ['vL', 'vR']).transpose(self.acts_on)
        res.iset_leg_labels(self.acts_on)
        return res if labels == self.acts_on else res.transpose(labels)

    def _build_program(self, theta):
        fp = self._plans(theta) if self.factored else None
        if fp is None:
            return None
        p1, a0, p2 = fp['p1'], fp['a0'], fp['p2']
        if not self._replayable(theta, self._LPf, self._RPf, *(p for p in (p1, a0, p2) if p is not None)):
            return None
        prog = _Program(self._LPf._arena, self._RPf._arena)
        src = prog.scratch('lanczos_t1', p1.res_total, p1.dtype)
        prog.gemm(p1, 0, -1, src, 'lanczos_sk1')
        if a0 is not None:
            t3 = prog.scratch('lanczos_t3', a0.total, a0.dtype)
            prog.mpo_step(a0, src, t3)
            src = t3
        prog.gemm(p2, src, 1, -2, 'lanczos_sk2')
        return prog.finish((p1, p2)), p2

    def adjoint(self):
        return AdjointH(self)

    def plus_hc(self):
        """See :meth:`TwoSiteH.plus_hc`."""
        return _plus_hc_operator(self)

    def to_matrix(self):
        """``self`` contracted to a matrix ``[(vR*.p0.vL*), (vR.p0*.vL)]`` (reference :1205-1207, :1520-1521)."""
        contr = self.LP
        if self.W0 is not None:
            contr = npc.tensordot(contr, self.W0, axes=['wR', 'wL'])
        contr = npc.tensordot(contr, self.RP, axes=['wR', 'wL'])
        if self.W0 is not None:
            return contr.combine_legs([['vR*', 'p0', 'vL*'], ['vR', 'p0*', 'vL']], qconj=[+1, -1])
        return contr.combine_legs([['vR*', 'vL*'], ['vR', 'vL']], qconj=[+1, -1])


class OneSiteH(_LocalH):
    """Effective one-site Hamiltonian ``LP - W0 - RP`` acting on ``theta [vL, p0, vR]`` (reference ``OneSiteH``,
    mps_common.py:1040) for ``combine=False``, which is what TDVP uses."""
    length = 1
    acts_on = ['vL', 'p0', 'vR']

    def __init__(self, env, i0, combine=False, move_right=True):
        if combine:
            raise NotImplementedError("tenpy_amd.OneSiteH (stand-alone driver): only combine=False")
        self.move_right = move_right
        self._env = env
        self._setup(env.get_LP(i0), env.H.get_W(i0), env.get_RP(i0), i0, env.H.dtype)

    @classmethod
    def from_LP_W0_RP(cls, LP, W0, RP, i0=0, combine=False, move_right=True):
        if combine:
            raise NotImplementedError("tenpy_amd.OneSiteH: only combine=False")
        self = cls.__new__(cls)
        self.move_right = move_right
        self._setup(LP.transpose(['vR*', 'wR', 'vR']), W0, RP.transpose(['wL', 'vL', 'vL*']), i0, LP.dtype)
        return self

    def combine_theta(self, theta):
        return theta if list(theta.get_leg_labels()) == self.acts_on else theta.transpose(self.acts_on)

    def update_LP(self, env, i, U=None):
        env.get_LP(i, store=True)

    def update_RP(self, env, i, VH=None):
        env.get_RP(i, store=True)


class ZeroSiteH(_LocalH):
    """Effective zero-site Hamiltonian ``LP - RP`` acting on the bond matrix ``theta [vL, vR]`` left of site ``i0`` (reference
    ``ZeroSiteH``, mps_common.py:1440)."""
    length = 0
    acts_on = ['vL', 'vR']

    def __init__(self, env, i0):
        self._env = env
        self._setup(env.get_LP(i0), None, env.get_RP(i0 - 1), i0, env.H.dtype)

    @classmethod
    def from_LP_RP(cls, LP, RP, i0=0):
        self = cls.__new__(cls)
        self._setup(LP.transpose(['vR*', 'wR', 'vR']), None, RP.transpose(['wL', 'vL', 'vL*']), i0, LP.dtype)
        return self


# ---------------------------------------------------------------------------------------------------------------------
# H + h.c.: MPOs with ``explicit_plus_hc`` store half of the Hamiltonian, and the engines apply ``H_eff + H_eff^dagger`` (reference
# mps_common.py:519, tdvp.py:310, :422 -- ``SumNpcLinearOperator(eff_H, eff_H.adjoint())``: two matvecs and an axpy).  The sum is itself an
# MPO-shaped operator, the direct sum along the MPO bond:
#     LPd = [LP ; LP^dagger] (stacked on wR),   Wd = W (+) W^dagger (block diagonal in wL, wR),   RPd = [RP ; RP^dagger] (stacked on wL)
#     LPd . theta . (W0d W1d) . RPd = H theta + H^dagger theta
# with the tensors of the reference's ``adjoint()`` (:1404-1419, :1210, :1524): ``LP^dagger[vR*, wR, vR] = conj(LP)`` with the two virtual
# legs exchanged, ``W^dagger[wL, wR, p, p*] = conj(W[wL, wR, p*, p])``.  ``conj()`` flips the ``qconj`` of the MPO bond legs; next to the
# plain half the adjoint half carries ``leg.conj().flip_charges_qconj()`` -- negated charges, the original ``qconj``.  The stacked legs are
# unsorted and repeat charges.  1-wide bond blocks stay 1-wide and scalar MPO blocks stay scalar, so everything that exists for a plain
# operator (the factored matvec and its launch program, the native Krylov loops, the projections of ``OrthogonalNpcLinearOperator``)
# serves the doubled one through its tables: three launches per matvec, the sum over the two halves inside the accumulation chains of
# the second GEMM.  ``TPA_PLUS_HC=0``: the routing without all of this.
PLUS_HC = _os.environ.get('TPA_PLUS_HC', '1') != '0'
plus_hc_stats = {'env_builds': 0, 'env_hits': 0, 'W_builds': 0}
_HC_SWAP = {'vR*': 'vR', 'vR': 'vR*', 'vL': 'vL*', 'vL*': 'vL'}


def _hc_leg(leg):
    """The MPO bond leg of an adjoint tensor as it stands next to the plain one: negated charges, the same ``qconj``."""
    return leg.conj().flip_charges_qconj()


def _doubled_leg(leg):
    """``[leg ; _hc_leg(leg)]``: block ``q`` of the adjoint half is block ``leg.block_number + q``."""
    return leg.extend(_hc_leg(leg))


def _hc_part(A, labels, hc, w_shift=0):
    """Blocks of ``A`` (``hc``: of its adjoint) as blocks of a tensor with the legs in the order ``labels``: their block indices, and the
    rows of a ``tpa_copy_batch`` job table without the destination offsets (conjugating, virtual legs exchanged for ``hc``)."""
    src_ax = [A.get_leg_index(_HC_SWAP.get(l, l) if hc else l) for l in labels]
    qd = np.array(A._qdata[:, src_ax], dtype=np.intp)
    w_ax = [k for k, l in enumerate(labels) if l in ('wR', 'wL')][0]
    qd[:, w_ax] += w_shift
    shapes = A._block_shapes()
    M = npc.COPY_MAXDIM
    jobs = np.zeros((len(qd), 4 + 3 * M), dtype=np.int64)
    jobs[:, 1], jobs[:, 2], jobs[:, 3] = A._offsets, A.rank, 1 if hc else 0
    jobs[:, 4:4 + A.rank] = shapes[:, src_ax]
    jobs[:, 4 + M:4 + M + A.rank] = npc._c_strides(shapes[:, src_ax])
    jobs[:, 4 + 2 * M:4 + 2 * M + A.rank] = npc._c_strides(shapes)[:, src_ax]
    return qd, jobs


def _hc_assemble(A, legs, labels, parts):
    """The tensor with ``legs`` whose blocks are those of ``parts`` (``_hc_part``), written by one copy launch per part."""
    res = npc.Array(legs, A.dtype, A.chinfo.make_valid(), labels)
    qd = np.concatenate([p[0] for p in parts])
    order = np.lexsort(qd.T)                # last leg most significant, like every sorted _qdata
    res._set_blocks(qd[order], qdata_sorted=True)
    dst = np.empty(len(qd), dtype=np.int64)
    dst[order] = res._offsets
    sizes = A._block_sizes_flat()
    n0 = 0
    for _, jobs in parts:
        jobs[:, 0] = dst[n0:n0 + len(jobs)]
        n0 += len(jobs)
        npc._run_copy(A.dtype, jobs, int(np.max(sizes)) if len(sizes) else 0, A._arena, res._arena)
    return res


def _hc_env_ok(A, left):
    """Whether ``A`` is an environment tensor whose adjoint lives on the same legs: standard labels, charge-neutral, the bra leg the
    conjugate of the ket leg (bra is ket)."""
    labels = ['vR*', 'wR', 'vR'] if left else ['wL', 'vL', 'vL*']
    if sorted(A.get_leg_labels()) != sorted(labels) or A.stored_blocks == 0 or np.any(A.qtotal != 0):
        return False
    ket, bra = ('vR', 'vR*') if left else ('vL', 'vL*')
    try:
        A.get_leg(ket).conj().test_equal(A.get_leg(bra))
    except ValueError:
        return False
    return True


def _adjoint_env(A, left):
    """``LP^dagger`` (``left``) / ``RP^dagger`` of the reference's ``adjoint()`` in the label order of ``A``: the conjugate with the two
    virtual legs exchanged; its MPO bond leg is ``_hc_leg`` of ``A``'s.  One conjugating, transposing copy launch."""
    labels = list(A.get_leg_labels())
    w = 'wR' if left else 'wL'
    legs = [_hc_leg(leg) if l == w else leg for leg, l in zip(A.legs, labels)]
    return _hc_assemble(A, legs, labels, [_hc_part(A, labels, True)])


def _plus_hc_env(A, left, cache=None, site=None):
    """``[LP ; LP^dagger]`` stacked on ``wR`` (``left``) / ``[RP ; RP^dagger]`` stacked on ``wL``, in the leg order the factored forms
    contract (``_envs_factorable``), whatever the stored order of ``A``.  The arena is written by two copy launches: the plain blocks,
    and the adjoint blocks conjugated and transposed on the way.  ``cache``: dict ``(side, site) -> (A, doubled)`` kept by the caller
    (the pattern of ``env._heff_cache``); an entry is valid while ``A`` is the tensor it was built from."""
    key = ('L' if left else 'R', site)
    hit = cache.get(key) if cache is not None else None
    if hit is not None and hit[0] is A:
        plus_hc_stats['env_hits'] += 1
        return hit[1]
    labels = ['vR*', 'wR', 'vR'] if left else ['wL', 'vL', 'vL*']
    w = 'wR' if left else 'wL'
    legs = [_doubled_leg(A.get_leg(l)) if l == w else A.get_leg(l) for l in labels]
    res = _hc_assemble(A, legs, labels, [_hc_part(A, labels, False), _hc_part(A, labels, True, A.get_leg(w).block_number)])
    plus_hc_stats['env_builds'] += 1
    if cache is not None:
        cache[key] = (A, res)
    return res


def _plus_hc_W(W):
    """``W (+) W^dagger``, block diagonal in (wL, wR), for an MPO tensor with the labels ``wL, wR, p, p*``; ``None`` for other labels or a
    charged tensor.  Built once per MPO tensor on the host and cached on it, so that its host tables (``_tpa_entries``, ``_mpo_blocks``,
    ``_mpo_coo``) are read once per run as well."""
    Wd = getattr(W, '_tpa_plus_hc', False)
    if Wd is False:
        Wd = None
        if list(W.get_leg_labels()) == ['wL', 'wR', 'p', 'p*'] and not np.any(W.qtotal != 0) and W.stored_blocks > 0:
            D = W.to_ndarray()
            DL, DR = D.shape[:2]
            full = np.zeros((2 * DL, 2 * DR) + D.shape[2:], dtype=D.dtype)
            full[:DL, :DR] = D
            full[DL:, DR:] = D.conj().transpose(0, 1, 3, 2)
            legs = [_doubled_leg(W.get_leg('wL')), _doubled_leg(W.get_leg('wR')), W.get_leg('p'), W.get_leg('p*')]
            Wd = npc.Array.from_ndarray(full, legs, dtype=W.dtype, qtotal=W.qtotal, labels=['wL', 'wR', 'p', 'p*'])
            plus_hc_stats['W_builds'] += 1
        W._tpa_plus_hc = Wd
    return Wd


class _HeffCacheHolder:
    """What ``TwoSiteH.combine_Heff`` asks of an environment: the dict of the fused tensors (here: of the doubled operator)."""

    def __init__(self, cache):
        self._heff_cache = cache


def _plus_hc_operator(op):
    """``PlusHcH`` for the plain operator ``op`` (``TwoSiteH`` / ``OneSiteH`` / ``ZeroSiteH`` or a subclass), or ``None``: switch off,
    bra is not ket, a charged tensor, mixed dtypes, MPO tensors or environments that the factored forms do not take when doubled."""
    if not PLUS_HC:
        return None
    env = getattr(op, '_env', None)
    if env is not None and getattr(env, 'bra', None) is not getattr(env, 'ket', None):
        return None
    LP, RP = op.LP, op.RP
    Ws = [W for W in (getattr(op, 'W0', None), getattr(op, 'W1', None)) if W is not None]
    if not (_hc_env_ok(LP, True) and _hc_env_ok(RP, False)) or LP.dtype != RP.dtype:
        return None
    if any(np.result_type(W.dtype, LP.dtype) != LP.dtype for W in Ws):
        return None
    Wd = [_plus_hc_W(getattr(W, '_tpa_origin', None) or W) for W in Ws]
    if any(W is None for W in Wd):
        return None
    store = env.__dict__ if env is not None else {}
    cache = store.setdefault('_plus_hc_cache', {})
    i0, n = op.i0, op.length
    LPd = _plus_hc_env(LP, True, cache, i0)
    RPd = _plus_hc_env(RP, False, cache, i0 + n - 1)
    if n == 2:
        factored = bool(getattr(op, 'factored', False))
        if factored and not factored_matvec_possible(LPd, RPd, *Wd):
            return None
        holder = _HeffCacheHolder(store.setdefault('_plus_hc_heff_cache', {}))
        inner = TwoSiteH(holder, i0, combine=True, move_right=op.move_right, tensors=(LPd, RPd, Wd[0], Wd[1]), factored=factored)
    else:
        inner = (OneSiteH if n == 1 else ZeroSiteH).__new__(OneSiteH if n == 1 else ZeroSiteH)
        inner.move_right = op.move_right
        inner._setup(LPd, Wd[0] if n == 1 else None, RPd, i0, op.dtype)
        if not inner.factored:
            return None
    return PlusHcH(op, inner)


class PlusHcH:
    """``H_eff + H_eff^dagger`` of a plain effective Hamiltonian as one operator: ``matvec``, ``matvec_program``, ``native_input`` and the
    flop / byte counts are those of the same class on the doubled tensors (``_plus_hc_operator``); everything else -- ``LP``, ``RP``,
    ``W0``, ``W1``, ``LHeff``, ``RHeff``, the pipes, ``combine_theta``, ``prepare_svd``, ``update_LP`` / ``update_RP``, ``i0``, ``length``,
    ``acts_on``, ``combine``, ``move_right`` -- is the plain operator's: the mixers add the h.c. part themselves (reference
    mps_common.py:2007, :2021, :2158, :2188), and the environments that are stored and updated are the plain ones."""

    def __init__(self, plain, doubled):
        self.plain = plain
        self.doubled = doubled

    def __getattr__(self, name):
        if name in ('plain', 'doubled'):            # (not yet set: unpickling / copy)
            raise AttributeError(name)
        return getattr(self.plain, name)

    def matvec(self, theta):
        labels = theta.get_leg_labels()
        res = self.doubled.matvec(theta)
        if list(res.get_leg_labels()) != list(labels):
            res.itranspose(labels)
        return res

    def matvec_program(self, theta):
        return self.doubled.matvec_program(theta)

    def native_input(self, theta, *args, **kwargs):
        return self.doubled.native_input(theta, *args, **kwargs)

    flops_per_matvec = property(lambda self: getattr(self.doubled, 'flops_per_matvec', None))
    bytes_per_matvec = property(lambda self: getattr(self.doubled, 'bytes_per_matvec', None))

    def adopt_plans(self, plans):
        """The contraction plans a driver keeps from visit to visit of a bond: those of the doubled tensors."""
        self.doubled.adopt_plans(plans)

    def plans_to_keep(self):
        return self.doubled.plans_to_keep()

    def adjoint(self):
        return self

    def plus_hc(self):
        raise ValueError("the operator is H + h.c. already")

    def to_matrix(self):
        """The plain matrix plus its adjoint, in the form the plain operator returns (host matrix or matrix Array)."""
        return _plus_adjoint_matrix(self.plain.to_matrix(), +1)


def _plus_adjoint_matrix(mat, keep):
    """``keep * mat + mat^dagger`` for a host matrix or a matrix Array with legs ``[x, x*]``."""
    if isinstance(mat, np.ndarray):
        return keep * mat + mat.conj().T
    adj = mat.conj().itranspose([1, 0])
    adj.iset_leg_labels(mat.get_leg_labels())
    return adj if keep == 0 else mat + adj


class AdjointH:
    """The Hermitian conjugate of a plain effective Hamiltonian as an operator of its own, for callers that use it alone (and for
    ``SumNpcLinearOperator(op, op.adjoint())`` where ``op.plus_hc()`` declines): the reference's contractions (mps_common.py:1146-1149,
    :1321-1348, :1512-1514) on the conjugated tensors of its ``adjoint()``, step by step, for ``theta`` with the labels of
    ``op.acts_on``.  Everything but the matvec is looked up on ``op``."""

    def __init__(self, op):
        self.op = op

    def __getattr__(self, name):
        if name == 'op':
            raise AttributeError(name)
        return getattr(self.op, name)

    def adjoint(self):
        return self.op

    def native_input(self, theta, *args, **kwargs):
        return None                 # (the launch program that `__getattr__` would hand out is the plain operator's)

    matvec_program = native_input

    def matvec(self, theta):
        op = self.op
        labels = list(theta.get_leg_labels())
        fused = op.length == 2 and theta.rank == 2
        if fused:
            theta = theta.split_legs()
        res = npc.tensordot(op.LP.conj().ireplace_label('wR*', 'wR'), theta, axes=['vR', 'vL'])
        for k, W in enumerate([W for W in (getattr(op, 'W0', None), getattr(op, 'W1', None)) if W is not None]):
            p = 'p%d' % k
            Wc = W.conj().ireplace_labels(['wL*', 'wR*'], ['wL', 'wR'])
            res = npc.tensordot(res, Wc, axes=[['wR', p], ['wL', p + '*']])
        res = npc.tensordot(res, op.RP.conj().ireplace_label('wL*', 'wL'), axes=[['wR', 'vR'], ['wL', 'vL']])
        res.ireplace_labels(['vR*', 'vL*'], ['vL', 'vR'])
        if fused:
            res = op.prepare_svd(res.transpose(['vL', 'p0', 'p1', 'vR']))
        return res.itranspose(labels)

    def to_matrix(self):
        return _plus_adjoint_matrix(self.op.to_matrix(), 0)
