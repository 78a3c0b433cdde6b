"""Finite MPO and MPO environments for the stand-alone drivers (boxes without TeNPy): ``MPO`` (list of W with labels
``'wL','wR','p','p*'``), ``mpo_from_dense`` (charges of the virtual legs deduced from the entries) and ``MPOEnvironment`` with
cached ``LP`` / ``RP`` (labels ``'vR*','wR','vR'`` and ``'vL','wL','vL*'``; ``_contract_LP`` / ``_contract_RP`` as reference
networks/mpo.py:3087-3105).  Everything is a device tensordot; at chi=2048 all L environments (~100 x 2 x 35 MB) stay resident
in HBM instead of the reference's disk cache.  With TeNPy installed its own classes run on the mirror.
"""
import numpy as np

from ..linalg import np_conserved as npc
from ..linalg.charges import LegCharge

__all__ = ['MPO', 'MPOEnvironment', 'mpo_from_dense']


class MPO:
    bc = 'finite'
    finite = True

    def __init__(self, p_legs, Ws, IdL=0, IdR=-1, explicit_plus_hc=False):
        self.explicit_plus_hc = bool(explicit_plus_hc)      # the tensors hold half of H: the operator is this MPO plus its h.c. (reference mpo.py:170)
        self.p_legs = list(p_legs)
        self._W = list(Ws)
        self.L = len(Ws)
        self.IdL, self.IdR = IdL, IdR
        self.chinfo = Ws[0].chinfo
        self.dtype = Ws[0].dtype

    def get_W(self, i):
        return self._W[i]

    @property
    def chi(self):
        return [W.get_leg('wL').ind_len for W in self._W] + [self._W[-1].get_leg('wR').ind_len]

    def _zipup_IdL(self, i):
        """Index of the "only identities to the left" state on the bond left of site i (one number for all bonds, or one per bond)."""
        Id = self.IdL[i] if isinstance(self.IdL, (list, tuple)) else self.IdL
        return Id % self._W[i].get_leg('wL').ind_len

    def _zipup_IdR(self, i):
        """Index of the "only identities to the right" state on the bond right of site i."""
        Id = self.IdR[i + 1] if isinstance(self.IdR, (list, tuple)) else self.IdR
        return Id % self._W[i].get_leg('wR').ind_len

    def expectation_value(self, psi, tol=1.e-10, max_range=100, init_env_data={}):
        """``<psi|self|psi>`` of a finite chain, ignoring ``psi.norm`` (reference mpo.py:1111-1171; ``tol`` and ``max_range`` concern
        infinite chains only).  One walk on the device (``networks/moments.py``); where ``moments.decline_reason`` names a reason
        (counted in ``moments.moments_stats['why']``), the reference's statements: ``MPOEnvironment.full_contraction``."""
        from . import moments
        return moments.expectation_value(psi, self, lambda: moments.expectation_value_generic(psi, self), init_env_data)[0]

    def variance(self, psi, exp_val=None):
        """``<psi|self^2|psi> - <psi|self|psi>^2`` of a finite chain, ignoring ``psi.norm`` (reference mpo.py:1296-1342).  ``exp_val``:
        ``<psi|self|psi>`` if known (0 gives ``<psi|self^2|psi>`` alone); ``None``: both moments come from the same walk
        (``networks/moments.py``).  A declined call runs the reference's statements."""
        from . import moments
        if self.bc != 'finite':
            raise ValueError("works only for finite systems")
        if self.L != psi.L:
            raise ValueError("expect same L")
        if getattr(psi, '_p_label', ['p']) != ['p']:
            raise NotImplementedError("not adjusted for non-standard MPS.")
        if self.explicit_plus_hc:
            raise NotImplementedError("not implemented for explicit_plus_hc flag")

        def generic():
            return moments.variance_generic(psi, self, self.expectation_value(psi) if exp_val is None else exp_val)
        return moments.variance(psi, self, exp_val, generic)[0]

    def apply(self, psi, options):
        """Apply the MPO to ``psi`` in place and compress it (reference mpo.py:1562-1609): ``compression_method='zip_up'`` is the one
        method served -- ``apply_zipup``, then ``psi.compress_svd(trunc_params)``.  Returns the summed truncation error."""
        method = options['compression_method']
        if method != 'zip_up':
            raise ValueError("compression_method %r is not served: this driver serves 'zip_up'" % (method,))
        trunc_err = self.apply_zipup(psi, options)
        return trunc_err + psi.compress_svd(options['trunc_params'])

    def apply_zipup(self, psi, options):
        """One left-to-right pass of the zip-up method (reference mpo.py:1679-1767): every site's ``W . B`` with the ``VH`` of the site
        before is decomposed with the relaxed truncation ``chi_max * m_temp`` (``svd_min * trunc_weight``).  Interior sites build their
        matrix by ``mps_common.device_zipup_step`` (one GEMM over chi and the MPO step on the device); the two boundary sites, and
        interior sites the device route declines, run the reference's statements.  ``psi`` is afterwards only approximately canonical
        (``apply`` compresses it).  Options: ``trunc_params``, ``m_temp`` (2), ``trunc_weight`` (1.).  Returns the truncation error;
        ``psi.norm`` is updated."""
        from ..algorithms.mps_common import device_zipup_step
        from ..linalg.truncation import TruncationError, svd_theta
        m_temp, trunc_weight = int(options.get('m_temp', 2)), float(options.get('trunc_weight', 1.))
        relax_trunc = dict(options['trunc_params'])
        relax_trunc['chi_max'] *= m_temp
        if 'svd_min' in relax_trunc:
            relax_trunc['svd_min'] *= trunc_weight
        if psi.L != self.L:
            raise ValueError('Length of MPS and MPO not the same')
        if self.explicit_plus_hc:
            raise NotImplementedError("Can't use explicit_plus_hc with apply_zipup")
        trunc_err = TruncationError()
        VH = None
        for i in range(psi.L):
            W, last = self.get_W(i), i == psi.L - 1
            M = device_zipup_step(VH, psi.get_B(i, 'B'), W) if 0 < i and not last else None
            if M is None:
                M = npc.tensordot(psi.get_B(i, 'B'), W, axes=('p', 'p*'))
                if i == 0:
                    M = M.take_slice(self._zipup_IdL(i), 'wL')
                else:
                    M = npc.tensordot(VH, M, axes=(['wR', 'vR'], ['wL', 'vL']))
                if last:
                    M = M.take_slice(self._zipup_IdR(i), 'wR').combine_legs(['vL', 'p'], qconj=[-1])
                else:
                    M = M.combine_legs([['vL', 'p'], ['wR', 'vR']], qconj=[+1, -1])
            U, S, VH, err, norm_new = svd_theta(M, relax_trunc, [M.qtotal, None] if last else [None, None])
            trunc_err = trunc_err + err
            psi.norm *= norm_new
            if not last:
                VH = VH.split_legs().iscale_axis(S, 'vL')
            psi.set_SR(i, S)
            psi.set_B(i, U.split_legs(), 'A')
        return trunc_err


def mpo_from_dense(W_dense_list, p_legs, chinfo, dtype=np.float64, IdL=0, IdR=-1, explicit_plus_hc=False):
    """Build a finite MPO from dense ``W[i]`` of shape (D_l, D_r, d, d).  The charges of the virtual MPO legs are deduced
    from the non-zero entries (every entry must conserve charge) in two passes: forward from the left boundary (index
    ``IdL`` of the first leg = charge 0) and backward from the right boundary (index ``IdR`` of the last leg = charge 0).
    An index that neither pass reaches cannot contribute to any contraction; its entries are dropped.  An index reached
    from one side only is kept: e.g. the "only identities to the right" state on the bond right of the first site when
    no one-site term exists -- the subspace expansion relies on ``W[IdR, IdR] = 1`` being there on every site."""
    L = len(W_dense_list)
    Ws_d = [np.array(Wd) for Wd in W_dense_list]
    nq = chinfo.qnumber
    pqs = [p.to_qflat() * p.qconj for p in p_legs]

    def entries(Wd):
        nz = np.abs(Wd) > 1e-15
        out = {}
        for a, b, s, t in np.argwhere(nz):
            out.setdefault((int(a), int(b)), (int(s), int(t)))       # first non-zero physical entry of each (a, b)
        return out
    ents = [entries(Wd) for Wd in Ws_d]
    # charge rule of an entry: q_a - q_b + p[s] - p[t] = 0
    fq = [np.zeros((Ws_d[0].shape[0], nq), dtype=np.int64)]
    fk = [np.zeros(Ws_d[0].shape[0], dtype=bool)]
    fk[0][IdL % Ws_d[0].shape[0]] = True
    if Ws_d[0].shape[0] == 1:
        fk[0][:] = True
    for i in range(L):
        Dr = Ws_d[i].shape[1]
        q, k = np.zeros((Dr, nq), dtype=np.int64), np.zeros(Dr, dtype=bool)
        for (a, b), (s_, t_) in sorted(ents[i].items()):
            if not fk[i][a]:
                continue
            qb = chinfo.make_valid(fq[i][a] + pqs[i][s_] - pqs[i][t_])
            if k[b] and np.any(q[b] != qb):
                raise ValueError("MPO entry (%d,%d) on site %d violates charge conservation" % (a, b, i))
            q[b], k[b] = qb, True
        fq.append(q)
        fk.append(k)
    bq = [None] * (L + 1)
    bk = [None] * (L + 1)
    Dlast = Ws_d[-1].shape[1]
    bq[L], bk[L] = np.zeros((Dlast, nq), dtype=np.int64), np.zeros(Dlast, dtype=bool)
    bk[L][IdR % Dlast] = True
    if Dlast == 1:
        bk[L][:] = True
    for i in range(L - 1, -1, -1):
        Dl = Ws_d[i].shape[0]
        q, k = np.zeros((Dl, nq), dtype=np.int64), np.zeros(Dl, dtype=bool)
        for (a, b), (s_, t_) in sorted(ents[i].items()):
            if not bk[i + 1][b]:
                continue
            qa = chinfo.make_valid(bq[i + 1][b] - pqs[i][s_] + pqs[i][t_])
            if k[a] and np.any(q[a] != qa):
                raise ValueError("MPO entry (%d,%d) on site %d violates charge conservation" % (a, b, i))
            q[a], k[a] = qa, True
        bq[i], bk[i] = q, k
    bond_q, bond_k = [], []
    for j in range(L + 1):
        both = fk[j] & bk[j]
        if np.any(fq[j][both] != bq[j][both]):
            raise ValueError("MPO charges deduced from the left and from the right disagree on bond %d" % j)
        bond_q.append(np.where(fk[j][:, None], fq[j], bq[j]))
        bond_k.append(fk[j] | bk[j])
    Ws = []
    for i, Wd in enumerate(Ws_d):
        Wd[~bond_k[i]] = 0.
        Wd[:, ~bond_k[i + 1]] = 0.
        p = p_legs[i]
        wL = LegCharge.from_qflat(chinfo, chinfo.make_valid(bond_q[i]), qconj=+1)
        wR = LegCharge.from_qflat(chinfo, chinfo.make_valid(bond_q[i + 1]), qconj=-1)
        W = npc.Array.from_ndarray(Wd, [wL, wR, p, p.conj()], dtype=dtype, qtotal=None if nq == 0 else chinfo.make_valid(),
                                   labels=['wL', 'wR', 'p', 'p*'])
        Ws.append(W)
    return MPO(p_legs, Ws, IdL, IdR, explicit_plus_hc=explicit_plus_hc)


class MPOEnvironment:
    """``<psi| H |psi>`` environments of a finite chain; ``LP[i]`` is everything left of site i, ``RP[i]`` everything right
    of it."""

    def __init__(self, psi, H):
        self.psi = self.ket = self.bra = psi
        self.H = H
        self.L = psi.L
        self.dtype = np.result_type(psi.dtype, H.dtype)
        self._LP = [None] * self.L
        self._RP = [None] * self.L
        self._heff_cache = {}        # (side, site) -> (env tensor, fused Heff, pipe); see TwoSiteH.combine_Heff
        self._LP[0] = self._boundary(0, left=True)
        self._RP[self.L - 1] = self._boundary(self.L - 1, left=False)

    def _boundary(self, i, left):
        B, W = self.psi.get_B(i, None), self.H.get_W(i)
        leg_ket = B.get_leg('vL' if left else 'vR')
        leg_mpo = W.get_leg('wL' if left else 'wR').conj()
        dense = np.zeros((leg_ket.ind_len, leg_mpo.ind_len, leg_ket.ind_len), dtype=self.dtype)
        idx = (self.H.IdL if left else self.H.IdR) % leg_mpo.ind_len
        dense[np.arange(leg_ket.ind_len), idx, np.arange(leg_ket.ind_len)] = 1.
        if left:
            return npc.Array.from_ndarray(dense, [leg_ket, leg_mpo, leg_ket.conj()], dtype=self.dtype, labels=['vR*', 'wR', 'vR'])
        return npc.Array.from_ndarray(dense, [leg_ket.conj(), leg_mpo, leg_ket], dtype=self.dtype, labels=['vL', 'wL', 'vL*'])

    def get_LP(self, i, store=True):
        """LP left of site i, grown from the nearest stored one."""
        i0 = max(j for j in range(i + 1) if self._LP[j] is not None)
        LP = self._LP[i0]
        for k in range(i0, i):
            LP = self._contract_LP(k, LP)
            if store:
                self._LP[k + 1] = LP
        return LP

    def get_RP(self, i, store=True):
        i0 = min(j for j in range(i, self.L) if self._RP[j] is not None)
        RP = self._RP[i0]
        for k in range(i0, i, -1):
            RP = self._contract_RP(k, RP)
            if store:
                self._RP[k - 1] = RP
        return RP

    def set_LP(self, i, LP, age=None):
        self._LP[i] = LP

    def set_RP(self, i, RP, age=None):
        self._RP[i] = RP

    def invalidate(self, i0, i1, keep_LP, keep_RP):
        """After the tensors of sites i0, i1 changed: drop every stored part that contains one of them, except the one the
        bond update has just computed itself (``LP[i1]`` when moving right, ``RP[i0]`` when moving left)."""
        for j in range(i1 + (1 if keep_LP else 0), self.L):
            if j > 0:
                self._LP[j] = None
        for j in range(i0 - (1 if keep_RP else 0), -1, -1):
            if j < self.L - 1:
                self._RP[j] = None

    def _contract_LP(self, i, LP):
        """LP(i+1) from LP(i): contract with A[i], W[i], A*[i]  (reference mpo.py:3087)."""
        A = self.psi.get_B(i, 'A')
        LP = npc.tensordot(LP, A, axes=('vR', 'vL'))
        LP = npc.tensordot(self.H.get_W(i), LP, axes=(['p*', 'wL'], ['p', 'wR']))
        return npc.tensordot(A.conj(), LP, axes=(['p*', 'vL*'], ['p', 'vR*']))      # 'vR*', 'wR', 'vR'

    def _contract_RP(self, i, RP):
        """RP(i-1) from RP(i): contract with B[i], W[i], B*[i]  (reference mpo.py:3097)."""
        B = self.psi.get_B(i, 'B')
        RP = npc.tensordot(B, RP, axes=('vR', 'vL'))
        RP = npc.tensordot(RP, self.H.get_W(i), axes=(['p', 'wL'], ['p*', 'wR']))
        return npc.tensordot(RP, B.conj(), axes=(['p', 'vL*'], ['p*', 'vR*']))       # 'vL', 'wL', 'vL*'

    def full_contraction(self, i0):
        """<psi|H|psi> evaluated at bond (i0, i0+1)."""
        LP = self.get_LP(i0 + 1, store=False)
        S = self.psi.get_SR(i0)
        RP = self.get_RP(i0, store=False)
        LP = LP.scale_axis(S, 'vR').scale_axis(np.conj(S), 'vR*')
        res = npc.inner(LP, RP, axes=(['vR*', 'wR', 'vR'], ['vL*', 'wL', 'vL']), do_conj=False)
        if getattr(self.H, 'explicit_plus_hc', False):
            res = res + np.conj(res)        # (reference mpo.py:3083)
        return res
