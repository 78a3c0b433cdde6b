"""Finite MPS of device-resident site tensors for the stand-alone drivers (``algorithms/dmrg.py``, ``tebd.py``, ``tdvp.py``)
on boxes without TeNPy.  It holds what those two drivers touch -- ``from_product_state``, ``get_B`` / ``set_B`` /
``get_theta`` / ``set_SL`` / ``set_SR`` with the reference's leg labels ``('vL', 'p', 'vR')`` and canonical-form convention
``B = S**nuL  Gamma  S**nuR`` ('A' = (1,0), 'B' = (0,1), 'Th' = (1,1)), ``expectation_value``, ``entanglement_entropy``.
With TeNPy installed, its own 7.6 kLoC ``MPS`` class (infinite systems, canonical forms, correlation functions, ...)
runs unchanged on the mirror (``tenpy_amd/install.py``).
"""
import numpy as np

from ..linalg import np_conserved as npc
from ..linalg.charges import LegCharge

__all__ = ['MPS', 'OverlapEnvironment']

_FORMS = {'A': (1., 0.), 'B': (0., 1.), 'C': (0.5, 0.5), 'G': (0., 0.), 'Th': (1., 1.), None: None}


class MPS:
    bc = 'finite'
    finite = True

    def __init__(self, p_legs, Bs, SVs, form='B'):
        self.p_legs = list(p_legs)          # physical leg of each site
        self.L = len(Bs)
        self._B = list(Bs)
        self._S = [np.asarray(s, dtype=np.float64) for s in SVs]   # L+1 Schmidt spectra, host
        self.form = [_FORMS[form]] * self.L
        self.chinfo = Bs[0].chinfo
        self.dtype = Bs[0].dtype
        self.norm = 1.

    @classmethod
    def from_product_state(cls, p_legs, p_state, dtype=np.float64):
        """Product state; ``p_state[i]`` is the flat physical index occupied on site i."""
        chinfo = p_legs[0].chinfo
        Bs = []
        q_left = chinfo.make_valid()
        for leg_p, occupied in zip(p_legs, p_state):
            qi, _ = leg_p.get_qindex(int(occupied))
            q_right = chinfo.make_valid(q_left + leg_p.get_charge(qi))
            vL = LegCharge.from_qflat(chinfo, [q_left], qconj=+1)
            vR = LegCharge.from_qflat(chinfo, [q_right], qconj=-1)
            dense = np.zeros((1, leg_p.ind_len, 1), dtype=dtype)
            dense[0, int(occupied), 0] = 1.
            Bs.append(npc.Array.from_ndarray(dense, [vL, leg_p, vR], dtype=dtype, labels=['vL', 'p', 'vR']))
            q_left = q_right
        return cls(p_legs, Bs, [np.ones(1)] * (len(p_legs) + 1), form='B')

    @property
    def chi(self):
        return [min(s.shape) if isinstance(s, npc.Array) else len(s) for s in self._S[1:-1]]

    def get_SL(self, i):
        return self._S[i]

    def get_SR(self, i):
        return self._S[i + 1]

    def set_SL(self, i, S):
        """1D singular values, or -- while a mixer is on -- the general 2D bond matrix (Array, labels 'vL', 'vR'; reference
        mps.py ``set_SL``), which is kept as it is."""
        self._S[i] = S if isinstance(S, npc.Array) else np.asarray(S)

    def set_SR(self, i, S):
        self._S[i + 1] = S if isinstance(S, npc.Array) else np.asarray(S)

    def set_B(self, i, B, form='B'):
        self._B[i] = B.transpose(['vL', 'p', 'vR']) if B._labels != ['vL', 'p', 'vR'] else B
        self.form[i] = _FORMS[form] if not isinstance(form, tuple) else form

    @staticmethod
    def _scaled(B, S, power, axis):
        if power == 0.:
            return B
        if isinstance(S, npc.Array):        # a 2D bond matrix multiplies; its inverse or root is not available (as in the reference)
            if power != 1.:
                raise ValueError("a 2D bond matrix S can only be applied with power +1, got %r" % (power,))
            if axis == 'vL':
                return npc.tensordot(S, B, axes=['vR', 'vL'])
            res = npc.tensordot(B, S, axes=['vR', 'vL'])
            return res.transpose(B.get_leg_labels()) if list(res.get_leg_labels()) != list(B.get_leg_labels()) else res
        return B.scale_axis(S if power == 1. else S**power, axis)

    def get_B(self, i, form='B', copy=False):
        """Site tensor converted to ``form``; ``form=None`` returns the stored tensor."""
        want = _FORMS[form] if not isinstance(form, tuple) else form
        B = self._B[i]
        if want is not None and want != self.form[i]:
            have = self.form[i]
            B = self._scaled(B, self._S[i], want[0] - have[0], 'vL')
            B = self._scaled(B, self._S[i + 1], want[1] - have[1], 'vR')
        elif copy:
            B = B.copy(deep=True)
        return B

    def get_theta(self, i, n=2, formL=1., formR=1.):
        """Wave function of ``n`` sites: ``n=2`` labels ``'vL', 'p0', 'p1', 'vR'``, ``n=1`` labels ``'vL', 'p0', 'vR'`` (reference
        mps.py:3041)."""
        if n == 1:
            return self.get_B(i, (formL, formR)).replace_label('p', 'p0')
        assert n == 2
        i1 = i + 1
        B0 = self._scaled(self._B[i], self._S[i], formL - self.form[i][0], 'vL')
        B0 = self._scaled(B0, self._S[i1], 1. - self.form[i][1] - self.form[i1][0], 'vR')
        B1 = self._scaled(self._B[i1], self._S[i1 + 1], formR - self.form[i1][1], 'vR')
        return npc.tensordot(B0.replace_label('p', 'p0'), B1.replace_label('p', 'p1'), axes=['vR', 'vL'])

    def expectation_value(self, op, sites=None):
        """``<psi| op_i |psi>`` for every site in ``sites`` (default: all): ``op`` is a dense (d, d) host matrix [p, p*] (must
        conserve the charges) or a device Array with labels 'p', 'p*' (reference ``MPS.expectation_value`` for one-site
        operators, mps.py).  One tensordot and one inner product per site on the device.

        ``op`` may also be a list (or tuple) of such operators: the result is then a list with one array per operator, from one
        ``tpa_site_inner_batch`` launch per site for all of them and one host read for the whole call (``networks/measure.py``) --
        or, where ``measure.decline_reason`` names a reason (counted in ``measure.measure_stats['why']``), from the statements of
        the one-operator form."""
        sites = range(self.L) if sites is None else sites
        if isinstance(op, (list, tuple)):
            from . import measure
            hosts = {}
            vals = measure.expectation_values(self, [self._site_ops(o, hosts) for o in op], list(sites), hosts)
            return [np.real_if_close(vals[:, k]) for k in range(len(op))]
        res = []
        for i in sites:
            th = self.get_B(i, 'Th')
            if isinstance(op, npc.Array):
                O = op
            else:
                leg = th.get_leg('p')
                O = npc.Array.from_ndarray(np.asarray(op), [leg, leg.conj()], labels=['p', 'p*'])
            C = npc.tensordot(O, th, axes=['p*', 'p'])
            res.append(npc.inner(th, C, axes='labels', do_conj=True))
        res = np.array(res)
        return np.real_if_close(res)

    def _site_ops(self, op, hosts=None):
        """``op`` (dense host matrix or device Array, 'p', 'p*') as one device Array per site; sites sharing a leg share the Array.
        ``hosts``: the call's table of host copies (``measure.as_site_op``)."""
        from . import measure
        made = {}
        for leg in self.p_legs:
            if id(leg) not in made:
                made[id(leg)] = measure.as_site_op(op, leg, hosts)
        return [made[id(leg)] for leg in self.p_legs]

    def correlation_function(self, op1, op2, sites1=None, sites2=None, opstr=None, str_on_first=True, hermitian=False):
        """``C[x, y] = <psi| op1_i op2_j |psi>`` for i = sites1[x], j = sites2[y] (default: all sites; both are sorted), a complex
        matrix unless all imaginary parts vanish (reference ``MPS.correlation_function``, mps.py:680-887).  The operators are dense
        (d, d) host matrices [p, p*] or device Arrays with the labels 'p', 'p*'; charged ones (Sp, Sm, Cd, C) are fine.  There are no
        site classes here, hence no ``autoJW``: a Jordan-Wigner string is passed as ``opstr``, which is applied on the sites between
        i and j and -- with ``str_on_first`` -- multiplied onto the operator of the smaller of the two sites, as in the reference.
        The diagonal is the expectation value of ``op1 . op2`` (``measure.expectation_values``); ``hermitian=True`` (only for sites1 == sites2) takes the lower
        triangle as the conjugate of the upper one, ``hermitian=False`` costs a second walk with the operators exchanged.
        The rows come from one stacked walk over the chain (``measure.corr_up`` / ``device_corr_up``) unless
        ``measure.decline_reason`` names a reason for the row-by-row statements (``measure.measure_stats['why']``)."""
        from . import measure
        sites1 = np.sort(np.arange(self.L) if sites1 is None else np.asarray(sites1, dtype=np.int64).reshape(-1))
        sites2 = np.sort(np.arange(self.L) if sites2 is None else np.asarray(sites2, dtype=np.int64).reshape(-1))
        for s in (sites1, sites2):
            if len(s) and (s[0] < 0 or s[-1] >= self.L):
                raise ValueError("site index out of range for a finite chain")
        hosts = {}
        ops1 = self._site_ops(op1, hosts)
        ops2 = self._site_ops(op2, hosts)
        strs = None if opstr is None else self._site_ops(opstr, hosts)
        if hermitian and not np.array_equal(sites1, sites2):
            hermitian = False
        C = np.zeros((len(sites1), len(sites2)), dtype=np.complex128)
        above = sites2[None, :] > sites1[:, None]
        up = measure.corr_up(self, ops1, ops2, sites1, sites2, strs, str_on_first, True, hosts=hosts)
        C[above] = up[above]
        below = sites1[:, None] > sites2[None, :]
        if hermitian:
            C[below] = np.conj(up).T[below]
        else:
            low = measure.corr_up(self, ops2, ops1, sites2, sites1, strs, str_on_first, False, hosts=hosts)      # [y, x]: the values with sites1[x] > sites2[y]
            C[below] = low.T[below]
        same = sites2[None, :] == sites1[:, None]
        if np.any(same):
            diag_sites = sorted(set(int(i) for i in sites1) & set(int(j) for j in sites2))
            prod = {}           # op1 . op2 once per pair of (shared) site operators; its host copy where both factors have one
            for i in range(self.L):
                key = (id(ops1[i]), id(ops2[i]))
                if key not in prod:
                    prod[key] = npc.tensordot(ops1[i], ops2[i], axes=['p*', 'p'])
                    if key[0] in hosts and key[1] in hosts:
                        hosts[id(prod[key])] = (prod[key], hosts[key[0]][1] @ hosts[key[1]][1])
            op12 = [prod[(id(ops1[i]), id(ops2[i]))] for i in range(self.L)]
            on_site = measure.expectation_values(self, [op12], diag_sites, hosts)[:, 0]       # one launch per site, one host read
            vals = dict(zip(diag_sites, on_site))
            for x, y in zip(*np.nonzero(same)):
                C[x, y] = vals[int(sites1[x])]
        return np.real_if_close(C)

    def sample_measurements(self, first_site=0, last_site=None, ops=None, rng=None, norm_tol=1.e-12, complex_amplitude=True, n_samples=None):
        """Projective measurements on the sites ``first_site .. last_site`` (default: to the end of the chain), the other sites traced
        out (reference ``MPS.sample_measurements``, mps.py:4349-4442).  ``ops``: a list of dense Hermitian (d, d) host matrices [p, p*]
        or device Arrays ('p', 'p*') -- there are no site classes here -- of which ``ops[(i - first_site) % len(ops)]`` is measured at
        site i and its eigenvalue returned; without ``ops`` the outcome is the index of the local basis state.  ``rng``: a
        ``numpy.random.Generator`` (default: a new one).  With ``n_samples=None`` the result is the reference's: ``(sigmas, weight)``,
        a list and a scalar -- ``weight`` the amplitude ``<sigmas|psi>`` with its phase for a whole chain, else the square root of the
        probability; with ``complex_amplitude=False`` the reference's ``abs(total_weight)**2``, which it takes after every site.  With
        ``n_samples=n`` it is ``(ndarray (n, n_sites), ndarray (n,))``, outcome for outcome what n consecutive single calls with
        the same generator return: the uniforms are ``rng.random((n, n_sites))``.

        A batch is carried through the chain as one stack, three device steps and one host read of 32 n bytes per site
        (``networks/sample.py``: ``device_sample``, ``tpa_sample_select_batch`` / ``tpa_sample_gather_batch``), unless
        ``sample.decline_reason`` names a reason for the sample-by-sample statements (``sample.sample_stats['why']``): ``first_site``
        inside the chain, a site wider than 64 states, ``TPA_SAMPLE=0``, and ``TPA_SAMPLE_SINGLE=0`` for a single-sample call."""
        from . import sample
        return sample.sample_measurements(self, first_site, last_site, ops, rng, norm_tol, complex_amplitude, n_samples)

    def mutinf_two_site(self, max_range=None, n=1):
        """``(coords, mutinf)``: the two-site mutual information ``I(i:j) = S(i) + S(j) - S(i, j)`` for all pairs with
        ``0 < j - i <= max_range`` (default: all), ``coords`` in the order ``for i: for j`` and ``n`` the entropy (1: von Neumann,
        else Renyi, ``numpy.inf`` included) -- reference ``MPS.mutinf_two_site``, mps.py:4180-4233.  The density matrices come from
        one stacked walk over the chain (``networks/rho.py``: ``device_two_site_rho``, ``tpa_site_rho_batch``) and the entropies from
        host eigenvalues per charge block, unless ``rho.decline_reason`` names a reason for the pair-by-pair statements
        (``rho.rho_stats['why']``): a physical sector wider than 4 states, ``TPA_MUTINF=0``."""
        from . import rho
        return rho.mutinf_two_site(self, max_range, n)

    def two_site_rho(self, max_range=None):
        """``(coords, rhos)``: the reduced density matrices of all pairs of sites with ``0 < j - i <= max_range`` as host arrays
        ``[p0, p1, p0*, p1*]`` (the reference's ``get_rho_segment([i, j])``, mps.py:3979-4023), ``coords`` as in
        ``mutinf_two_site``; from the stacked walk of ``networks/rho.py`` or, with a counted reason, pair by pair."""
        from . import rho
        why = rho.decline_reason(self)
        if why is None:
            rho.rho_stats['device'] += 1
            return rho.device_two_site_rho(self, max_range)
        rho.rho_stats['generic'] += 1
        rho._count_why(why)
        return rho.two_site_rho_generic(self, max_range)

    def one_site_rho(self):
        """The one-site density matrices ``[p0, p0*]`` of all sites as host arrays: one ``tpa_site_rho_batch`` launch per site and one
        host read for all of them (``rho.device_one_site_rho``) or, with a counted reason, site by site."""
        from . import rho
        why = rho.decline_reason(self)
        if why is None:
            rho.rho_stats['device'] += 1
            return rho.device_one_site_rho(self)
        rho.rho_stats['generic'] += 1
        rho._count_why(why)
        return rho.one_site_rho_generic(self)

    def copy(self):
        """Copy sharing the (immutable) tensors: the engines replace tensors, they never modify them in place."""
        res = MPS(self.p_legs, list(self._B), list(self._S), form='B')
        res.form = list(self.form)
        res.norm = self.norm
        return res

    def entanglement_entropy(self):
        res = []
        for s in self._S[1:-1]:
            if isinstance(s, npc.Array):    # the singular values of a 2D bond matrix
                s = np.asarray(npc.svd(s, compute_uv=False))
                s = s / np.linalg.norm(s)
            p = s[s > 1e-30]**2
            res.append(float(-np.sum(p * np.log(p))))
        return np.array(res)

    def compress_svd(self, trunc_par):
        """Compress in place with one sweep of QRs from the left end to the right one, without truncation, and one sweep of truncating
        SVDs back (reference mps.py:5895-5933, finite chains); ``MPO.apply`` calls it after the zip-up pass.  Returns the truncation
        error; ``norm`` is updated."""
        from ..linalg.truncation import TruncationError, svd_theta
        trunc_err = TruncationError()
        B = self.get_B(0, 'Th')
        for i in range(self.L - 1):
            q, r = npc.qr(B.combine_legs(['vL', 'p']), inner_labels=['vR', 'vL'])
            self.set_B(i, q.split_legs(), form=None)
            B = npc.tensordot(r, self.get_B(i + 1, 'B'), axes=('vR', 'vL'))
        for i in range(self.L - 1, 0, -1):
            U, S, VH, err, norm_new = svd_theta(B.combine_legs(['p', 'vR']), trunc_par)
            trunc_err = trunc_err + err
            self.norm *= norm_new
            self.set_B(i, VH.split_legs(), form='B')
            B = npc.tensordot(self.get_B(i - 1, None), U, axes=('vR', 'vL')).iscale_axis(S, 'vR')
            self.set_SL(i, S)
        self.set_B(0, B, form='Th')
        return trunc_err

    def norm_test(self):
        """<psi|psi> by contracting the transfer matrices (device tensordots)."""
        B = self.get_B(0, 'B')
        E = npc.tensordot(B.conj(), B, axes=(['vL*', 'p*'], ['vL', 'p']))
        for i in range(1, self.L):
            B = self.get_B(i, 'B')
            E = npc.tensordot(B.conj(), npc.tensordot(E, B, axes=['vR', 'vL']), axes=(['vL*', 'p*'], ['vR*', 'p']))
        return E.to_ndarray().reshape(-1)[0]


class OverlapEnvironment:
    """``<bra|ket>`` environments of a finite chain in the shape of ``MPOEnvironment``: ``LP[i]`` (labels ``'vR*', 'vR'``) is
    everything left of site i, ``RP[i]`` (``'vL', 'vL*'``) everything right of it; grown from the nearest stored part by
    ``npc.tensordot`` on demand (reference ``MPSEnvironment``, networks/mps.py).  The excited-state search of the stand-alone DMRG
    driver keeps one per state it stays orthogonal to (bra = the state being optimised)."""

    def __init__(self, bra, ket):
        self.bra, self.ket, self.L = bra, ket, bra.L
        self._LP = [None] * self.L
        self._RP = [None] * self.L
        one = np.ones((1, 1), dtype=np.result_type(bra.dtype, ket.dtype))
        self._LP[0] = npc.Array.from_ndarray(one, [bra.get_B(0, None).get_leg('vL'), ket.get_B(0, None).get_leg('vL').conj()],
                                             labels=['vR*', 'vR'])
        last = self.L - 1
        self._RP[last] = npc.Array.from_ndarray(one, [ket.get_B(last, None).get_leg('vR').conj(), bra.get_B(last, None).get_leg('vR')],
                                                labels=['vL', 'vL*'])

    def get_LP(self, i, store=True):
        i0 = max(j for j in range(i + 1) if self._LP[j] is not None)
        LP = self._LP[i0]
        for k in range(i0, i):
            LP = npc.tensordot(LP, self.ket.get_B(k, 'A'), axes=('vR', 'vL'))
            LP = npc.tensordot(self.bra.get_B(k, 'A').conj(), LP, axes=(['p*', 'vL*'], ['p', 'vR*']))      # 'vR*', 'vR'
            if store:
                self._LP[k + 1] = LP
        return LP

    def get_RP(self, i, store=True):
        i0 = min(j for j in range(i, self.L) if self._RP[j] is not None)
        RP = self._RP[i0]
        for k in range(i0, i, -1):
            RP = npc.tensordot(self.ket.get_B(k, 'B'), RP, axes=('vR', 'vL'))
            RP = npc.tensordot(RP, self.bra.get_B(k, 'B').conj(), axes=(['p', 'vL*'], ['p*', 'vR*']))       # 'vL', 'vL*'
            if store:
                self._RP[k - 1] = RP
        return RP

    def full_contraction(self):
        """``<bra|ket>`` (both normalised; ``MPS.norm`` is not looked at)."""
        k = self.L - 1
        LP = npc.tensordot(self.get_LP(k, store=False), self.ket.get_B(k, 'A'), axes=('vR', 'vL'))
        LP = npc.tensordot(self.bra.get_B(k, 'A').conj(), LP, axes=(['p*', 'vL*'], ['p', 'vR*']))
        return LP.to_ndarray().reshape(-1)[0]

    def invalidate(self, i0, i1):
        """After the bra's tensors of sites i0, i1 changed: drop every stored part that contains one of them."""
        for j in range(i1, self.L):
            self._LP[j] = None
        for j in range(i0, -1, -1):
            self._RP[j] = None
