"""The stand-alone ``MPS.mutinf_two_site`` / ``two_site_rho`` / ``one_site_rho`` against what the reference returned on the recorded
states of ``tests/golden/mutinf.pkl`` (``make_golden_mutinf.py``): XXZ with Sz conserved, the same state after complex TEBD steps, TFI
without a charge (sector width 2), the S = 1 chain without a charge (width 3) and Fermi-Hubbard with N and Sz (d = 4, ten slots per
row).  On the numpy emulation (``mock``) and on the MI355X (``gpu``).

Density matrices: 1e-12 absolute, the project's golden tolerance (entries are at most 1).

Mutual information: a bound DERIVED from the measured deviation of the density matrices, not a fixed number.  Let eta = (the largest
Frobenius deviation of rho_i, rho_j, rho_ij from the recorded ones) + 16 m 2^-53, m the matrix size (the second term: the eigenvalue
solvers of both sides).  By Weyl every eigenvalue moves by at most eta.  n = 1: f(x) = -x ln x has the modulus of continuity
|f(x) - f(y)| <= -eta ln eta for |x - y| <= eta <= 1 / e, and the three matrices have d_i + d_j + d_i d_j eigenvalues:
|dI| <= (d_i + d_j + d_i d_j) (-eta ln eta).  n = 2: S_2 = -ln P with the purity P = sum lambda^2 >= 1 / m; |dP| <= sum |d lambda|
(lambda + lambda') <= eta (2 + m eta), so |dS_2| = |ln(P' / P)| <= m eta (2 + m eta) / (1 - m eta (2 + m eta)), which for m eta <= 0.1
is below 2.1 m eta / 0.79 < 4 m eta: |dS_2| <= 4 m eta per entropy, three entropies per pair."""
import numpy as np
import pytest

from rho_fixtures import rbackend, state  # noqa: F401
from tenpy_amd.linalg.charges import ChargeInfo, LegCharge
from tenpy_amd.networks import rho as rho_mod
from tenpy_amd.networks.mps import MPS

TOL = 1.e-12
NAMES = ['xxz', 'xxz_tebd', 'tfi', 'spin1', 'hubbard']
U = 2.**-53


def bound(n, eta, di, dj):
    """The derived bound on |I - I_ref| for deviations eta = (eta_i, eta_j, eta_ij) of the three matrices (module docstring)."""
    if n == 1:
        e = max(eta[0] + 16 * di * U, eta[1] + 16 * dj * U, eta[2] + 16 * di * dj * U)
        assert e < np.exp(-1.)
        return (di + dj + di * dj) * (-e * np.log(e))
    total = 0.
    for m, e in ((di, eta[0]), (dj, eta[1]), (di * dj, eta[2])):
        e = e + 16 * m * U
        assert m * e <= 0.1
        total += 4 * m * e
    return total


@pytest.mark.parametrize("name", NAMES)
def test_density_matrices_match_the_reference(rbackend, name):
    rec, psi = state(name, rbackend)
    L = psi.L
    coords, rhos = psi.two_site_rho()
    want = [(i, j) for i in range(L) for j in range(i + 1, L)]
    assert coords.tolist() == [list(p) for p in want] and coords.dtype.kind == 'i'
    worst = 0.
    for (i, j), r in zip(want, rhos):
        ref = rec['rho2'][(i, j)]
        assert r.shape == ref.shape
        worst = max(worst, float(np.max(np.abs(r - ref))))
    rho1 = psi.one_site_rho()
    worst1 = max(float(np.max(np.abs(a - b))) for a, b in zip(rho1, rec['rho1']))
    print("MUTINF golden %s: max |rho_ij - ref| %.3g, max |rho_i - ref| %.3g" % (name, worst, worst1))
    assert worst <= TOL and worst1 <= TOL
    st = rho_mod.rho_stats
    assert st['device'] == 2 and st['generic'] == 0 and st['walks'] == 1 and st['d2h'] == 1 and st['kernel_launches'] > L


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("max_range", [None, 3])
@pytest.mark.parametrize("name", NAMES)
def test_mutual_information_matches_the_reference(rbackend, name, max_range, n):
    rec, psi = state(name, rbackend)
    ref_coords, ref_mi = rec['mutinf'][(max_range, n)]
    coords, mi = psi.mutinf_two_site(max_range=max_range, n=n)
    assert np.array_equal(coords, ref_coords) and mi.shape == ref_mi.shape
    _, rhos = psi.two_site_rho(max_range)
    rho1 = psi.one_site_rho()
    eta1 = [float(np.linalg.norm(a - b)) for a, b in zip(rho1, rec['rho1'])]
    worst = 0.
    for k, (i, j) in enumerate(coords.tolist()):
        di, dj = rho1[i].shape[0], rho1[j].shape[0]
        eta = (eta1[i], eta1[j], float(np.linalg.norm(rhos[k] - rec['rho2'][(i, j)])))
        lim = bound(n, eta, di, dj)
        err = abs(mi[k] - ref_mi[k])
        worst = max(worst, err / lim)
        assert err <= lim, "pair (%d, %d): |dI| = %.3g, bound %.3g" % (i, j, err, lim)
    print("MUTINF golden %s max_range=%s n=%d: worst |dI| / bound %.3g, max |dI| %.3g" % (name, max_range, n, worst, float(np.max(np.abs(mi - ref_mi)))))
    assert rho_mod.rho_stats['generic'] == 0


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", NAMES)
def test_nearest_neighbour_mutual_information(rbackend, name, n):
    """``max_range=1``: the pairs (i, i + 1) in order, each value within the same derived bound of the value the reference recorded
    for that pair with ``max_range=None`` (the reference computes a pair's value the same way whatever the range)."""
    rec, psi = state(name, rbackend)
    ref_coords, ref_mi = rec['mutinf'][(None, n)]
    ref = {tuple(c): v for c, v in zip(ref_coords.tolist(), ref_mi)}
    coords, mi = psi.mutinf_two_site(max_range=1, n=n)
    assert coords.tolist() == [[i, i + 1] for i in range(psi.L - 1)]
    _, rhos = psi.two_site_rho(1)
    rho1 = psi.one_site_rho()
    eta1 = [float(np.linalg.norm(a - b)) for a, b in zip(rho1, rec['rho1'])]
    for k, (i, j) in enumerate(coords.tolist()):
        dev_ = float(np.max(np.abs(rhos[k] - rec['rho2'][(i, j)])))
        assert dev_ <= TOL, "pair (%d, %d): |rho - ref| = %.3g" % (i, j, dev_)
        eta = (eta1[i], eta1[j], float(np.linalg.norm(rhos[k] - rec['rho2'][(i, j)])))
        lim = bound(n, eta, rho1[i].shape[0], rho1[j].shape[0])
        assert abs(mi[k] - ref[(i, j)]) <= lim, "pair (%d, %d): |dI| = %.3g, bound %.3g" % (i, j, abs(mi[k] - ref[(i, j)]), lim)
    assert rho_mod.rho_stats['generic'] == 0


def singlet_chain(pairs, L):
    """The stand-alone MPS of singlets on ``pairs`` (nested or disjoint bonds, every site in one pair), Sz conserved."""
    chinfo = ChargeInfo([1])
    p = LegCharge.from_qflat(chinfo, [[1], [-1]])
    from tenpy_amd.linalg import np_conserved as npc
    partner = {}
    for a, b in pairs:
        partner[a], partner[b] = b, a
    # bond k (left of site k): the open singlets as a list of left sites; state of the bond = the spins of those sites
    Bs, Ss = [], [np.ones(1)]
    open_sites = []
    for k in range(L):
        before = list(open_sites)
        if partner[k] > k:
            after = before + [k]
        else:
            after = [s for s in before if s != partner[k]]
        nb, na = 2**len(before), 2**len(after)
        T = np.zeros((nb, 2, na))
        for ib in range(nb):
            spins = {s: (ib >> n) & 1 for n, s in enumerate(before)}
            for sp in range(2):
                if partner[k] > k:
                    new = dict(spins)
                    new[k] = sp
                    amp = 1.
                else:
                    if spins[partner[k]] == sp:
                        continue
                    amp = (1. if sp == 1 else -1.)      # (|01> - |10>): the sign goes with the closing spin
                    new = {s: v for s, v in spins.items() if s != partner[k]}
                ia = sum(new[s] << n for n, s in enumerate(after))
                T[ib, sp, ia] = amp
        # right-canonical: sum_{p, a} T T^dagger = 1 on the left bond
        T /= np.sqrt(np.einsum('bpa,bpa->b', T, T))[:, None, None]

        def bond_leg(sites, qconj):
            q = [[sum(1 if (i >> n) & 1 == 0 else -1 for n, _ in enumerate(sites))] for i in range(2**len(sites))]
            return LegCharge.from_qflat(chinfo, q if sites else [[0]], qconj=qconj)
        Bs.append(npc.Array.from_ndarray(T, [bond_leg(before, +1), p, bond_leg(after, -1)], labels=['vL', 'p', 'vR'], cutoff=0.))
        Ss.append(np.ones(na) / np.sqrt(na))
        open_sites = after
    return MPS([p] * L, Bs, Ss, form='B')


def test_singlet_pairs(rbackend):
    """Singlets on (0, 3), (1, 2), (4, 5): I = 2 ln 2 on the pairs and 0 elsewhere, within the bound for the exact density matrices
    (maximally mixed sites; a singlet / the maximally mixed pair)."""
    pairs = [(0, 3), (1, 2), (4, 5)]
    psi = singlet_chain(pairs, 6)
    assert abs(psi.norm_test() - 1.) < 1e-14
    coords, mi = psi.mutinf_two_site()
    _, rhos = psi.two_site_rho()
    rho1 = psi.one_site_rho()
    s = np.zeros((2, 2, 2, 2))
    for a, b, sg in ((0, 1, 1.), (1, 0, -1.)):
        for c, e, sg2 in ((0, 1, 1.), (1, 0, -1.)):
            s[a, b, c, e] = 0.5 * sg * sg2
    mixed = np.einsum('ac,bd->abcd', np.eye(2), np.eye(2)) / 4.
    for k, (i, j) in enumerate(coords.tolist()):
        exact = s if (i, j) in pairs else mixed
        eta = (float(np.linalg.norm(rho1[i] - np.eye(2) / 2)), float(np.linalg.norm(rho1[j] - np.eye(2) / 2)),
               float(np.linalg.norm(rhos[k] - exact)))
        want = 2 * np.log(2.) if (i, j) in pairs else 0.
        assert abs(mi[k] - want) <= bound(1, eta, 2, 2), (i, j, mi[k])
    assert rho_mod.rho_stats['generic'] == 0 and rho_mod.rho_stats['device'] == 3
