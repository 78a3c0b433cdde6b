"""Generate the sampling fixtures from the REFERENCE implementation (TeNPy, pure-Python path): what its ``MPS.sample_measurements``
(networks/mps.py:4349-4442) returns, call by call with one seeded generator, on the small states of ``make_golden_measure.py``.

Run in the build container only (the reference tree does not exist on the GPU box):

    TENPY_NO_CYTHON=1 python tests/golden/make_golden_sample.py

Output (committed): ``tests/golden/sample.pkl`` -- plain dict / list / numpy content only.  A list of states -- the XXZ chain L = 8 with
Sz conserved, spinless fermions with N conserved, the TFI chain without a charge, the complex XXZ state after three TEBD steps -- each
with the tensors in the format of ``measure.pkl`` (``Bs``, ``forms``, ``S``, ``chinfo_mod``, ``complex``), the dense one-site operators
``ops`` by name, the ``seed`` and three groups of calls, each a dict with

* ``seed``     of ``numpy.random.default_rng`` handed to the reference for the consecutive calls of the group,
* ``kw``       ``last_site`` / ``ops`` (names) of the calls,
* ``u``        the uniforms ``default_rng(seed).random((calls, n_sites))`` -- ``Generator.choice`` draws exactly one ``random()`` per
               site, so these are the numbers the reference's calls consumed (asserted: the outcomes follow from them),
* ``sigmas``   ``[calls, n_sites]`` what the reference returned (indices; eigenvalues with ``ops``), ``weights`` ``[calls]``,
* ``margins``  ``[calls, n_sites]`` the distance of u from the nearest edge of the cdf (extended precision),
* ``e_ref``    the largest relative deviation of the reference's weight (its modulus with ``ops``: the phase of an eigenvector is
               the eigensolver's choice) from a ``np.longdouble`` restatement of the same loop on the dense tensors with the recorded
               outcomes.

Groups: ``full`` 32 calls over the whole chain; ``part`` 8 calls with ``last_site = 4``; ``ops`` (XXZ states: ``['Sz']``, TFI:
``['Sigmax', 'Sigmaz']``; operators that are non-degenerate inside every charge block) 8 calls.  The seed is walked until every margin
is >= 1e-6, so every recorded sample can be compared and none is skipped."""
import os
import pickle
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from oracle import build_ref  # noqa: E402  (where the reference lives)

sys.path.insert(0, build_ref.reference_root())
os.environ.setdefault('TENPY_NO_CYTHON', '1')
from make_golden_measure import L, ground_state  # noqa: E402
from make_golden_mpo_apply import dense  # noqa: E402
from tenpy.algorithms import tebd  # noqa: E402
from tenpy.models.fermions_spinless import FermionChain  # noqa: E402
from tenpy.models.spins import SpinChain  # noqa: E402
from tenpy.models.tf_ising import TFIChain  # noqa: E402

LD, CLD = np.longdouble, np.clongdouble
MARGIN = 1.e-6


def restate(psi, u, sigmas, last_site, op_mats):
    """The loop of the reference in extended precision on the dense tensors for the RECORDED outcomes: ``(weight, margins)``."""
    v = np.ones((1, 1), dtype=CLD)
    margins, weight = [], LD(1.)
    for k, i in enumerate(range(last_site + 1)):
        B = psi.get_B(i, 'Th' if i == 0 else 'B').copy().itranspose(['vL', 'p', 'vR']).to_ndarray().astype(CLD)
        x = np.tensordot(v[0], B, axes=(0, 0))              # (p, vR)
        if op_mats is not None:
            W, V = op_mats[k % len(op_mats)]
            x = V.conj().T.astype(CLD) @ x
            pick = int(np.argmin(np.abs(W - sigmas[k])))
            assert abs(W[pick] - sigmas[k]) < 1.e-12
        else:
            pick = int(sigmas[k])
        p = np.sum(x.real**2 + x.imag**2, axis=1)
        cdf = np.cumsum(p) / np.sum(p)
        edges = np.concatenate([[LD(0.)], cdf])
        # (with operators: ascending eigenvalues, which is the order of the reference's eigh for these operators)
        assert int(np.searchsorted(cdf, LD(u[k]), side='right')) == pick, "the recorded uniform does not give the recorded outcome"
        margins.append(float(np.min(np.abs(edges - LD(u[k])))))
        w = np.sqrt(p[pick])
        weight = weight * w
        v = (x[pick] / w)[None, :]
    if last_site == psi.L - 1:
        weight = weight * v[0, 0]
    return complex(weight), margins


def group(psi, seed, n_calls, last_site, op_names):
    rng = np.random.default_rng(seed)
    n_sites = (psi.L if last_site is None else last_site + 1)
    u = np.random.default_rng(seed).random((n_calls, n_sites))
    kw = dict(last_site=last_site, ops=op_names)
    op_mats = None
    if op_names is not None:
        op_mats = []
        for n in op_names:
            M = psi.sites[0].get_op(n).copy().itranspose(['p', 'p*']).to_ndarray()
            W, V = np.linalg.eigh(M)
            assert np.min(np.diff(W)) > 0.1, "degenerate measurement operator"
            op_mats.append((W, V))
    sig, wts, margins, e_ref = [], [], [], 0.
    for c in range(n_calls):
        s, w = psi.sample_measurements(0, last_site, ops=op_names, rng=rng)
        sig.append([float(x) for x in s] if op_names is not None else [int(x) for x in s])
        wts.append(complex(w))
        w_ld, m = restate(psi, u[c], sig[-1], n_sites - 1, op_mats)
        margins.append(m)
        if op_names is not None:
            e_ref = max(e_ref, abs(abs(w) - abs(w_ld)) / abs(w_ld))
        else:
            e_ref = max(e_ref, abs(w - w_ld) / abs(w_ld))
    assert rng.random() == np.random.default_rng(seed).random((n_calls, n_sites + 1)).reshape(-1)[n_calls * n_sites], \
        "the reference drew more than one number per site"
    wts = np.array(wts)
    if np.all(wts.imag == 0):
        wts = wts.real
    return dict(seed=seed, kw=kw, u=u, sigmas=np.array(sig), weights=wts, margins=np.array(margins), e_ref=float(e_ref))


def record(name, psi, op_names, measured):
    site = psi.sites[0]
    ops = {n: site.get_op(n).copy().itranspose(['p', 'p*']).to_ndarray() for n in op_names}
    rec = dict(name=name, L=psi.L, chinfo_mod=np.array(psi.chinfo.mod), complex=bool(psi.dtype.kind == 'c'),
               Bs=[dense(psi.get_B(i, None), ['vL', 'p', 'vR']) for i in range(psi.L)], forms=[tuple(f) for f in psi.form],
               S=[np.array(psi.get_SL(i)) for i in range(psi.L)] + [np.array(psi.get_SR(psi.L - 1))], ops=ops)
    seed = 1000
    while True:
        groups = dict(full=group(psi, seed, 32, None, None), part=group(psi, seed + 1, 8, 4, None))
        if measured is not None:
            groups['ops'] = group(psi, seed + 2, 8, None, measured)
        if min(float(np.min(g['margins'])) for g in groups.values()) >= MARGIN:
            break
        seed += 10
    rec.update(seed=seed, groups=groups)
    print(name, 'chi', psi.chi, 'dtype', psi.dtype, 'seed', seed, 'min margin %.3g' % min(float(np.min(g['margins'])) for g in groups.values()),
          'e_ref', {k: '%.3g' % g['e_ref'] for k, g in groups.items()})
    return rec


def main():
    out = []
    hz = 0.5 * (-1.)**np.arange(L)
    xxz = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=hz, conserve='Sz', bc_MPS='finite', sort_charge=True))
    psi = ground_state(xxz, ['up', 'down'])
    out.append(record('xxz', psi, ['Sz'], ['Sz']))
    fer = FermionChain(dict(L=L, J=1., V=0.5, mu=0., conserve='N', bc_MPS='finite'))
    out.append(record('fermions', ground_state(fer, ['full', 'empty']), ['N'], None))
    tfi = TFIChain(dict(L=L, J=1., g=1.3, conserve=None, bc_MPS='finite'))
    out.append(record('tfi', ground_state(tfi, ['up', 'up']), ['Sigmax', 'Sigmaz'], ['Sigmax', 'Sigmaz']))
    psi_c = psi.copy()           # a quench: the ground state in the staggered field evolves under the chain without it
    xxz0 = SpinChain(dict(L=L, S=0.5, Jx=1., Jy=1., Jz=0.7, hz=0., conserve='Sz', bc_MPS='finite', sort_charge=True))
    tebd.TEBDEngine(psi_c, xxz0, {'dt': 0.1, 'order': 2, 'N_steps': 3, 'trunc_params': {'chi_max': 16, 'svd_min': 1.e-10}}).run()
    assert psi_c.dtype.kind == 'c'
    out.append(record('xxz_tebd', psi_c, ['Sz'], ['Sz']))
    return out


if __name__ == '__main__':
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = main()
    path = os.path.join(HERE, 'sample.pkl')
    with open(path, 'wb') as f:
        pickle.dump(out, f, protocol=4)
    print("wrote sample.pkl", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1000000
