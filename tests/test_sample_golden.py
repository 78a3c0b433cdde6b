"""The stand-alone ``MPS.sample_measurements`` against what the reference returned, call by call with one seeded generator, on the
recorded states of ``tests/golden/sample.pkl`` (``make_golden_sample.py``): XXZ with Sz conserved, spinless fermions with N conserved,
the TFI chain without a charge and the complex XXZ state after a quench.  On the numpy emulation (``mock``) and on the MI355X
(``gpu``).

Outcomes: equal exactly -- every recorded uniform lies at least 1e-6 from every edge of the cdf (the generator asserts it), the
probabilities carry errors of a few 1e-16.  Weights: within ``16 * max(e_ref, n_sites * u)`` relative, u = 2^-53: ``e_ref`` is the
recorded deviation of the reference's own weight from an extended-precision restatement, a product of n_sites correctly rounded
factors alone carries n_sites * u, and the factor 16 covers the different summation order of a tree reduction and the GEMM.  With
``ops`` the moduli are compared (the phase of an eigenvector is the eigensolver's choice).

With ``TPA_WRITE_PROFILES=1`` the measured deviations are written to ``profiles/sample_golden.txt`` when the last test of the module has run."""
import os

import numpy as np
import pytest

from sample_fixtures import build_psi, golden, sbackend  # noqa: F401
from tenpy_amd.networks import sample

U = 2.0**-53
NAMES = ['xxz', 'fermions', 'tfi', 'xxz_tebd']
_psi = {}
MEASURED = {}       # (backend, state, group) -> (device err, e_ref, bound)


@pytest.fixture(scope='module', autouse=True)
def _profile():
    yield
    if os.environ.get('TPA_WRITE_PROFILES') != '1' or not MEASURED:
        return
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'sample_golden.txt')
    lines = ["MPS.sample_measurements against tests/golden/sample.pkl: largest relative deviation of a weight (tests/test_sample_golden.py)",
             "(bound: 16 max(e_ref, n_sites 2^-53); e_ref: the reference's own deviation from an extended-precision restatement)", "",
             "%-8s %-10s %-6s %12s %12s %12s" % ("backend", "state", "group", "device", "e_ref", "bound")]
    lines += ["%-8s %-10s %-6s %12.3g %12.3g %12.3g" % (k + v) for k, v in sorted(MEASURED.items())]
    with open(path, 'w') as f:
        f.write("\n".join(lines) + "\n")


def state(name, backend):
    key = (name, backend)
    if key not in _psi:
        rec = [r for r in golden() if r['name'] == name][0]
        _psi[key] = (rec, build_psi(rec))
    return _psi[key]


def call(psi, rec, g, n_samples, rng, **over):
    kw = dict(last_site=g['kw']['last_site'], ops=None if g['kw']['ops'] is None else [rec['ops'][n] for n in g['kw']['ops']])
    kw.update(over)
    return psi.sample_measurements(0, rng=rng, n_samples=n_samples, **kw)


def rel_err(got, want, modulus):
    if modulus:
        got, want = np.abs(got), np.abs(want)
    return float(np.max(np.abs(got - want) / np.abs(want)))


@pytest.mark.parametrize("name", NAMES)
def test_batch_matches_the_recorded_reference_calls(sbackend, name):
    """One batch per group of recorded calls: all outcomes equal, all weights within the bound; served by the device route."""
    rec, psi = state(name, sbackend)
    for gname, g in rec['groups'].items():
        n, n_sites = g['u'].shape
        assert np.min(g['margins']) >= 1.e-6
        sig, wts = call(psi, rec, g, n, np.random.default_rng(g['seed']))
        assert sig.shape == (n, n_sites) and wts.shape == (n,)
        if gname == 'ops':
            assert np.max(np.abs(sig - g['sigmas'])) < 1.e-12
        else:
            assert sig.dtype.kind == 'i' and np.array_equal(sig, g['sigmas'])
        err = rel_err(wts, g['weights'], gname == 'ops')
        bound = 16 * max(g['e_ref'], n_sites * U)
        print("SAMPLE golden %s %s: n=%d max rel err of a weight %.3g (e_ref %.3g, bound %.3g)" % (name, gname, n, err, g['e_ref'], bound))
        MEASURED[(sbackend, name, gname)] = (err, g['e_ref'], bound)
        assert err <= bound
        assert np.iscomplexobj(wts) == np.iscomplexobj(g['weights'])
    assert sample.sample_stats['device'] == len(rec['groups']) and sample.sample_stats['generic'] == 0
    assert sample.sample_stats['select_launches'] > 0 and sample.sample_stats['gather_launches'] > 0


@pytest.mark.parametrize("name", NAMES)
def test_batch_is_the_single_calls_with_one_generator(sbackend, name):
    """A batch of 32 and 32 consecutive single-sample calls (``n_samples=None``: a list and a scalar) on generators with one seed:
    outcome for outcome the same, and both are the recorded calls; the weights agree within the bound above."""
    rec, psi = state(name, sbackend)
    g = rec['groups']['full']
    n, n_sites = g['u'].shape
    sig, wts = call(psi, rec, g, n, np.random.default_rng(g['seed']))
    rng = np.random.default_rng(g['seed'])
    singles = [call(psi, rec, g, None, rng) for _ in range(n)]
    assert all(isinstance(s, list) and len(s) == n_sites and np.ndim(w) == 0 for s, w in singles)
    assert np.array_equal(np.array([s for s, _ in singles]), sig) and np.array_equal(sig, g['sigmas'])
    one = np.array([w for _, w in singles])
    bound = 16 * max(g['e_ref'], n_sites * U)
    assert rel_err(one, wts, False) <= bound and rel_err(one, g['weights'], False) <= bound
    assert sample.sample_stats['device'] == n + 1 and sample.sample_stats['walks'] == n + 1


@pytest.mark.parametrize("name", ['xxz', 'xxz_tebd'])
def test_probability_instead_of_amplitude(sbackend, name):
    """``complex_amplitude=False``: the reference takes ``abs(total_weight)**2`` after EVERY site (mps.py:4439-4441 stands inside the
    loop); the route returns that number, rebuilt here from the recorded amplitudes' factors through the generic statements."""
    rec, psi = state(name, sbackend)
    g = rec['groups']['part']
    n, n_sites = g['u'].shape
    sig, prob = call(psi, rec, g, n, np.random.default_rng(g['seed']), complex_amplitude=False)
    assert np.array_equal(sig, g['sigmas']) and prob.dtype == np.float64
    for s in range(n):
        s_gen, p_gen = sample.sample_generic(psi, 0, g['kw']['last_site'], u=g['u'][s], complex_amplitude=False)
        assert list(s_gen) == list(sig[s])
        assert abs(prob[s] - p_gen) <= 2.**n_sites * 16 * n_sites * U * abs(p_gen)       # (n_sites nested squares double the relative error each)
    # one site: the plain square of the modulus of the weight
    sig1, p1 = call(psi, rec, g, n, np.random.default_rng(g['seed']), last_site=0, complex_amplitude=False)
    _, w1 = call(psi, rec, g, n, np.random.default_rng(g['seed']), last_site=0)
    assert np.array_equal(p1, np.abs(w1)**2)


def test_norm_tol_error_for_a_scaled_state(sbackend):
    """A state whose first tensor is scaled by 1 + 1e-6: ``ValueError('not normalized ...')`` as in the reference, from the batch and
    from a single-sample call; with ``norm_tol=1e-4`` the same state is sampled."""
    from measure_fixtures import build_psi as build
    rec, _ = state('xxz', sbackend)
    psi = build(rec)
    psi.set_B(0, psi.get_B(0, None) * (1. + 1.e-6), form=psi.form[0])
    for n in (4, None):
        with pytest.raises(ValueError, match='not normalized'):
            psi.sample_measurements(rng=np.random.default_rng(1), n_samples=n)
    sig, _ = psi.sample_measurements(rng=np.random.default_rng(1), n_samples=4, norm_tol=1.e-4)
    assert sig.shape == (4, psi.L)
    assert sample.sample_stats['generic'] == 0
