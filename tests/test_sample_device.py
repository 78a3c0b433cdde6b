"""The batched sampling route on ground states from the stand-alone DMRG driver, on the numpy emulation (``mock``) and on the MI355X
(``gpu``): ``device_sample`` against the sample-by-sample statements (``sample_generic``) on the same uniforms, and the frequencies of
4096 samples against the dense ``|psi|^2``.

States: the XXZ chain L = 12 with Sz conserved, chi <= 32 (two-state sites, one charge), and the Fermi-Hubbard ladder 2 x 3 (L = 6
four-state sites, the two charges N and 2 Sz).  The seeds are fixed; on the emulation no uniform number of theirs lies closer than 1e-9
to an edge of the cdf (``sample_generic`` reports the margins; asserted on both backends), so the outcomes of the two routes, whose
probabilities differ by rounding errors of 1e-15, have to be equal."""
import numpy as np
import pytest

from sample_fixtures import sbackend  # noqa: F401
from tenpy_amd.networks import sample

U = 2.0**-53
_states = {}


def ground(kind, backend):
    """The state after three sweeps of two-site DMRG in the 'B' form, built once per backend."""
    if (kind, backend) not in _states:
        from tenpy_amd.algorithms.dmrg import TwoSiteDMRGEngine
        from tenpy_amd.networks.mps import MPS
        if kind == 'hubbard':
            from tenpy_amd.models.hubbard import hubbard_ladder_mpo, spinful_fermion_leg
            H, (_, p), init = hubbard_ladder_mpo(3, 1., 4., 0.), spinful_fermion_leg(), [1, 2] * 3
        else:
            from tenpy_amd.models.spin_chains import spin_half_leg, xxz_chain_mpo
            L = 12 if kind == 'xxz' else 6
            H, (_, p), init = xxz_chain_mpo(L, 1., 0.7, 0.), spin_half_leg('Sz'), [1, 0] * (L // 2)
        psi = MPS.from_product_state([p] * len(init), init)
        eng = TwoSiteDMRGEngine(psi, H, {'trunc_params': {'chi_max': 32, 'svd_min': 1e-10}})
        for _ in range(3):
            eng.sweep()
        # the sweeps leave the first sites in the 'A' form, whose conversion divides by small singular values: one sweep of QRs and
        # SVDs brings every site to the 'B' form, so that the state is normalised to 1e-12 site by site
        psi.compress_svd({'chi_max': 32, 'svd_min': 1e-10})
        _states[(kind, backend)] = psi
    return _states[(kind, backend)]


@pytest.mark.parametrize("kind,seed", [('xxz', 11), ('hubbard', 12)])
def test_device_route_against_the_generic_statements(sbackend, kind, seed):
    """n = 64 on the same uniforms: equal outcomes, every margin above 1e-9, weights within 16 n_sites u."""
    psi = ground(kind, sbackend)
    n, L = 64, psi.L
    assert psi.get_B(0, None).get_leg('p').ind_len == (4 if kind == 'hubbard' else 2) and psi.chinfo.qnumber == (2 if kind == 'hubbard' else 1)
    u = np.random.default_rng(seed).random((n, L))
    sig, _, w, phase = sample.device_sample(psi, n, L - 1, u)
    wts = sample._weights(w, phase, True, True)
    st = sample.sample_stats
    assert (st['walks'], st['tensordots'], st['select_launches'], st['gather_launches'], st['d2h']) == (1, L, L, L, L + 1)
    worst_margin, worst_err = 1., 0.
    for s in range(n):
        margins = []
        s_gen, w_gen = sample.sample_generic(psi, u=u[s], margins=margins)
        worst_margin = min(worst_margin, min(margins))
        assert list(s_gen) == sig[s].tolist(), (s, min(margins))
        worst_err = max(worst_err, abs(wts[s] - w_gen) / abs(w_gen))
    print("SAMPLE device %s: n=%d smallest margin %.3g, max rel err of a weight against the generic statements %.3g" % (kind, n, worst_margin, worst_err))
    assert worst_margin > 1.e-9
    assert worst_err <= 16 * L * U
    assert len(set(map(tuple, sig.tolist()))) > 8           # (not one string over and over)


def test_frequencies_against_the_dense_state(sbackend):
    """4096 samples of the XXZ ground state L = 6 (64 strings, 20 of them in the Sz = 0 sector): every string within 5 binomial
    standard deviations of 4096 |psi|^2, the strings outside the sector never; the weights are the amplitudes."""
    psi = ground('xxz6', sbackend)
    L, n = psi.L, 4096
    amp = psi.get_B(0, 'Th').to_ndarray()[0]                 # (p, vR)
    for i in range(1, L):
        amp = np.tensordot(amp, psi.get_B(i, 'B').to_ndarray(), axes=(-1, 0))
    amp = amp.reshape(-1)
    prob = np.abs(amp)**2
    assert abs(prob.sum() - 1) < 1e-12 and np.count_nonzero(prob > 1e-20) <= 20
    sig, wts = psi.sample_measurements(rng=np.random.default_rng(2024), n_samples=n)
    index = sig @ (2**np.arange(L - 1, -1, -1))
    counts = np.bincount(index, minlength=2**L)
    sd = np.sqrt(n * prob * (1 - prob))
    dev_sd = np.abs(counts - n * prob) / np.maximum(sd, 1e-300)
    print("SAMPLE frequencies: %d strings seen, largest deviation %.2f standard deviations" % (np.count_nonzero(counts), np.max(dev_sd[prob > 1e-20])))
    assert np.all(counts[prob <= 1e-20] == 0)
    assert np.all(np.abs(counts - n * prob) <= 5 * sd)
    assert np.max(np.abs(wts - amp[index])) <= 16 * L * U
    assert sample.sample_stats['walks'] == 1 and sample.sample_stats['select_launches'] == L
