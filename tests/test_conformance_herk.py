"""Conformance of ``tpa_herk_chain`` (csrc/tpa_herk.hip; both instantiations: real and complex data) with the extended-precision
statement of the header (tests/herk_reference.py), on the numpy emulation (``mock``, tests/mock_mixer.py) and on the HIP kernel (``gpu``).

Cases, canaries and the derivation of the tolerance: tests/conformance_herk_cases.py.  Shapes are the smallest at which each mechanism
can break: m in {1, 15, 16, 17, 63, 64, 65, 129} (one MFMA tile, the 64-row tile edge +- 1, three tiles per side: strictly lower,
diagonal and skipped tiles), k in {1, 3, 4, 5, 16, 17} per link (the MFMA k = 4 and the k-tile of 16, +- 1), chains of 1 to 7 live
links with an empty link at the start, in the middle or at the end."""
import numpy as np
import pytest

import conformance_herk_cases as ch
import kernel_reference as kref
import mock_mixer
from mixer_fixtures import mbackend  # noqa: F401
from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import _herk

DTYPES = [pytest.param(False, id='real'), pytest.param(True, id='complex')]


def _report(what, inst, n_cases, ratio):
    print("CONFORMANCE %s %s cases=%d max_err_over_bound=%.4f" % (what, inst, n_cases, ratio))


def test_herk_design_covers_the_mechanisms():
    """What the seeded cases contain (host only): every factor level, every (w_len, w_inner) of a periodic weight, exact zero and
    negative weights, Hermitian tasks with strictly lower, diagonal and skipped tiles, general tasks with and without a mirror, both
    operand layouts, ldc > n everywhere, both ways of passing the bases."""
    for cplx in (False, True):
        cs = list(ch.cases(cplx))
        assert len(cs) == 34
        links = np.concatenate([c.links for c in cs])
        live = links[links[:, 2] > 0]
        per = live[(live[:, 7] >= 0) & (live[:, 8] > 1)]
        assert {(a, b) for a, b in per[:, 8:10].tolist()} == {(a, b) for a in ch.W_LEN for b in ch.W_INNER}
        assert (live[:, 7] < 0).any() and ((live[:, 7] >= 0) & (live[:, 8] == 1)).any()
        wv = np.concatenate([c.w[np.isfinite(c.w)] for c in cs])
        assert (wv == 0.0).any() and (wv < 0).any()
        assert (live[:, 4] == 1).any() and (live[:, 3] == 1).any()          # k fast / row fast
        assert {c.split for c in cs} == {False, True}
        tasks = np.concatenate([c.tasks for c in cs])
        assert (tasks[:, 3] > tasks[:, 2]).all()                             # ldc > n
        assert ((tasks[:, 7] == 0) & (tasks[:, 8] >= 0)).any() and ((tasks[:, 7] == 0) & (tasks[:, 8] < 0)).any()
        assert set(tasks[tasks[:, 7] != 0][:, 6].tolist()) == {0, 1} and set(tasks[tasks[:, 7] == 0][:, 6].tolist()) == {0, 1}
        big = [c for c in cs if (c.tasks[:, 1] == 129).any()]
        for c in big:       # three tiles per side: 3 diagonal + 3 strictly lower tiles of the Hermitian 129 x 129 task, 3 skipped
            t = int(np.flatnonzero((c.tasks[:, 1] == 129) & (c.tasks[:, 7] != 0))[0])
            mine = c.tiles[c.tiles[:, 0] == t]
            assert len(mine) == 6 and (mine[:, 1] >= mine[:, 2]).all() and (mine[:, 1] > mine[:, 2]).sum() == 3
        assert big
        for c in cs:        # chains: empty links where the design says; 1 .. 7 live links
            nl = c.tasks[0, 5]
            assert 1 <= nl <= 8 and (c.links[:nl, 2] > 0).sum() <= 7


@pytest.mark.parametrize("cplx", DTYPES)
def test_herk_cases(mbackend, cplx):
    """Every case: the error bound per element, untouched guard zones / pad columns / gaps, Hermitian and mirror bits, a real diagonal,
    exact all-empty chains; every fourth case twice: identical bits."""
    worst, count = 0.0, 0
    for i, c in enumerate(ch.cases(cplx)):
        C = ch.run_case(c)
        worst = max(worst, ch.check_case(c, C))
        if i % 4 == 0:
            assert np.array_equal(kref.bits(ch.run_case(c)), kref.bits(C)), "two identical calls differ: " + c.label
        count += 1
    assert count == 34
    assert worst <= 1.0
    _report("tpa_herk_chain", 'complex' if cplx else 'real', count, worst)


@pytest.mark.parametrize("cplx", DTYPES)
def test_herk_tile_above_the_diagonal_is_ignored(mbackend, cplx):
    """Header: a Hermitian task is covered by its tiles on and below the diagonal; a tile above it is ignored."""
    rng = np.random.default_rng([ch.SEED, 7, int(cplx)])
    row = dict(m=129, lay='kfast', acc=0, k=17, live=2, empty='middle', weights='periodic')
    c = ch.make_case(cplx, row, rng, ch.tile_rows(cplx))
    C = ch.run_case(c)
    assert ch.check_case(c, C) <= 1.0
    t = int(np.flatnonzero((c.tasks[:, 1] == 129) & (c.tasks[:, 7] != 0))[0])
    c.tiles = np.concatenate([np.array([[t, 0, 2, 0], [t, 1, 2, 0]], np.int32), c.tiles])
    assert np.array_equal(kref.bits(ch.run_case(c)), kref.bits(C))


def test_herk_argument_errors(mbackend):
    """TPA_E_BADARG (-> ValueError) for a dtype that is neither F64 nor C128; n_tiles <= 0 returns 0 and writes nothing."""
    rng = np.random.default_rng([ch.SEED, 8])
    c = ch.make_case(False, dict(m=17, lay='kfast', acc=0, k=5, live=1, empty='none', weights='scalar'), rng, ch.tile_rows(False))
    d = [dev.to_device(x) for x in (c.tasks, c.links, c.tiles, c.A, c.w, c.C0)]
    L = dev.lib()

    def call(code, n_tiles):
        return L.tpa_herk_chain(code, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_tiles, d[3].data_ptr(), d[3].data_ptr(),
                                d[4].data_ptr(), d[5].data_ptr(), dev.stream())
    for code in (2, -1):
        with pytest.raises(ValueError):
            dev.check(call(code, len(c.tiles)), "herk_chain")
    for n_tiles in (0, -3):
        assert call(0, n_tiles) == 0
    assert np.array_equal(kref.bits(dev.to_host(d[5])), kref.bits(c.C0))
    _herk.herk_chain(np.float64, d[0], d[1], d[2], len(c.tiles), d[3], d[3], d[4], d[5])      # the product's own wrapper
    assert ch.check_case(c, dev.to_host(d[5])) <= 1.0


def test_herk_tile_table_longest_chains_first():
    tasks = np.array([_herk.task_row(0, 65, 65, 70, 0, 1, 0, 1), _herk.task_row(0, 65, 10, 70, 1, 2, 0, 0)], np.int64)
    links = np.array([_herk.link_row(0, 0, 5, 5, 1, 5, 1), _herk.link_row(0, 0, 4, 4, 1, 4, 1), _herk.link_row(0, 0, 3, 3, 1, 3, 1)], np.int64)
    tiles = _herk.tile_table(tasks, links, 64)
    assert tiles.dtype == np.int32 and tiles.tolist() == [[1, 0, 0, 0], [1, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [0, 1, 1, 0]]
    assert _herk.tile_table(tasks[:0], links, 64).shape == (0, 4)


# defect -> the checker that has to fire (a part of its message)
EXPECTED = {'no_weight': 'beyond the bound', 'no_conj': 'beyond the bound', 'w_inner_ignored': 'beyond the bound',
            'one_triangle': 'NaN / Inf in the output', 'mirror_rounded_again': 'in bits', 'diagonal_not_real': 'Im C[i,i] != 0'}


@pytest.mark.parametrize("defect", mock_mixer.DEFECTS)
def test_herk_checkers_reject_a_broken_emulation(monkeypatch, defect):
    """Sensitivity: the emulation with ONE deliberate defect is rejected, and by the checker that is there for it: the error bound
    for a dropped weight, a dropped conjugate (complex data) and an ignored w_inner; the NaN canary of an ``accumulate = 0`` block for
    a triangle that is not written; the bit comparison for a mirror that was rounded once more (one ulp: inside every bound -- only that comparison and
    the exactness of all-empty chains see it); the exact test of the diagonal for an imaginary part of rounding size.  The unbroken emulation passes the same cases."""
    mock_mixer.install(monkeypatch)
    cplx = defect in ('no_conj', 'diagonal_not_real')
    cs = list(ch.cases(cplx))[::2]
    for c in cs:
        ch.check_case(c, ch.run_case(c))
    monkeypatch.setattr(mock_mixer, 'DEFECT', defect)
    messages = []
    for c in cs:
        try:
            ch.check_case(c, ch.run_case(c))
        except AssertionError as e:
            messages.append(str(e))
    assert messages, defect
    assert any(EXPECTED[defect] in m for m in messages), (defect, sorted({m.split(':')[0] for m in messages}))
