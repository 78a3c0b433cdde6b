"""``tpa_unit_defect_batch``: the largest ``|B - 1|`` entry over a list of square blocks, exact (a maximum, no sums), against numpy's
maximum.  Blocks of n in {1, 31, 64, 100} with a leading dimension wider than n, NaN between and behind the rows of a block."""
import numpy as np
import pytest

from tenpy_amd.linalg import _device as dev
from tenpy_amd.linalg import np_conserved as npc

NS = (1, 31, 64, 100)


@pytest.fixture(params=["mock", pytest.param("gpu", marks=pytest.mark.gpu)])
def dbackend(request, monkeypatch):
    from tenpy_amd import _lib
    npc.clear_device_caches()
    if request.param == "mock":
        import mock_device_ex
        mock_device_ex.install(monkeypatch)
    else:
        _lib.require_gpu()
    yield request.param
    npc.clear_device_caches()


def _blocks(rng, cplx=False):
    """-> (arena, jobs, views): unit matrices in a NaN-filled arena."""
    jobs, size = [], 7
    for n in NS:
        ld = n + int(rng.integers(0, 5))
        jobs.append([size, n, ld, 0])
        size += n * ld + 11
    arena = np.full(size, np.nan, dtype=np.complex128 if cplx else np.float64)
    views = []
    for off, n, ld, _ in jobs:
        v = np.lib.stride_tricks.as_strided(arena[off:], shape=(n, n), strides=(ld * arena.itemsize, arena.itemsize))
        v[...] = np.eye(n)
        views.append(v)
    return arena, np.array(jobs, dtype=np.int64), views


def _defect(arena, jobs):
    d_arena, d_jobs = dev.to_device(arena), dev.to_device(jobs)
    out = dev.to_device(np.array([123.0]))
    dev.check(dev.lib().tpa_unit_defect_batch(dev.code(arena.dtype), d_jobs.data_ptr(), len(jobs), d_arena.data_ptr(), out.data_ptr(),
                                              dev.stream()), "unit_defect")
    return float(dev.to_host(out)[0])


def test_unit_matrices_give_zero(dbackend):
    arena, jobs, _ = _blocks(np.random.default_rng(1))
    assert _defect(arena, jobs) == 0.0
    assert _defect(arena, jobs[:0]) == 0.0
    for j in range(len(NS)):
        assert _defect(arena, jobs[j:j + 1]) == 0.0


@pytest.mark.parametrize("where", ['diagonal', 'off_diagonal', 'last_row', 'last_column', 'everywhere'])
def test_planted_deviation_comes_back_exactly(dbackend, where):
    rng = np.random.default_rng([2, len(where)])
    for b, n in enumerate(NS):
        arena, jobs, views = _blocks(rng)
        v = views[b]
        eps = float(rng.uniform(1e-15, 1e-9))
        if where == 'diagonal':
            i = int(rng.integers(n))
            v[i, i] += eps
        elif where == 'off_diagonal':
            if n == 1:
                continue
            i = int(rng.integers(n - 1))
            v[i + 1, i] = -eps
        elif where == 'last_row':
            v[n - 1, int(rng.integers(n))] += eps
        elif where == 'last_column':
            v[int(rng.integers(n)), n - 1] -= eps
        else:
            for w in views:
                w += rng.uniform(-1e-12, 1e-12, size=w.shape)
        want = max(float(np.max(np.abs(w - np.eye(len(w))))) for w in views)
        assert want > 0
        assert _defect(arena, jobs) == want


def test_nan_is_not_dropped(dbackend):
    arena, jobs, views = _blocks(np.random.default_rng(3))
    views[2][5, 7] = np.nan
    assert _defect(arena, jobs) == np.inf


def test_complex_blocks(dbackend):
    rng = np.random.default_rng(4)
    arena, jobs, views = _blocks(rng, cplx=True)
    assert _defect(arena, jobs) == 0.0
    views[1][3, 4] = 3e-11 - 4e-11j
    views[3][99, 99] += 1e-12j
    want = max(float(np.max(np.abs(w - np.eye(len(w))))) for w in views)
    assert abs(_defect(arena, jobs) - want) <= 4 * np.finfo(float).eps * want       # (a modulus: hypot on both sides)
