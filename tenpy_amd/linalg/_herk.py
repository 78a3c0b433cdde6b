"""Host side of ``tpa_herk_chain`` (include/tenpy_amd.h, K1h): table layouts, the tile table and the launch.

The kernel forms ``C = [C +] sum_l A_l diag(s_l) B_l^dagger`` per task; a Hermitian task (``A_l = B_l``) is given only the tiles on and
below the diagonal of its tile grid and comes out Hermitian bit for bit.  The caller of the density-matrix mixer
(``algorithms/mixer.py``) builds one task per pair of pipe slices inside a charge sector."""
import ctypes

import numpy as np

from . import _device as dev

LINK_W, TASK_W = 12, 10
_bt = {}


def tile_rows(dtype):
    """Rows (= columns) of a tile of ``tpa_herk_chain`` for this dtype."""
    code = dev.code(dtype)
    if code not in _bt:
        from .. import _lib
        bt = ctypes.c_int()
        _lib.load().tpa_herk_tile_shape(code, ctypes.byref(bt))
        _bt[code] = bt.value
    return _bt[code]


def link_row(a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off=-1, w_len=1, w_inner=1):
    return [a_off, b_off, k, a_rs, a_ks, b_rs, b_ks, w_off, w_len, w_inner, 0, 0]


def task_row(c_off, m, n, ldc, link_begin, link_count, accumulate=0, herm=0, mirror_off=-1, mirror_ldc=0):
    return [c_off, m, n, ldc, link_begin, link_count, accumulate, herm, mirror_off, mirror_ldc]


def tile_table(tasks, links, bt):
    """int32[n_tiles][4] = {task, tile_row, tile_col, 0}: every tile of a general task, the tiles with tile_row >= tile_col of a
    Hermitian task; the tiles of the longest chains (sum of k over the live links) first, as for ``tpa_gemm_chain``."""
    tasks = np.asarray(tasks, np.int64).reshape(-1, TASK_W)
    links = np.asarray(links, np.int64).reshape(-1, LINK_W)
    kcum = np.concatenate([[0], np.cumsum(np.maximum(links[:, 2], 0))])
    work = kcum[tasks[:, 4] + tasks[:, 5]] - kcum[tasks[:, 4]]
    rows = []
    for t in np.argsort(-work, kind='stable'):
        _, m, n, _, _, _, _, herm = tasks[t, :8]
        tr, tc = -(-int(m) // bt), -(-int(n) // bt)
        ii, jj = np.meshgrid(np.arange(tr), np.arange(tc), indexing='ij')
        keep = (ii >= jj) if herm else np.ones_like(ii, bool)
        rows.append(np.stack([np.full(keep.sum(), t), ii[keep], jj[keep], np.zeros(keep.sum(), np.int64)], axis=1))
    if not rows:
        return np.zeros((0, 4), np.int32)
    return np.concatenate(rows).astype(np.int32)


def herk_chain(dtype, tasks_d, links_d, tiles_d, n_tiles, A, B, wvec, C):
    """Launch on the current stream; the tables are device tensors, A / B / C arenas, ``wvec`` a float64 arena or None."""
    L = dev.lib()
    dev.check(L.tpa_herk_chain(dev.code(dtype), tasks_d.data_ptr(), links_d.data_ptr(), tiles_d.data_ptr(), int(n_tiles), A.data_ptr(),
                               B.data_ptr(), dev.ptr(wvec), C.data_ptr(), dev.stream()), "herk_chain")
