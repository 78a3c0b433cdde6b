"""``tpa_site_inner_batch`` and ``tpa_site_inner_work`` are declared in include/tenpy_amd.h, exported by the library (which loads
without a GPU) and bound in ``tenpy_amd._lib`` with the declared prototypes; the declaration cites the reference statements it replaces.
The batch entry point itself is never called here."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_site_inner_symbols_declared_exported_and_bound():
    from tenpy_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'tenpy_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+tpa_site_inner_batch\s*\(([^)]*)\)', code)
    assert m and len(m.group(1).split(',')) == 13
    m = re.search(r'\bint64_t\s+tpa_site_inner_work\s*\(([^)]*)\)', code)
    assert m and len(m.group(1).split(',')) == 4
    doc = src[:src.index('int64_t tpa_site_inner_work')]
    doc = doc[doc.rindex('/*'):]
    assert 'mps.py:1312-1316' in doc and ':591-596' in doc and 'TPA_MPO_APPLY_MAXD' in doc
    lib = _lib.load()
    for name in ('tpa_site_inner_batch', 'tpa_site_inner_work'):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert len(lib.tpa_site_inner_batch.argtypes) == 13 and lib.tpa_site_inner_batch.restype is ctypes.c_int
    assert len(lib.tpa_site_inner_work.argtypes) == 4 and lib.tpa_site_inner_work.restype is ctypes.c_int64


def test_site_inner_work_without_a_gpu():
    """The work-area size is host arithmetic: 2 doubles per (job, workgroup, stack slot), the workgroups of a job capped at 512."""
    from tenpy_amd import _lib
    W = _lib.load().tpa_site_inner_work
    assert W(0, 3, 1, 100) == 0 and W(3, 0, 1, 100) == 0
    assert W(2, 3, 5, 1) == 2 * 2 * 1 * 3 and W(2, 3, 5, 1025) == 2 * 2 * 2 * 3 and W(7, 9, 1, 10**12) == 2 * 7 * 512 * 9
