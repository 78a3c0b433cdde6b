"""``tpa_sample_select_batch`` and ``tpa_sample_gather_batch`` are declared in include/tenpy_amd.h, exported by the library (which
loads without a GPU) and bound in ``tenpy_amd._lib`` with the declared prototypes; the declaration cites the reference statements it
replaces and names the constant that bounds the site dimension.  Neither entry point is called here."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sample_symbols_declared_exported_and_bound():
    from tenpy_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'tenpy_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+tpa_sample_select_batch\s*\(([^)]*)\)', code)
    assert m and len(m.group(1).split(',')) == 11
    m = re.search(r'\bint\s+tpa_sample_gather_batch\s*\(([^)]*)\)', code)
    assert m and len(m.group(1).split(',')) == 7
    m = re.search(r'#define\s+TPA_SAMPLE_MAX_DIM\s+(\d+)', code)
    assert m and int(m.group(1)) == _lib.SAMPLE_MAX_DIM == 64
    doc = src[:src.index('#define TPA_SAMPLE_MAX_DIM')]
    doc = doc[doc.rindex('/*'):]
    assert 'mps.py:4403-4433' in doc and 'TPA_SAMPLE_MAX_DIM' in doc and 'TPA_E_BADARG' in doc and '16-byte' in doc
    lib = _lib.load()
    for name in ('tpa_sample_select_batch', 'tpa_sample_gather_batch'):
        assert hasattr(lib, name) and name in _lib.exported_symbols()
    assert len(lib.tpa_sample_select_batch.argtypes) == 11 and lib.tpa_sample_select_batch.restype is ctypes.c_int
    assert len(lib.tpa_sample_gather_batch.argtypes) == 7 and lib.tpa_sample_gather_batch.restype is ctypes.c_int
    assert 'tpa_sample.hip' in __import__('tenpy_amd._build', fromlist=['SOURCES']).SOURCES
