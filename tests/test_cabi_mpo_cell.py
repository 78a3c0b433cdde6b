"""``tpa_mpo_cell_apply_batch`` is declared in include/tenpy_amd.h, exported by the library (which loads without a GPU) and bound in
``tenpy_amd._lib``; the header states its row limit.  The entry point itself is never called here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_symbol_declared_exported_and_bound():
    from tenpy_amd import _lib
    src = open(os.path.join(ROOT, 'include', 'tenpy_amd.h')).read()
    code = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    assert re.search(r'\bint\s+tpa_mpo_cell_apply_batch\s*\(', code)
    assert re.search(r'#define\s+TPA_MPO_CELL_MAXROWS\s+32\b', code)
    lib = _lib.load()
    assert hasattr(lib, 'tpa_mpo_cell_apply_batch')
    assert 'tpa_mpo_cell_apply_batch' in _lib.exported_symbols()
    assert len(lib.tpa_mpo_cell_apply_batch.argtypes) == 11
