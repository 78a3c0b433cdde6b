"""Writes ``heff_programs.json``: the launch programs of the effective Hamiltonians as ``tests/test_heff_programs.py`` builds and
encodes them, on the emulated device.  Run it on the commit whose programs are to be kept:  python tests/golden/make_golden_programs.py [out]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pytest  # noqa: E402

import test_heff_programs as cases  # noqa: E402

if __name__ == '__main__':
    out = {}
    for name in cases.CASES:
        mp = pytest.MonkeyPatch()
        try:
            out[name] = cases.build(name, mp)
        finally:
            mp.undo()
    with open(sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(out[k], sort_keys=True)) for k in out) + '\n}\n')
