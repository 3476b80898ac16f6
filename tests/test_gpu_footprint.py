"""The write-footprint audit of the device-resident C ABI on the MI355X: one test per row of footprint_cases.ROWS.  Every shape of a
row runs twice inside a guarded arena -- run A on a fresh context, run B on the same context after a polluter call of another family
and with other prefills -- and must return SH_OK, leave every guard and every read-only payload intact, and give byte-identical
outputs in both runs; at the row's anchor shape the output also equals the exact model.  Rows whose path is chosen by a STARKHIP_*
knob run in a child process (a knob is read once per process), through this file's own __main__ dispatch."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), ROOT]
import footprint_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(row_id):
    from starks_amd import _lib
    return fc.run_row(_lib.lib(), fc.by_id()[row_id])


def _child():
    print(json.dumps(_run(sys.argv[2])))


@pytest.mark.parametrize("r", fc.ROWS, ids=lambda r: r.id)
def test_footprint(r):
    if r.env:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "row-child", r.id], capture_output=True, text=True,
                             env=dict(os.environ, **r.env), timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        found = json.loads(out.stdout.strip().splitlines()[-1])
    else:
        found = _run(r.id)
    assert found == [], "%d findings, the first: %r" % (len(found), found[:5])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"row-child": _child}[sys.argv[1]]()
