"""GPU parity tests (`-m gpu`) of the multi-query and join roads -- rf_filter_multi_u32 / _f64, rf_topk_multi_u32 / _f64, rf_join_u32 / _f64 -- on every corpus LAYOUT
the packers can produce: the five of tests/test_gpu_layouts.py and `no_rename_file`, a corpus packed and saved under RF_NO_RENAME and loaded without the knob.  The
tests of those roads pack every corpus in-process with no knob set; what they never see is what RF_NO_MIXED_TILES produces: padding lanes INSIDE the exact tiles of a
tiled corpus (a length with one candidate left over is a tile with 63 of them), length windows that begin and end strictly inside the corpus on partial tiles, a query
corpus of a join in such a layout, two sides of a join that store different codes, and a tile table, slot map and sigma that come from a file.

The inputs (tests/layout_multi_inputs.py; tests/test_layout_multi_inputs.py checks them on the host) are one scanned corpus P of ~6 700 candidates of 0..70 symbols in
which every length ends in a partial tile, eleven queries planted into padded and into full tiles, and a query corpus QC of 147 rows.  Every value is compared for
equality with the CPU oracle, f64 scores by their bit patterns; tests/layout_multi_check.py holds the checks and runs once per leg in a child process with the leg's
knobs (read once per process) and RF_TRACE_PLAN=1: the "[rf plan]" lines must show that only the 65-symbol query went per query, so no pass comes from the fallback
road.  A file leg has a second child before it, which packs and saves under the knob and tests nothing.  No child is retried; every child has a timeout."""
import os
import subprocess
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
from test_gpu_layouts import LAYOUTS, NO_MIXED  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(TESTS)
CHECK = os.path.join(TESTS, "layout_multi_check.py")
# leg -> the environment of the child that packs and saves, for the legs whose testing process loads files with no knob set
SAVED = {"no_mixed_file": LAYOUTS["no_mixed_file"], "no_rename_file": LAYOUTS["no_rename"]}
LEGS = list(LAYOUTS) + ["no_rename_file"]


def _run(args, env, timeout):
    return subprocess.run([sys.executable, CHECK] + args, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=timeout)


@pytest.mark.parametrize("leg", LEGS)
def test_multi_query_and_join_roads(leg, tmp_path):
    files = []
    if leg in SAVED:
        files = [str(tmp_path / "p.rfc"), str(tmp_path / "qc.rfc")]
        s = _run(["save"] + files, SAVED[leg], 120)
        assert s.returncode == 0, s.stdout[-2000:] + s.stderr[-3000:]
    r = _run([leg, "1" if leg in NO_MIXED else "0"] + files, dict({} if leg in SAVED else LAYOUTS[leg], RF_TRACE_PLAN="1"), 300)
    print(r.stdout)  # (every section's verdict and wall time)
    failed = [ln for ln in r.stdout.splitlines() if ln.endswith("FAILED") or ln.startswith("FAILED SECTIONS")]
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, "\n".join(failed) + "\n" + r.stdout[-3000:] + r.stderr[-2000:]
