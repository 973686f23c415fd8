"""The 6-bit roads at 62, 63, 64 and 65 distinct corpus symbols (run with `-m gpu` on an MI355X): tests/symbol_edge_check.py in child processes, one leg each.

tests/symbol_edge_check.py (its head has the inputs, the query families and what each leg asserts) compares every value with the oracle and every road with
what the alphabet size and the length alone allow; DESIGN.md section 4 has the table of bounds and the leg that guards each row."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# leg -> the children it starts: (argv[1] of tests/symbol_edge_check.py, extra environment); their result vectors must be the same (the DIGEST line).
# Each child takes a few seconds on an MI355X, most of it the imports; the time limit is per child.
LEGS = {
    "payload": [("payload", {"RF_PACK6_MIN_TILES": "1"})],
    "bucketed": [("bucketed", {"RF_PACK6_MIN_TILES": "1"})],
    "heads": [("heads", {"RF_HEAD8_MIN": "1", "RF_BAND_FILTER": "1"}), ("heads", {"RF_HEAD8_MIN": "1", "RF_BAND_FILTER": "1", "RF_HEAD6": "0"})],
    "jaro": [("jaro", {"RF_JARO_PRIV": "1"}), ("jaro", {})],
    "norename": [("norename", {"RF_NO_RENAME": "1", "RF_PACK6_MIN_TILES": "1", "RF_HEAD8_MIN": "1", "RF_BAND_FILTER": "1"})],
    "saveload": [("saveload", {"RF_PACK6_MIN_TILES": "1"})],
}
LIMIT = 120  # seconds per child


@pytest.mark.parametrize("leg", list(LEGS))
def test_six_bit_roads_at_63_64_and_65_symbols(leg):
    """One leg of tests/symbol_edge_check.py (its head has the inputs, the query families and what each leg asserts).  A child that fails ends its leg."""
    switches = ("RF_PACK6_MIN_TILES", "RF_PACK6", "RF_HEAD8_MIN", "RF_BAND_FILTER", "RF_HEAD6", "RF_JARO_PRIV", "RF_NO_RENAME", "RF_STREAM", "RF_ASM_STREAM", "RF_ASM_CHUNK")
    base = {k: v for k, v in os.environ.items() if k not in switches}
    digests = []
    for arg, extra in LEGS[leg]:
        env = dict(base, RF_TRACE_PLAN="1", RF_PACK_TIMING="1", **extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "symbol_edge_check.py"), arg], capture_output=True, text=True, cwd=ROOT, env=env, timeout=LIMIT)
        print(f"--- {arg} {extra}: exit status {r.returncode}\n{r.stdout}")
        assert r.returncode == 0, (extra, r.stdout[-4000:], r.stderr[-3000:])
        assert "FAILURES 0" in r.stdout
        lines = [ln for ln in r.stdout.splitlines() if " checks, " in ln]
        assert lines and all(ln.endswith(", 0 bad") and int(ln.split(": ")[-1].split()[0]) > 0 for ln in lines), r.stdout[-4000:]
        digests += [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
    assert len(digests) == len(LEGS[leg]) and len(set(digests)) == 1, digests
