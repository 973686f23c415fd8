"""f64 cutoffs that equal a candidate's score, and the doubles on either side of it, on every result road (run with `-m gpu` on an MI355X): tests/cutoff_edge_check.py
in child processes, one per test id, each under the switches of the road it is named after.

tests/cutoff_edge_inputs.py has the corpora, the metric / argument sets and the cutoff grid (its head says why the expected value is the oracle called WITH the
cutoff); tests/cutoff_edge_check.py lists the result roads and what each forced road must show in the trace; tests/test_cutoff_edge_inputs.py keeps the inputs to
their conditions without a GPU.  DESIGN.md section 3 ("Cutoffs that equal a score") says which compare each id holds and has the measured seconds."""
import os
import subprocess
import sys

import pytest

from cutoff_edge_check import ROADS, SWITCHES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 180  # seconds per child


def _sliced(leg, road, m):
    return [(f"{leg}:{i}/{m}", road) for i in range(m)]


# (leg of tests/cutoff_edge_inputs.py, optionally a slice of it; road of tests/cutoff_edge_check.py)
IDS = (
    # ragged corpora (lengths 0..80), queries of 0, 1, 5, 32, 33, 40 and 64 symbols: emit_fin / tile_fin, plan()'s length window, the switch into the early-out
    # kernels and first_check, may_pass(); the Jaro epilogue, jaro_need and its host window; rf_filter_f64 / rf_topk_f64 and the multi-query entry points over them
    _sliced("lev-alnum", "early", 2) + _sliced("lev-abcd", "early", 2) + _sliced("lcs-alnum", "early", 2) + _sliced("lcs-abcd", "early", 2)
    + _sliced("jaro-alnum", "default", 4) + _sliced("jaro-abcd", "default", 4)
    # three of those queries with the corpus as length runs behind the head plane, and on the compiled twins of the asm scans
    + [("lev-alnum-few", "heads-runs"), ("lev-alnum-few", "compiled"), ("lcs-alnum-few", "compiled")]
    # single-length corpora: plan_band_filter's K at the quotients k / maximum (head plane, lane and tile lists, the prefilter off), the 6-bit payload and
    # stream_asm_f64_table on both sides of maximum 255, the single-word Jaro kernels
    + _sliced("rows-lev", "early", 2) + [("rows-lev64", "heads"), ("rows-lev64", "heads-tiles"), ("rows-lev64", "heads-nofilter"), ("rows-lev64", "compiled")]
    + [("rows-lcs", "early"), ("rows-lcs", "pack6"), ("rows-lcs64", "pack6-compiled"), ("table-edge", "pack6"), ("table-edge", "pack6-compiled"), ("table-edge", "default")]
    + _sliced("rows-jaro", "default", 3) + [("rows-jaro64", "jaro-priv")]
    + [("jaro-multiword", "default"), ("chars", "default")]
    # two corpora sized from the CU count so that every wavefront of a scan walks two tiles or more (asserted from each call's plan line), a thin grid
    + _sliced("multitile", "multitile", 2)
)


@pytest.mark.parametrize("leg,road", IDS, ids=[f"{leg}-{road}" for leg, road in IDS])
def test_f64_cutoffs_at_and_beside_a_score(leg, road):
    """One leg of tests/cutoff_edge_check.py under one road's switches: every value and every None bit-equal to the oracle, and the road seen in the trace."""
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env = dict(base, RF_TRACE_PLAN="1", **ROADS[road][0])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cutoff_edge_check.py"), leg, road], capture_output=True, text=True, cwd=ROOT, env=env, timeout=LIMIT)
    print(f"--- {leg} {road}: exit status {r.returncode}\n{r.stdout}")
    assert r.returncode == 0, (leg, road, r.stdout[-6000:], r.stderr[-3000:])
    assert "FAILURES 0" in r.stdout
    lines = [ln for ln in r.stdout.splitlines() if " checks, " in ln]
    assert lines and all(" 0 bad" in ln for ln in lines) and sum(int(ln.split(": ")[-1].split()[0]) for ln in lines) > 0, r.stdout[-4000:]
