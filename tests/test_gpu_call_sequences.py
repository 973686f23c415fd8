"""No result depends on the calls that came before it (`-m gpu`): tests/call_sequence_check.py in a child process per mode.  The header promises that handles are
immutable after creation and that no variable changes a result; the library keeps per-stream scratch with counters, pinned reports that steer the next launch, lazily
built structures, comparator caches and process-wide buffers all the same.  tests/call_sequences.py has the corpora, the catalogue of calls and the schedule (every
ordered pair of calls on a corpus, then a walk across the corpora), and tests/test_call_sequences_host.py holds them to their conditions without a GPU."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequence_check as CC  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", list(CC.MODES))
def test_no_result_depends_on_the_calls_before_it(mode):
    """One child per mode, started once, under a timeout of three times the seconds measured on an MI355X and at least 60 (CC.MEASURED_SECONDS).  `default` and
    `default-side` run what ships; `forced` and `forced-ten` set the knobs that put the small corpora on the stateful roads of large ones, and the child asserts from
    the RF_TRACE_PLAN trace that each road was taken before it looks at a value."""
    extra, _streams = CC.MODES[mode]
    env = {k: v for k, v in os.environ.items() if k not in CC.FORCED_ENV}
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "call_sequence_check.py"), mode], capture_output=True, text=True, cwd=ROOT, env=env, timeout=CC.timeout_of(mode))
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "FAILURES 0" and not [ln for ln in lines if ln.startswith(("MISMATCH", "ROAD MISSING"))], r.stdout[-4000:]
    if extra:
        roads = [ln for ln in lines if ln.startswith("roads: ")]
        assert len(roads) == 1 and all(int(w.split("=")[1]) >= 1 for w in roads[0][len("roads: "):].split(", ")), roads
