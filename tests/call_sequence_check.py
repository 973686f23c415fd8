"""Run by tests/test_gpu_call_sequences.py in a child process per mode: no result depends on the calls that came before it.

The library keeps more state between calls than any other part of it (tests/call_sequences.py and DESIGN.md list it).  The other tests check each road on
freshly made handles in the one order their author wrote down; a kernel that leaves a counter half-armed on one exit path, a host decision read from the previous
call's report, a cache entry taken over from another stream show in the NEXT call only, and only if it is the right next call.  So here the three corpora of
tests/call_sequences.py are made once and kept to the end, every comparator is made once and used on every corpus it serves, and the schedule of that module runs:
per corpus an Eulerian circuit through every ordered pair of its letters (a letter after itself included), then a seeded walk of 400 calls across all corpora.
Every call's value is compared with its letter's expected value, which comes from the CPU side alone, once per letter.

argv[1] is the mode (the test sets the environment: MODES below):
  default       what ships, every call on the default stream: filter_last_survivors, the gather temporary's growth, the comparator caches, the streamed buffer sets
  default-side  the same, every call on one side stream
  forced        FORCED_ENV puts these small corpora on the stateful roads of large ones -- the head plane with its two-pass lane compaction, length runs, band runs with
                their pinned report, the 6-bit payload, hinted scans with their sample and trust, the gather temporary, the top-k sample pass (RF_TOPK_SAMPLE=8: U's
                129 tiles are >= 8 x 8) -- on one side stream.  The kept score buffer of the scan-plus-one-pass top-k needs no knob (a Levenshtein query of 65 to
                256 symbols reaches it); that it was reached is read from the trace with the rest.  That each road was taken at least once is read from the RF_TRACE_PLAN trace BEFORE a value is looked
                at: ROADS below; a road that was not taken fails the mode.
  forced-ten    the same on ten side streams, step i on stream i mod 10: more streams than any StreamCache keeps entries for (8, 4 and 4), so entries are taken over
                together with their reports and counters.
A call with device-resident output (topk_entries_device) is synchronized on its own stream before it is read, but not before the next letter has been issued; at
most two are outstanding.

One line `MISMATCH step=... after=<previous letter> letter=... stream=...` per differing value -- a mismatch is a value, the child runs to its end --, `ROAD MISSING ...`
per road not taken, `FAILURES n` last; exit status 0 only if n is 0 and every road was taken.  A HIP error (RF_ERR_HIP) raises and ends the child there.

Planted errors tried on an MI355X (not committed); mismatching steps of the 1996 per mode, default / default-side / forced / forced-ten:
  the root workgroup of topk_block_publish leaving `*p.topk_bound = kth + 1` whatever topk_bound_from_result says: 110 / 110 / 60 / 59.  Without the sample pass
      (the default modes) every in-scan top-k of U that follows one with a smaller k-th key comes back short: u.top16, u.top64, u.top24<=3, u.top64<=2.short,
      u.top16.entries.b; so do r.topk_multi while the bound that r.top16.q200 left stands on R, and w.top16.wql and w.top5.wql2 while a smaller one stands on W
      (the one pass over the score vector publishes through the same scratch; the bound outlives the calls in between that are no top-k).  In the forced modes U's two letters under a cutoff go red (their calls skip the sample pass) and W's two; elsewhere
      the sample pass itself runs under the stale bound, finds fewer than k and leaves ~0, which hides the error from the main pass.
  the `lowered` map of a comparator keyed by a constant instead of the corpus' uid: 27 / 27 / 27 / 27, every w2.lev (the `char` query on W2 after its first call on W,
      through W's alphabet).
  the last workgroup of filter_select_kernel not zeroing the count of select_workspace(device): 0 / 0 / 15 / 15 -- u.filter<=3.few, u.filter<=3.many,
      u.filter<=3.many.cap50, u.filter<=4.by_score after another lane-compacted filter call (the road exists under RF_HEAD8_MIN=1 only), until the count passes the
      workspace's room and every later call takes the general compaction.
  the scan-plus-one-pass top-k taking the kept `scores` buffer of its (corpus, stream) for its own scores once the buffer is there (the scan skipped): 27 / 27 /
      27 / 21.  On one stream every w.top5.wql2 selects from the scores of w.top16.wql, which wrote the buffer first; on ten streams either letter is wrong on the
      streams the other one reached first.  r.top16.q200, the only such call on R, stays green under this error: one query per corpus cannot tell its own old
      scores from new ones, which is why W has two.

Seconds per mode, the wall clock of the whole child measured once on an MI355X: MEASURED_SECONDS below; the timeouts of the test are three times these, and at
least 60 s.
"""
import os
import sys
import tempfile
import time

import numpy as np

MEASURED_SECONDS = {"default": 5, "default-side": 5, "forced": 5, "forced-ten": 5}  # whole child process, wall clock (4.5, 4.1, 4.1, 4.4)
FORCED_ENV = {"RF_HEAD8_MIN": "1", "RF_BAND_FILTER": "1", "RF_RUN_MIN_TILES": "1", "RF_BAND_RUN_MIN_TILES": "1", "RF_PACK6_MIN_TILES": "1", "RF_HINT_MIN_TILES": "1",
              "RF_HINT_SAMPLE_MIN_TILES": "1", "RF_UNSCATTER_MIN": "1", "RF_TOPK_SAMPLE": "8", "RF_TRACE_PLAN": "1"}
# mode -> (extra environment, streams: 0 = the default stream)
MODES = {"default": ({}, 0), "default-side": ({}, 1), "forced": (FORCED_ENV, 1), "forced-ten": (FORCED_ENV, 10)}
# what the trace of a forced mode must hold at least once: (name, alternatives)
ROADS = [("two-pass", ("[rf road] two-pass:",)), ("lane compaction", ("[rf plan] filter: lane compaction",)), ("hinted scan", ("hint lists:", "hint pass:")),
         ("band report", ("band report:",)), ("gather", ("gather=1",)), ("6-bit payload", ("data6=1",)),
         ("top-k sample pass", ("sample=1 via_scores=0",)), ("top-k kept score buffer", ("via_scores=1 kept_scores=1",))]
RF_ERR_HIP = 2


def timeout_of(mode):
    return max(60, 3 * MEASURED_SECONDS[mode])


class Context:
    """the handles of one child: corpora and comparators are made once and live to its end"""

    def __init__(self, tmp):
        import torch

        import rapidfuzz_rs_amd as rf
        import call_sequences as S

        self.rf, self.torch, self.S = rf, torch, S
        self.corpus, self.path, self.slot_index, self._bc = {}, {}, {}, {}
        for name in ("U", "R", "W", "W2"):
            data, offsets = S.corpus_input(name)
            self.corpus[name] = (rf.Corpus.from_ragged_u32 if data.dtype == np.uint32 else rf.Corpus.from_ragged)(data, offsets)
            assert len(self.corpus[name]) == S.corpus_size(name)
            self.path[name] = os.path.join(tmp, name + ".rfc")
            self.corpus[name].save(self.path[name])
        self.slot_index["R"] = self.corpus["R"].slot_index()
        own, overflow = self.corpus["W"].alphabet_size()
        assert own == 254 and overflow == len(S.corpus_w()["W"]["overflow"]), (own, overflow)

    def bc(self, metric, qname):
        key = (metric, qname)
        if key not in self._bc:
            self._bc[key] = getattr(self.rf.distance, metric).BatchComparator(self.S.all_queries()[qname])
        return self._bc[key]

    def entries(self, k):
        return self.torch.empty((k, 2), dtype=self.torch.int64, device="cuda")  # (no fill: a fill would go to torch's current stream, unordered with the call's; the call writes all k rows)


def main(mode):
    import torch

    import rapidfuzz_rs_amd as rf
    import call_sequences as S
    from multitile_lists_check import Trace

    extra, n_streams = MODES[mode]
    for k, v in extra.items():
        assert os.environ.get(k) == v, f"run with {k}={v}"
    forced = bool(extra)
    if not forced:
        assert not [k for k in FORCED_ENV if k in os.environ and k != "RF_TRACE_PLAN"], "run without the forcing knobs"
    letters, sched = S.letters(), S.schedule()
    print(f"mode {mode}: seed {S.SEED:#x}, {len(sched)} calls over {len(letters)} letters, {n_streams or 'the default'} stream(s)", flush=True)
    for lt in letters.values():  # the CPU side, once per letter, before the first device call
        lt.expected
    if forced:  # the sample pass of the in-scan top-k applies to U: from the tile count (and, after the run, from the trace: ROADS)
        assert (S.corpus_size("U") + 63) // 64 >= 8 * int(os.environ["RF_TOPK_SAMPLE"])
    trace = Trace() if os.environ.get("RF_TRACE_PLAN") else None
    failures = 0
    try:
        with tempfile.TemporaryDirectory() as tmp:
            ctx = Context(tmp)
            streams = [torch.cuda.Stream() for _ in range(n_streams)] or [None]

            def handle(s):
                return None if s is None else s.cuda_stream

            def synchronize(s):
                (torch.cuda.default_stream() if s is None else s).synchronize()

            got = [None] * len(sched)
            outstanding = []  # (step, stream, Pending)

            def settle(upto):
                while outstanding and outstanding[0][0] < upto:
                    step, s, pending = outstanding.pop(0)
                    synchronize(s)
                    got[step] = pending.read()

            for step, (_part, name) in enumerate(sched):
                s = streams[step % len(streams)]
                try:
                    value = letters[name].call(ctx, handle(s))
                except rf.RfError as e:
                    if e.status == RF_ERR_HIP:
                        raise
                    value = (np.array([-e.status], dtype=np.int64),)  # an unexpected refusal is a value, and a wrong one
                if isinstance(value, S.Pending):
                    settle(step)  # at most two outstanding: this one and the one before it
                    outstanding.append((step, s, value))
                else:
                    got[step] = value
                    settle(step)  # (issued before this letter: this letter went out first)
            settle(len(sched))
            torch.cuda.synchronize()
            text = trace.take() if trace is not None else ""
            # ---- the roads, before a value is looked at
            if forced:
                for road, marks in ROADS:
                    if not any(m in text for m in marks):
                        failures += 1
                        print(f"ROAD MISSING {road}: none of {marks} in the trace", flush=True)
                print("roads: " + ", ".join(f"{road}={sum(text.count(m) for m in marks)}" for road, marks in ROADS), flush=True)
            # ---- the values
            bad_letters = {}
            for step, (part, name) in enumerate(sched):
                if not letters[name].agrees(got[step]):
                    failures += 1
                    bad_letters[name] = bad_letters.get(name, 0) + 1
                    after = sched[step - 1][1] if step else "-"
                    print(f"MISMATCH step={step} after={after} letter={name} stream={step % len(streams) if n_streams else 'default'} part={part}", flush=True)
            if bad_letters:
                print("letters with mismatches: " + ", ".join(f"{k} x{v}" for k, v in sorted(bad_letters.items())), flush=True)
            del ctx
    finally:
        if trace is not None:
            trace.close()  # (a traceback goes to the real stderr)
    return failures


if __name__ == "__main__":
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    t_start = time.time()
    n_bad = main(sys.argv[1] if len(sys.argv) > 1 else "default")
    print(f"SECONDS {time.time() - t_start:.1f}")
    print("FAILURES", n_bad)
    sys.exit(1 if n_bad else 0)
