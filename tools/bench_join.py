"""Self-join of rows of a packed corpus: BatchComparator.join (rf_join_u32: the queries stay in HBM, a work list per batch) against what a caller could do
before it existed -- Corpus.take of the query rows, one BatchComparator per row, BatchComparator.filter_multi in chunks of 256 -- in ONE process and session,
the two alternating.  Both return host results, so each call ends in a device synchronise: the times are host wall-clock times around the calls
(time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported, and road (b)'s own spread between repetitions
is the margin: (a) must not be slower than (b) by more than that.  The triples of the two roads are compared once (`triples_equal`); the timed calls are
given the sizes that comparison found (the number of triples; the longest row) as their capacities, so neither road runs anything twice.
The queries are `--queries` rows of the corpus itself (random rows, as query_indices), so every query has at least one match.  One JSON line per measurement
on stdout; --out appends them to a file.  --count-only runs both roads with capacity 0 (the count of triples, compared, and no triple): the scans and their
counted appends without the output's host arrays, for shapes whose result does not fit in host memory.  A mismatch between the roads, or a shape on which join
is slower than the other road by more than that road's spread, ends the run with an assertion.

    python tools/bench_join.py [--candidates 10000000] [--queries 4096,65536] [--reps 3] [--warmup 1] [--shapes ragged_lev2,ragged_indel4,rows_lev2,rows_indel4]
                               [--out profiles/join.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth

SHAPES = {  # name: (metric, cutoff, corpus: "rows" = single length 64, "ragged" = lengths 1..64)
    "ragged_lev2": ("levenshtein", 2, "ragged"), "ragged_indel4": ("indel", 4, "ragged"), "rows_lev2": ("levenshtein", 2, "rows"), "rows_indel4": ("indel", 4, "rows"),
}
CHUNK = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=10_000_000)
    ap.add_argument("--queries", default="4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--count-only", action="store_true", help="capacity 0 on both roads: the number of triples and no triple (the scan without the output's host arrays)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "3 or more alternating repetitions"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.candidates
    batch = int(os.environ.get("RF_JOIN_BATCH", "16384"))
    lines = []
    held = {}
    for name in sorted(args.shapes.split(","), key=lambda s: SHAPES[s][2]):
        metric, cutoff, kind = SHAPES[name]
        if kind not in held:
            held.clear()  # one corpus in HBM at a time
            torch.cuda.empty_cache()
            if kind == "ragged":
                data, offsets = synth.ragged_host(n, 64, seed=0xC0FFEE03, min_len=1)
                held[kind] = (rf.Corpus.from_ragged(data, offsets, device=0), np.diff(offsets.astype(np.int64)))
                del data, offsets
            else:
                held[kind] = (rf.Corpus.from_device_rows(synth.rows_device(n, 64, seed=0xC0FFEE03, device=dev)), np.full(n, 64))
        corpus, lens = held[kind]
        cls = getattr(rf.distance, metric).BatchComparator
        for nq in [int(x) for x in args.queries.split(",")]:
            qi = np.random.default_rng(nq).choice(n, size=nq, replace=False).astype(np.uint64)

            def join(cap=None):  # (None: a count pass in front)
                return cls.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=cutoff, query_indices=qi, capacity=cap)

            def before(cap=None):  # (None: filter_multi's first guess per row, and a repeat of the chunk where a row overflowed)
                oq, oi, sc = [], [], []
                for at in range(0, nq, CHUNK):
                    part = qi[at: at + CHUNK]
                    cs = [cls(row) for row in corpus[part]]
                    for j, (idx, val) in enumerate(cls.filter_multi(cs, N.OP_DISTANCE, corpus, capacity=cap, score_cutoff=cutoff)):
                        oq.append(np.full(len(idx), int(part[j]), dtype=np.uint64)), oi.append(idx), sc.append(val)
                return np.concatenate(oq), np.concatenate(oi), np.concatenate(sc)

            if args.count_only:
                # both roads with capacity 0: they count every pair and bring none home.  What is compared is the number of triples.
                def join(cap=None):
                    cls.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=cutoff, query_indices=qi, capacity=0)
                    return (np.zeros(cls.last_join_count, dtype=np.uint8),)

                def before(cap=None):
                    total = 0
                    for at in range(0, nq, CHUNK):
                        cs = [cls(row) for row in corpus[qi[at: at + CHUNK]]]
                        cls.filter_multi(cs, N.OP_DISTANCE, corpus, capacity=0, score_cutoff=cutoff)
                        total += sum(cls.last_filter_counts)
                    return (np.zeros(total, dtype=np.uint8),)

            a, b = join(), before()  # (the triples compared; also the first warm-up of both)
            same = all(np.array_equal(x, y) for x, y in zip(a, b))
            assert same, f"{name}, {nq} queries: join and take + filter_multi return different triples ({len(a[0])} against {len(b[0])})"
            # the timed calls know their sizes, so that neither road runs anything twice: the true number of triples, the longest row
            cap_a = max(len(a[0]), 1)
            cap_b = 0 if args.count_only else max(int(np.bincount(np.searchsorted(np.sort(qi), b[0])).max()) if len(b[0]) else 1, 1)
            del a, b
            for _ in range(args.warmup):
                join(cap_a), before(cap_b)
            t = {"join": [], "before": []}
            for _ in range(args.reps):  # alternating: both see the same clocks and the same neighbours
                for label, fn in (("join", join), ("before", before)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(cap_a if label == "join" else cap_b)
                    t[label].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            qlens = lens[qi.astype(np.int64)]
            classes = int((qlens <= 32).any()) + int((qlens > 32).any())
            line = {"shape": name, "metric": metric, "cutoff": cutoff, "corpus": kind, "candidates": n, "queries": nq, "reps": args.reps, "warmup": args.warmup,
                    "count_only": bool(args.count_only), "triples_equal": bool(same), "triples": cap_a, "longest_row": cap_b, "batches": -(-nq // batch), "launches_per_batch": 1 + classes,
                    "before_launches": -(-nq // 4)}  # (the two launch figures are arithmetic -- 1 + query classes present, queries / 4 -- not observed)
            for label in ("join", "before"):
                line[f"{label}_ms_median"] = round(med[label], 3)
                line[f"{label}_ms_min"] = round(min(t[label]), 3)
                line[f"{label}_ms_max"] = round(max(t[label]), 3)
                line[f"{label}_queries_per_s"] = round(nq / med[label] * 1e3, 1)
            line["before_spread_ms"] = round(max(t["before"]) - min(t["before"]), 3)
            line["before_over_join"] = round(med["before"] / med["join"], 3)
            line["join_within_bar"] = bool(med["join"] <= med["before"] + (max(t["before"]) - min(t["before"])))
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line), flush=True)
            lines.append(line)
            # the bar: no shape the device road takes may be slower than what a caller had before by more than that road's own spread
            assert line["join_within_bar"], f"{name}, {nq} queries: join {med['join']:.1f} ms against {med['before']:.1f} ms -- route this shape away from the device road"
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
