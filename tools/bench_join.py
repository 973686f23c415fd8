"""Self-join of rows of a packed corpus: BatchComparator.join (rf_join_u32: the queries stay in HBM, a work list per batch) against what a caller could do
before it existed -- Corpus.take of the query rows, one BatchComparator per row, BatchComparator.filter_multi in chunks of 256 -- in ONE process and session,
the two alternating.  Both return host results, so each call ends in a device synchronise: the times are host wall-clock times around the calls
(time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported, and road (b)'s own spread between repetitions
is the margin: (a) must not be slower than (b) by more than that.  The triples of the two roads are compared once (`triples_equal`); the timed calls are
given the sizes that comparison found (the number of triples; the longest row) as their capacities, so neither road runs anything twice.
The queries are `--queries` rows of the corpus itself (random rows, as query_indices), so every query has at least one match.  One JSON line per measurement
on stdout; --out appends them to a file.  --count-only runs both roads with capacity 0 (the count of triples, compared, and no triple): the scans and their
counted appends without the output's host arrays, for shapes whose result does not fit in host memory.  A mismatch between the roads, or a shape on which join
is slower than the other road by more than that road's spread, ends the run with an assertion -- after every shape has been measured and written.

The normalized shapes (*_levns95: Levenshtein normalized_similarity >= 0.95, *_ratio95: fuzz ratio >= 0.95) time BatchComparator.join_f64 (rf_join_f64) against
the same "before" road by normalized score (filter_multi is then rf_filter_multi_f64).  On the single-length corpus they also time, in the same alternation,
`join` (rf_join_u32) under the raw cutoff that keeps the same pairs -- 64-symbol rows: a normalized distance of at most 0.05 is a distance of at most 3 --
and compare the pairs: `join_u32_*` and `f64_over_u32` are what the f64 looks and the wider score cost.

    python tools/bench_join.py [--candidates 10000000] [--queries 4096,65536] [--reps 3] [--warmup 1] [--shapes ragged_lev2,ragged_indel4,rows_lev2,rows_indel4]
                               [--out profiles/join.txt]
    python tools/bench_join.py --shapes rows_levns95,rows_ratio95,ragged_levns95,ragged_ratio95 --out profiles/join_f64.txt
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
    # by normalized score (join_f64): a float cutoff
    "ragged_levns95": ("levenshtein", 0.95, "ragged"), "ragged_ratio95": ("ratio", 0.95, "ragged"), "rows_levns95": ("levenshtein", 0.95, "rows"),
    "rows_ratio95": ("ratio", 0.95, "rows"),
}
# the u32 join that keeps the same pairs over 64-symbol rows: 1 - d / 64 >= 0.95 <=> d <= 3 (the ratio: the inner lcs_seq comparator's distance 64 - lcs)
SAME_PAIRS_U32 = {"rows_levns95": ("levenshtein", 3), "rows_ratio95": ("lcs_seq", 3)}
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
    beyond_bar = []
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
        norm = isinstance(cutoff, float)
        cls = rf.fuzz.RatioBatchComparator if metric == "ratio" else getattr(rf.distance, metric).BatchComparator
        op = N.OP_DISTANCE if not norm else (N.OP_SIMILARITY if metric == "ratio" else N.OP_NORMALIZED_SIMILARITY)
        cls_join = cls.join_f64 if norm else cls.join
        for nq in [int(x) for x in args.queries.split(",")]:
            qi = np.random.default_rng(nq).choice(n, size=nq, replace=False).astype(np.uint64)

            def join(cap=None):  # (None: a count pass in front)
                return cls_join(corpus, corpus, op, score_cutoff=cutoff, query_indices=qi, capacity=cap)

            def before(cap=None):  # (None: filter_multi's first guess per row, and a repeat of the chunk where a row overflowed)
                oq, oi, sc = [], [], []
                for at in range(0, nq, CHUNK):
                    part = qi[at: at + CHUNK]
                    cs = [cls(row) for row in corpus[part]]
                    for j, (idx, val) in enumerate(cls.filter_multi(cs, op, corpus, capacity=cap, score_cutoff=cutoff)):
                        oq.append(np.full(len(idx), int(part[j]), dtype=np.uint64)), oi.append(idx), sc.append(val)
                return np.concatenate(oq), np.concatenate(oi), np.concatenate(sc)

            if args.count_only:
                # both roads with capacity 0: they count every pair and bring none home.  What is compared is the number of triples.
                def join(cap=None):
                    cls_join(corpus, corpus, op, score_cutoff=cutoff, query_indices=qi, capacity=0)
                    return (np.zeros(cls.last_join_count, dtype=np.uint8),)

                def before(cap=None):
                    total = 0
                    for at in range(0, nq, CHUNK):
                        cs = [cls(row) for row in corpus[qi[at: at + CHUNK]]]
                        cls.filter_multi(cs, op, corpus, capacity=0, score_cutoff=cutoff)
                        total += sum(cls.last_filter_counts)
                    return (np.zeros(total, dtype=np.uint8),)

            a, b = join(), before()  # (the triples compared; also the first warm-up of both)
            same = all(np.array_equal(x, y) for x, y in zip(a, b))
            assert same, f"{name}, {nq} queries: join and take + filter_multi return different triples ({len(a[0])} against {len(b[0])})"
            # the timed calls know their sizes, so that neither road runs anything twice: the true number of triples, the longest row
            cap_a = max(len(a[0]), 1)
            cap_b = 0 if args.count_only else max(int(np.bincount(np.searchsorted(np.sort(qi), b[0])).max()) if len(b[0]) else 1, 1)
            roads = [("join", join), ("before", before)]
            if name in SAME_PAIRS_U32:  # the u32 join of the same pairs, in the same alternation
                u32_metric, u32_cutoff = SAME_PAIRS_U32[name]
                u32_cls = getattr(rf.distance, u32_metric).BatchComparator

                def join_u32(cap=None):
                    if args.count_only:
                        u32_cls.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=u32_cutoff, query_indices=qi, capacity=0)
                        return (np.zeros(u32_cls.last_join_count, dtype=np.uint8),)
                    return u32_cls.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=u32_cutoff, query_indices=qi, capacity=cap)

                c = join_u32()
                assert len(c[0]) == len(a[0]) and all(np.array_equal(x, y) for x, y in zip(a[:2], c[:2])), f"{name}, {nq} queries: the u32 join keeps other pairs"
                del c
                roads.append(("join_u32", join_u32))
            del a, b
            for _ in range(args.warmup):
                for label, fn in roads:
                    fn(cap_b if label == "before" else cap_a)
            t = {label: [] for label, _ in roads}
            for _ in range(args.reps):  # alternating: all see the same clocks and the same neighbours
                for label, fn in roads:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(cap_b if label == "before" else cap_a)
                    t[label].append((time.perf_counter() - t0) * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            qlens = lens[qi.astype(np.int64)]
            classes = int((qlens <= 32).any()) + int((qlens > 32).any())
            line = {"shape": name, "metric": metric, "cutoff": cutoff, "corpus": kind, "candidates": n, "queries": nq, "reps": args.reps, "warmup": args.warmup,
                    "count_only": bool(args.count_only), "triples_equal": bool(same), "triples": cap_a, "longest_row": cap_b, "batches": -(-nq // batch), "launches_per_batch": 1 + classes,
                    "before_launches": -(-nq // 4)}  # (the two launch figures are arithmetic -- 1 + query classes present, queries / 4 -- not observed)
            for label, _ in roads:
                line[f"{label}_ms_median"] = round(med[label], 3)
                line[f"{label}_ms_min"] = round(min(t[label]), 3)
                line[f"{label}_ms_max"] = round(max(t[label]), 3)
                line[f"{label}_queries_per_s"] = round(nq / med[label] * 1e3, 1)
            line["before_spread_ms"] = round(max(t["before"]) - min(t["before"]), 3)
            line["before_over_join"] = round(med["before"] / med["join"], 3)
            line["join_within_bar"] = bool(med["join"] <= med["before"] + (max(t["before"]) - min(t["before"])))
            if "join_u32" in med:
                line["f64_over_u32"] = round(med["join"] / med["join_u32"], 3)
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line), flush=True)
            lines.append(line)
            if not line["join_within_bar"]:
                beyond_bar.append(f"{name}, {nq} queries: join {med['join']:.1f} ms against {med['before']:.1f} ms -- route this shape away from the device road")
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    # the bar: no shape the device road takes may be slower than what a caller had before by more than that road's own spread
    assert not beyond_bar, "; ".join(beyond_bar)


if __name__ == "__main__":
    main()
