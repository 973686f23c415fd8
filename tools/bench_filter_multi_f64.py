"""Thresholded matches by normalized score for many queries: BatchComparator.filter_multi with a normalized op (rf_filter_multi_f64, tight-cutoff queries 4 to
a pass over the corpus) against the same queries through a loop of BatchComparator.filter_many (rf_filter_f64, one scan sequence and one host round trip per
query), in ONE process and session, the two alternating.  Both return host results, so each call ends in a device synchronise: the times are host wall-clock
times around the calls (time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported and the spread between
repetitions is the margin for "faster".  The rows of the two roads are compared once (`rows_equal`: indices and doubles as bit patterns; `pairs` = how many
(index, score) pairs that comparison covered).  Queries are near-copies (one substitution) of candidates of the corpus where it holds candidates of the query's
length, random strings otherwise, so the rows are not all empty.  One JSON line per measurement on stdout; --out appends them to a file.

    python tools/bench_filter_multi_f64.py [--candidates 10000,10000000,30000000,100000000] [--ragged-candidates 10000000] [--queries 16,256]
                                           [--cutoffs 0.9,0.95] [--reps 5] [--warmup 1] [--shapes lev64,lev24,indel64,indel24,ratio64,ratio24,ragged_...]
                                           [--u32] [--out profiles/filter_multi_f64.txt]

Every scorer runs normalized_similarity >= cutoff (the ratio: its similarity).  --u32 adds, on the single-length corpora, the u32 call (rf_filter_multi_u32)
under the raw cutoff that keeps the same candidates there -- distance <= floor((1 - cutoff) * maximum), the maximum being one number in such a corpus -- as
`u32_fused_ms_*`: the cost of the normalized emission is fused over u32_fused.  Every line records RF_FILTER_MULTI and RF_FILTER_MULTI_F64_ROUTE as the process
had them (the library reads them as on unless they are 0: the first would send filter_multi down the loop's road too, the second fuses the shapes the f64
planner's routing rules send per query), and `plan`, the call's own [rf plan] line when RF_TRACE_PLAN is set.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth

SHAPES = {}  # name: (metric, query length, corpus: "rows" = single length 64, "ragged" = lengths 1..64)
for _kind, _prefix in (("rows", ""), ("ragged", "ragged_")):
    for _metric, _short in (("levenshtein", "lev"), ("indel", "indel"), ("ratio", "ratio")):
        for _qlen in (64, 24):
            SHAPES[f"{_prefix}{_short}{_qlen}"] = (_metric, _qlen, _kind)
NS = N.OP_NORMALIZED_SIMILARITY


def queries_from(pick, qlen, count, seed):
    """`count` queries of qlen symbols: candidate pick(j) with one symbol replaced where the corpus has candidates of that length, else random"""
    rng = np.random.default_rng(seed)
    qs = []
    for j in range(count):
        row = pick(j)
        if row is None:
            qs.append(synth.query(qlen, seed + j))
            continue
        row = np.array(row, dtype=np.uint8)
        row[int(rng.integers(0, len(row)))] = 126
        qs.append(row.tobytes())
    return qs


def plan_line(fn):
    """what the call's [rf plan] filter_multi_f64 line says (RF_TRACE_PLAN set), read from this process' own stderr"""
    if not os.environ.get("RF_TRACE_PLAN"):
        return None
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = [ln for ln in tmp.read().decode("utf-8", "replace").splitlines() if ln.startswith("[rf plan] filter_multi_f64:")]
    if not lines:
        return None
    groups = lines[-1].split("fused_groups=[")[1].split("]")[0]
    sizes = [int(x) for x in groups.split(",") if x]
    return {"groups_of_4": sizes.count(4), "groups_of_2": sizes.count(2), "per_query": int(lines[-1].rsplit("per_query=", 1)[1])}


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="10000,10000000,30000000,100000000", help="sizes of the single-length corpora, comma-separated")
    ap.add_argument("--ragged-candidates", default="10000000", help="sizes of the ragged corpora, comma-separated")
    ap.add_argument("--queries", default="16,256")
    ap.add_argument("--cutoffs", default="0.9,0.95")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--u32", action="store_true", help="also time rf_filter_multi_u32 under the equivalent raw cutoff (single-length corpora, levenshtein / indel)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "3 or more alternating repetitions"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    jobs = []  # (name, metric, query length, kind, candidates)
    for name in args.shapes.split(","):
        metric, qlen, kind = SHAPES[name]
        sizes = [int(x) for x in (args.ragged_candidates if kind == "ragged" else args.candidates).split(",") if x]
        jobs += [(name, metric, qlen, kind, n) for n in sizes]
    jobs.sort(key=lambda j: (j[3], j[4]))  # (stable: the shapes of one corpus stay together and in the order given)
    held = {}
    out = open(args.out, "a") if args.out else None
    for name, metric, qlen, kind, n_rows in jobs:
        key = (kind, n_rows)
        if key not in held:
            held.clear()  # one corpus in HBM at a time
            torch.cuda.empty_cache()
            if kind == "ragged":
                data, offsets = synth.ragged_host(n_rows, 64, seed=0xC0FFEE03, min_len=1)
                lens = np.diff(offsets.astype(np.int64))
                by_len = {ln: np.nonzero(lens == ln)[0] for ln in {s[1] for s in SHAPES.values()}}

                def pick(j, ln, data=data, offsets=offsets, by_len=by_len):
                    at = by_len[ln]
                    if len(at) == 0:
                        return None
                    i = int(at[(j * 7919) % len(at)])
                    return data[int(offsets[i]): int(offsets[i + 1])]

                held[key] = (rf.Corpus.from_ragged(data, offsets, device=0), pick)
            else:
                rows = synth.rows_device(n_rows, 64, seed=0xC0FFEE03, device=dev)
                sample = rows[torch.arange(0, 512, device=dev) * 7919 % n_rows].cpu().numpy()
                held[key] = (rf.Corpus.from_device_rows(rows), lambda j, ln, sample=sample: sample[j % len(sample)] if ln == 64 else None)
                del rows
        corpus, pick = held[key]
        cls = rf.fuzz.RatioBatchComparator if metric == "ratio" else getattr(rf.distance, metric).BatchComparator
        op = N.OP_SIMILARITY if metric == "ratio" else NS
        for nq in [int(x) for x in args.queries.split(",")]:
            cs = [cls(q) for q in queries_from(lambda j: pick(j, qlen), qlen, nq, 0xC0FFEE03)]
            for cutoff in [float(x) for x in args.cutoffs.split(",")]:
                roads = {"fused": lambda: cls.filter_multi(cs, op, corpus, score_cutoff=cutoff),
                         "loop": lambda: [c.filter_many(op, corpus, score_cutoff=cutoff) for c in cs]}
                raw_cutoff = None
                if args.u32 and kind == "rows" and metric != "ratio":
                    maximum = max(qlen, 64) if metric == "levenshtein" else qlen + 64
                    raw_cutoff = int(math.floor((1.0 - cutoff) * maximum + 1e-9))
                    roads["u32_fused"] = lambda: cls.filter_multi(cs, N.OP_DISTANCE, corpus, score_cutoff=raw_cutoff)
                a, b = roads["fused"](), roads["loop"]()  # (the rows compared; also the first warm-up of both)
                plan = plan_line(roads["fused"])
                for _ in range(args.warmup):
                    for fn in roads.values():
                        fn()
                same = all(x[0].tolist() == y[0].tolist() and bits(x[1]) == bits(y[1]) for x, y in zip(a, b))
                pairs = sum(len(y[0]) for y in b)
                t = {label: [] for label in roads}
                for _ in range(args.reps):  # alternating: all see the same clocks and the same neighbours
                    for label, fn in roads.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        t[label].append((time.perf_counter() - t0) * 1e3)
                n = len(corpus)
                med = {k_: statistics.median(v) for k_, v in t.items()}
                line = {"shape": name, "metric": metric, "op": "normalized_similarity", "cutoff": cutoff, "query_len": qlen, "corpus": kind, "candidates": n, "queries": nq,
                        "reps": args.reps, "warmup": args.warmup, "rows_equal": same, "pairs": pairs, "RF_FILTER_MULTI": os.environ.get("RF_FILTER_MULTI", "1"),
                        "RF_FILTER_MULTI_F64_ROUTE": os.environ.get("RF_FILTER_MULTI_F64_ROUTE", "1"), "plan": plan}
                for label in roads:
                    line[f"{label}_ms_median"] = round(med[label], 4)
                    line[f"{label}_ms_min"] = round(min(t[label]), 4)
                    line[f"{label}_ms_max"] = round(max(t[label]), 4)
                    line[f"{label}_gpairs_per_s"] = round(n * nq / med[label] / 1e6, 2)
                line["loop_over_fused"] = round(med["loop"] / med["fused"], 3)
                line["ranges_apart"] = bool(max(t["fused"]) < min(t["loop"]) or max(t["loop"]) < min(t["fused"]))
                if raw_cutoff is not None:
                    line["u32_cutoff"] = raw_cutoff
                    line["fused_over_u32_fused"] = round(med["fused"] / med["u32_fused"], 3)
                line["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(line), flush=True)
                if out:
                    out.write(json.dumps(line) + "\n")
                    out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
