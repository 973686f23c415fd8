"""Top-k of normalized scores for many queries: BatchComparator.topk_multi with a normalized op (rf_topk_multi_f64, fusable queries 4 to a pass over the
corpus, a 32-bit score image in the in-scan lists) against the same queries through a loop of BatchComparator.topk (rf_topk_f64: one scan into an n-entry
f64 vector, a radix selection and a host synchronization per query), in ONE process and session, the two alternating.  A third road is timed in the same
alternation for the usize metrics: topk_multi by raw similarity (rf_topk_multi_u32), the same fused kernel without the key computation at the tile's end --
`f64_over_u32_fused` is what the key costs.  All calls return host results, so each ends in a device synchronise: the times are host wall-clock times around
the calls (time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported and the spread between repetitions of
the loop is the margin for "not slower".  The rows of the fused road and the loop are compared once.  One JSON line per measurement on stdout; --out appends
each line to a file as soon as it exists.

    python tools/bench_topk_multi_f64.py [--candidates 100000000] [--ragged-candidates 100000000] [--small 10000[,...]] [--queries 16] [--k 16] [--reps 7]
                                         [--warmup 2] [--shapes indel64,indel24,lev64,lev24,ratio64,ratio24,ragged_indel,ragged_lev,ragged_ratio,small_...]
                                         [--out profiles/topk_multi_f64.txt]

Every line records RF_TOPK_MULTI as the process had it (the library reads it as on unless it is 0, which would send topk_multi down the loop's road too).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: F401
import torch

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth

# name: (metric, query length, corpus: "rows" = single length 64, "ragged" = lengths 1..64, "small" = rows of 64, once per size of --small); the score is
# normalized_similarity for levenshtein / indel and the similarity of fuzz::RatioBatchComparator for "ratio"
SHAPES = {}
for _m, _short in (("indel", "indel"), ("levenshtein", "lev"), ("ratio", "ratio")):
    SHAPES[f"{_short}64"] = (_m, 64, "rows")
    SHAPES[f"{_short}24"] = (_m, 24, "rows")
    SHAPES[f"ragged_{_short}"] = (_m, 64, "ragged")
    SHAPES[f"ragged_{_short}24"] = (_m, 24, "ragged")
    SHAPES[f"small_{_short}"] = (_m, 64, "small")
    SHAPES[f"small_{_short}24"] = (_m, 24, "small")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=100_000_000)
    ap.add_argument("--ragged-candidates", type=int, default=100_000_000)
    ap.add_argument("--small", default="10000", help="sizes of the small corpora, comma-separated")
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    corpora = {}
    jobs = []  # (name, metric, query length, kind, candidates)
    for name in args.shapes.split(","):
        metric, qlen, kind = SHAPES[name]
        sizes = [int(x) for x in args.small.split(",")] if kind == "small" else [args.ragged_candidates if kind == "ragged" else args.candidates]
        jobs += [(name, metric, qlen, kind, n) for n in sizes]
    jobs.sort(key=lambda j: (j[3], j[4]))  # (stable: the shapes of one corpus stay together and in the order given)
    for name, metric, qlen, kind, n_rows in jobs:
        kind = (kind, n_rows)
        if kind not in corpora:
            corpora.clear()  # one corpus in HBM at a time
            torch.cuda.empty_cache()
            if kind[0] == "ragged":
                data, offsets = synth.ragged_host(n_rows, 64, seed=0xC0FFEE02, min_len=1)
                corpora[kind] = rf.Corpus.from_ragged(data, offsets, device=0)
                del data, offsets
            else:
                corpora[kind] = rf.Corpus.from_device_rows(synth.rows_device(n_rows, 64, seed=0xC0FFEE02, device=dev))
        corpus = corpora[kind]
        cls = rf.fuzz.RatioBatchComparator if metric == "ratio" else getattr(rf.distance, metric).BatchComparator
        op = N.OP_SIMILARITY if metric == "ratio" else N.OP_NORMALIZED_SIMILARITY
        cs = [cls(synth.query(qlen, 0xC0FFEE02 + j)) for j in range(args.queries)]
        fused = lambda: cls.topk_multi(cs, corpus, args.k, op)  # noqa: E731
        loop = lambda: [c.topk(corpus, args.k, op) for c in cs]  # noqa: E731
        roads = [("fused", fused), ("loop", loop)]
        if metric != "ratio":  # the same kernel without the key: raw similarity through rf_topk_multi_u32
            roads.append(("u32_fused", lambda: cls.topk_multi(cs, corpus, args.k, N.OP_SIMILARITY)))
        a, b = fused(), loop()  # (the rows compared; also the first warm-up of both)
        for _ in range(args.warmup):
            for _label, fn in roads:
                fn()
        same = all(x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() for x, y in zip(a, b))
        t = {label: [] for label, _ in roads}
        for _ in range(args.reps):  # alternating: all see the same clocks and the same neighbours
            for label, fn in roads:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[label].append((time.perf_counter() - t0) * 1e3)
        n = len(corpus)
        med = {k_: statistics.median(v) for k_, v in t.items()}
        line = {"shape": name, "metric": metric, "query_len": qlen, "corpus": kind[0], "candidates": n, "queries": args.queries, "k": args.k, "reps": args.reps,
                "warmup": args.warmup, "rows_equal": same, "RF_TOPK_MULTI": os.environ.get("RF_TOPK_MULTI", "1")}
        for label in t:
            line[f"{label}_ms_median"] = round(med[label], 4)
            line[f"{label}_ms_min"] = round(min(t[label]), 4)
            line[f"{label}_ms_max"] = round(max(t[label]), 4)
            line[f"{label}_gpairs_per_s"] = round(n * args.queries / med[label] / 1e6, 2)
        line["loop_over_fused"] = round(med["loop"] / med["fused"], 3)
        if "u32_fused" in med:
            line["f64_over_u32_fused"] = round(med["fused"] / med["u32_fused"], 3)
        line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
