"""Top-k for many queries: BatchComparator.topk_multi (rf_topk_multi_u32, fusable queries 4 to a pass over the corpus) against the same queries through a
loop of BatchComparator.topk (rf_topk_u32, one scan per query), in ONE process and session, the two alternating.  Both calls return host results, so each
ends in a device synchronise: the times are host wall-clock times around the calls (time.perf_counter), warm-up first, then --reps repetitions of each;
median, minimum and maximum are reported and the spread between repetitions is the margin for "faster".  The rows of the two roads are compared once.
One JSON line per measurement on stdout; --out appends them to a file.

    python tools/bench_topk_multi.py [--candidates 100000000] [--ragged-candidates 100000000] [--small 10000[,...]] [--queries 16] [--k 16] [--reps 7] [--warmup 2]
                                     [--shapes lev64,lev24,indel64,indel24,ragged_lev,ragged_indel,small_lev,small_lev24,small_indel,small_indel24]
                                     [--out profiles/topk_multi.txt]

Every line records RF_TOPK_MULTI as the process had it (the library reads it as on unless it is 0, which would send topk_multi down the loop's road too).
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
from rapidfuzz_rs_amd.utils import synth

SHAPES = {  # name: (metric, query length, corpus: "rows" = single length 64, "ragged" = lengths 1..64, "small" = rows of 64, once per size of --small)
    "lev64": ("levenshtein", 64, "rows"), "lev24": ("levenshtein", 24, "rows"), "indel64": ("indel", 64, "rows"), "indel24": ("indel", 24, "rows"),
    "ragged_lev": ("levenshtein", 64, "ragged"), "ragged_indel": ("indel", 64, "ragged"),
    "small_lev": ("levenshtein", 64, "small"), "small_lev24": ("levenshtein", 24, "small"), "small_indel": ("indel", 64, "small"),
    "small_indel24": ("indel", 24, "small"),
}


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
    lines = []
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
        mod = getattr(rf.distance, metric)
        cs = [mod.BatchComparator(synth.query(qlen, 0xC0FFEE02 + j)) for j in range(args.queries)]
        fused = lambda: mod.BatchComparator.topk_multi(cs, corpus, args.k)  # noqa: E731
        loop = lambda: [c.topk(corpus, args.k) for c in cs]  # noqa: E731
        a, b = fused(), loop()  # (the rows compared; also the first warm-up of both)
        for _ in range(args.warmup):
            fused(), loop()
        same = all(x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() for x, y in zip(a, b))
        t = {"fused": [], "loop": []}
        for _ in range(args.reps):  # alternating: both see the same clocks and the same neighbours
            for label, fn in (("fused", fused), ("loop", loop)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[label].append((time.perf_counter() - t0) * 1e3)
        n = len(corpus)
        med = {k_: statistics.median(v) for k_, v in t.items()}
        line = {"shape": name, "metric": metric, "query_len": qlen, "corpus": kind[0], "candidates": n, "queries": args.queries, "k": args.k, "reps": args.reps,
                "warmup": args.warmup, "rows_equal": same, "RF_TOPK_MULTI": os.environ.get("RF_TOPK_MULTI", "1")}
        for label in ("fused", "loop"):
            line[f"{label}_ms_median"] = round(med[label], 4)
            line[f"{label}_ms_min"] = round(min(t[label]), 4)
            line[f"{label}_ms_max"] = round(max(t[label]), 4)
            line[f"{label}_gpairs_per_s"] = round(n * args.queries / med[label] / 1e6, 2)
        line["loop_over_fused"] = round(med["loop"] / med["fused"], 3)
        line["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
