"""Thresholded matches for many queries: BatchComparator.filter_multi (rf_filter_multi_u32, tight-cutoff queries 4 to a pass over the corpus) against the same
queries through a loop of BatchComparator.filter_many (rf_filter_u32, one scan sequence and one host round trip per query), in ONE process and session, the
two alternating.  Both return host results, so each call ends in a device synchronise: the times are host wall-clock times around the calls
(time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported and the spread between repetitions is the
margin for "faster".  The rows of the two roads are compared once (`rows_equal`; `pairs` = how many (index, score) pairs that comparison covered).
Queries are near-copies (one substitution) of candidates of the corpus where it holds candidates of the query's length, random strings otherwise, so the rows
are not all empty.  One JSON line per measurement on stdout; --out appends them to a file.

    python tools/bench_filter_multi.py [--candidates 10000,10000000,100000000] [--ragged-candidates 10000000] [--queries 16,256] [--reps 5] [--warmup 1]
                                       [--shapes lev64,lev24,indel64,indel24,ragged_lev64,ragged_lev24,ragged_indel64,ragged_indel24]
                                       [--out profiles/filter_multi.txt]

Levenshtein runs under cutoff 3, Indel under cutoff 6.  Every line records RF_FILTER_MULTI as the process had it (the library reads it as on unless it is 0,
which would send filter_multi down the loop's road too).
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

SHAPES = {  # name: (metric, cutoff, query length, corpus: "rows" = single length 64, "ragged" = lengths 1..64)
    "lev64": ("levenshtein", 3, 64, "rows"), "lev24": ("levenshtein", 3, 24, "rows"), "indel64": ("indel", 6, 64, "rows"), "indel24": ("indel", 6, 24, "rows"),
    "ragged_lev64": ("levenshtein", 3, 64, "ragged"), "ragged_lev24": ("levenshtein", 3, 24, "ragged"),
    "ragged_indel64": ("indel", 6, 64, "ragged"), "ragged_indel24": ("indel", 6, 24, "ragged"),
}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="10000,10000000,100000000", help="sizes of the single-length corpora, comma-separated")
    ap.add_argument("--ragged-candidates", default="10000000", help="sizes of the ragged corpora, comma-separated")
    ap.add_argument("--queries", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "3 or more alternating repetitions"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []
    jobs = []  # (name, metric, cutoff, query length, kind, candidates)
    for name in args.shapes.split(","):
        metric, cutoff, qlen, kind = SHAPES[name]
        sizes = [int(x) for x in (args.ragged_candidates if kind == "ragged" else args.candidates).split(",") if x]
        jobs += [(name, metric, cutoff, qlen, kind, n) for n in sizes]
    jobs.sort(key=lambda j: (j[4], j[5]))  # (stable: the shapes of one corpus stay together and in the order given)
    held = {}
    for name, metric, cutoff, qlen, kind, n_rows in jobs:
        key = (kind, n_rows)
        if key not in held:
            held.clear()  # one corpus in HBM at a time
            torch.cuda.empty_cache()
            if kind == "ragged":
                data, offsets = synth.ragged_host(n_rows, 64, seed=0xC0FFEE03, min_len=1)
                lens = np.diff(offsets.astype(np.int64))
                by_len = {ln: np.nonzero(lens == ln)[0] for ln in {s[2] for s in SHAPES.values()}}

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
        mod = getattr(rf.distance, metric)
        for nq in [int(x) for x in args.queries.split(",")]:
            cs = [mod.BatchComparator(q) for q in queries_from(lambda j: pick(j, qlen), qlen, nq, 0xC0FFEE03)]
            fused = lambda: mod.BatchComparator.filter_multi(cs, N.OP_DISTANCE, corpus, score_cutoff=cutoff)  # noqa: E731
            loop = lambda: [c.filter_many(N.OP_DISTANCE, corpus, score_cutoff=cutoff) for c in cs]  # noqa: E731
            a, b = fused(), loop()  # (the rows compared; also the first warm-up of both)
            for _ in range(args.warmup):
                fused(), loop()
            same = all(x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() for x, y in zip(a, b))
            pairs = sum(len(y[0]) for y in b)
            t = {"fused": [], "loop": []}
            for _ in range(args.reps):  # alternating: both see the same clocks and the same neighbours
                for label, fn in (("fused", fused), ("loop", loop)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    t[label].append((time.perf_counter() - t0) * 1e3)
            n = len(corpus)
            med = {k_: statistics.median(v) for k_, v in t.items()}
            line = {"shape": name, "metric": metric, "cutoff": cutoff, "query_len": qlen, "corpus": kind, "candidates": n, "queries": nq, "reps": args.reps,
                    "warmup": args.warmup, "rows_equal": same, "pairs": pairs, "RF_FILTER_MULTI": os.environ.get("RF_FILTER_MULTI", "1")}
            for label in ("fused", "loop"):
                line[f"{label}_ms_median"] = round(med[label], 4)
                line[f"{label}_ms_min"] = round(min(t[label]), 4)
                line[f"{label}_ms_max"] = round(max(t[label]), 4)
                line[f"{label}_gpairs_per_s"] = round(n * nq / med[label] / 1e6, 2)
            line["loop_over_fused"] = round(med["loop"] / med["fused"], 3)
            line["ranges_apart"] = bool(max(t["fused"]) < min(t["loop"]) or max(t["loop"]) < min(t["fused"]))
            line["device"] = torch.cuda.get_device_name(0)
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
