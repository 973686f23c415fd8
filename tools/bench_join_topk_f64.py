"""Every row's k best candidates by normalized score: BatchComparator.join_topk_f64 (rf_join_topk_f64: the queries stay in HBM, a work list per batch, four
register-resident lists per lane ordered by the 32-bit image of the score) against
  (a) `before`    the only route a caller had before it existed -- Corpus.take of the query rows, one BatchComparator per row, BatchComparator.topk_multi with the
                  same normalized op in chunks of 256 -- with the rows of the two compared once, bit for bit (`rows_equal`), and
  (b) `join_u32`  rf_join_topk_u32 on the same shape (the distance of the same kernel family: levenshtein for levenshtein, indel for the ratio): what the
                  normalized tile end and the host's decode cost over the u32 call.  Reported, not bounded.
in ONE process and session, the three alternating.  All return host results, so each call ends in a device synchronise: the times are host wall-clock times around
the calls (time.perf_counter), warm-up first, then --reps repetitions of each; median, minimum and maximum are reported, and road (a)'s own spread between
repetitions is the margin.  The queries are `--queries` rows of the corpus itself (random rows, as query_indices).  One JSON line per measurement on stdout; --out
appends them to a file.  A mismatch between the roads ends the run with an assertion -- after every shape has been measured and written; a shape on which
join_topk_f64 is slower than (a) by more than (a)'s spread is reported in its line (`join_within_bar`), not asserted: the expectation is no gate.

    python tools/bench_join_topk_f64.py [--candidates 1000000] [--queries 4096,65536] [--k 1,16] [--reps 3] [--warmup 1]
                                        [--shapes rows_lev,rows_ratio,ragged_lev,ragged_ratio] [--out profiles/join_topk_f64.txt]
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

LEV, INDEL, RATIO = rf.distance.levenshtein.BatchComparator, rf.distance.indel.BatchComparator, rf.fuzz.RatioBatchComparator
SHAPES = {  # name: (label, class, op, the u32 sibling's class, corpus: "rows" = single length 64, "ragged" = lengths 1..64)
    "rows_lev": ("levenshtein normalized_similarity", LEV, N.OP_NORMALIZED_SIMILARITY, LEV, "rows"),
    "rows_ratio": ("fuzz::ratio", RATIO, N.OP_SIMILARITY, INDEL, "rows"),
    "ragged_lev": ("levenshtein normalized_similarity", LEV, N.OP_NORMALIZED_SIMILARITY, LEV, "ragged"),
    "ragged_ratio": ("fuzz::ratio", RATIO, N.OP_SIMILARITY, INDEL, "ragged"),
}
CHUNK = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=1_000_000)
    ap.add_argument("--queries", default="4096")
    ap.add_argument("--k", default="1,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="rows_lev,rows_ratio")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.reps >= 3, "3 or more alternating repetitions"
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    n = args.candidates
    unequal = []
    held = {}
    for name in sorted(args.shapes.split(","), key=lambda s: SHAPES[s][4]):
        label, cls, op, u32_cls, kind = SHAPES[name]
        if kind not in held:
            held.clear()  # one corpus in HBM at a time
            torch.cuda.empty_cache()
            if kind == "ragged":
                data, offsets = synth.ragged_host(n, 64, seed=0xC0FFEE03, min_len=1)
                held[kind] = rf.Corpus.from_ragged(data, offsets, device=0)
                del data, offsets
            else:
                held[kind] = rf.Corpus.from_device_rows(synth.rows_device(n, 64, seed=0xC0FFEE03, device=dev))
        corpus = held[kind]
        for nq in [int(x) for x in args.queries.split(",")]:
            qi = np.random.default_rng(nq).choice(n, size=nq, replace=nq > n).astype(np.uint64)  # (more queries than rows: repeats)
            for k in [int(x) for x in args.k.split(",")]:

                def join():
                    return cls.join_topk_f64(corpus, corpus, k, op, query_indices=qi)

                def join_u32():
                    return u32_cls.join_topk(corpus, corpus, k, N.OP_DISTANCE, query_indices=qi)

                def before():
                    scores, idx, cnt = np.empty((nq, k), dtype=np.float64), np.empty((nq, k), dtype=np.uint64), np.empty(nq, dtype=np.uint32)
                    for at in range(0, nq, CHUNK):
                        cs = [cls(row) for row in corpus[qi[at: at + CHUNK]]]
                        for j, (sc, ix) in enumerate(cls.topk_multi(cs, corpus, k, op)):
                            scores[at + j, : len(sc)], idx[at + j, : len(sc)], cnt[at + j] = sc, ix, len(sc)
                    return scores, idx, cnt

                roads = [("join", join), ("before", before), ("join_u32", join_u32)]
                a, b = join(), before()  # (the rows compared; also the first warm-up of both)
                same = bool((a[2] == b[2]).all() and (a[2] == k).all() and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1]))
                if not same:
                    unequal.append(f"{name}, {nq} queries, k {k}")
                del a, b
                for _ in range(args.warmup):
                    for _, fn in roads:
                        fn()
                t = {lb: [] for lb, _ in roads}
                for _ in range(args.reps):  # alternating: all see the same clocks and the same neighbours
                    for lb, fn in roads:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        t[lb].append((time.perf_counter() - t0) * 1e3)
                med = {key: statistics.median(v) for key, v in t.items()}
                line = {"shape": name, "score": label, "corpus": kind, "candidates": n, "queries": nq, "k": k, "reps": args.reps, "warmup": args.warmup, "rows_equal": same}
                for lb, _ in roads:
                    line[f"{lb}_ms_median"] = round(med[lb], 3)
                    line[f"{lb}_ms_min"] = round(min(t[lb]), 3)
                    line[f"{lb}_ms_max"] = round(max(t[lb]), 3)
                line["join_queries_per_s"] = round(nq / med["join"] * 1e3, 1)
                line["before_spread_ms"] = round(max(t["before"]) - min(t["before"]), 3)
                line["before_over_join"] = round(med["before"] / med["join"], 3)
                line["join_within_bar"] = bool(med["join"] <= med["before"] + (max(t["before"]) - min(t["before"])))
                line["join_over_join_u32"] = round(med["join"] / med["join_u32"], 3)
                line["device"] = torch.cuda.get_device_name(0)
                print(json.dumps(line), flush=True)
                if args.out:  # (line by line: a run that is cut short keeps what it measured)
                    with open(args.out, "a") as f:
                        f.write(json.dumps(line) + "\n")
    assert not unequal, "join_topk_f64 and take + topk_multi return different rows: " + "; ".join(unequal)


if __name__ == "__main__":
    main()
