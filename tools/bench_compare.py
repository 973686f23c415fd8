"""Throughput of the hamming / prefix / postfix scans (rf_compare.hip) with bench.py's method (bench.py has no such metric choice): synthetic corpus from
utils/synth, warm-up, clock settle, ONE pair of HIP events on the launch stream around the timed steps, results left on the device.  Beside every shape the
yardsticks of the same session on the same corpus: the no-cutoff Levenshtein and Indel distance scans.  One JSON line per measurement on stdout; --out
appends them to a file, followed by one line per shape that states the two sanity bounds these kernels were given in advance:
    hamming reads the bytes the Levenshtein scan reads and does far less arithmetic      -> hamming rate >= Levenshtein rate
    prefix / postfix read ONE chunk row per candidate of unrelated rows, hamming all     -> prefix, postfix rate > hamming rate

Bytes moved per candidate (`bytes_read`, `bytes_written`): what the kernel's loads and stores add up to from the shape alone -- hamming reads
ceil(min(len1, len2) / 16) chunks of 16 bytes, prefix and postfix the one chunk in which unrelated rows differ (16 symbols of a 62-symbol alphabet agree
with probability 62^-16), Levenshtein and Indel every chunk of the candidate; every scan writes one u32.

    python tools/bench_compare.py [--candidates 100000000] [--steps 5] [--warmup 2] [--shapes q64,q24,ragged] [--out profiles/compare_metrics.txt]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth

SHAPES = {  # name: (query length, candidate length or None = ragged 1..64, share of --candidates)
    "q64": (64, 64, 1.0), "q24": (24, 64, 1.0), "ragged": (64, None, 0.2),
}


def timed(fn, stream, steps, warmup, settle_ms):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, settle_steps = time.perf_counter(), 0
    while (time.perf_counter() - t0) * 1e3 < settle_ms:  # the set-up phase leaves the clock low
        fn()
        torch.cuda.synchronize()
        settle_steps += 1
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record(stream)
    for _ in range(steps):
        fn()
    ev1.record(stream)
    torch.cuda.synchronize()
    return ev0.elapsed_time(ev1) / steps, settle_steps


def chunks(lens):
    return (lens + 15) // 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle-ms", type=float, default=200.0)
    ap.add_argument("--shapes", default="q64,q24,ragged")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    pad = rf.Args().pad()
    for name in args.shapes.split(","):
        qlen, clen, share = SHAPES[name]
        n = max(64, int(args.candidates * share))
        if clen is None:
            data, offsets = synth.ragged_host(n, 64, seed=0xC0FFEE02, min_len=1)
            corpus = rf.Corpus.from_ragged(data, offsets, device=0)
            lens = np.diff(offsets.astype(np.int64))
            del data, offsets
        else:
            corpus = rf.Corpus.from_device_rows(synth.rows_device(n, clen, seed=0xC0FFEE02, device=dev))
            lens = np.full(1, clen, dtype=np.int64)  # (every candidate alike: the means below need one entry)
        all_chunks = float(chunks(lens).mean())
        common_chunks = float(chunks(np.minimum(lens, qlen)).mean())
        q = synth.query(qlen, 0xC0FFEE02)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        runs = [("hamming (pad)", rf.distance.hamming.BatchComparator(q), pad, common_chunks),
                ("prefix", rf.distance.prefix.BatchComparator(q), None, float((np.minimum(lens, qlen) > 0).mean())),
                ("postfix", rf.distance.postfix.BatchComparator(q), None, float((np.minimum(lens, qlen) > 0).mean())),
                ("levenshtein", rf.distance.levenshtein.BatchComparator(q), None, all_chunks),
                ("indel", rf.distance.indel.BatchComparator(q), None, all_chunks)]
        rate = {}
        for label, bc, a, read_chunks in runs:
            ms, settle_steps = timed(lambda: bc.many(N.OP_DISTANCE, corpus, a, out=out), stream, args.steps, args.warmup, args.settle_ms)
            moved = n * (16.0 * read_chunks + 4.0)
            rate[label] = n / ms / 1e6
            line = {"shape": name, "metric": label, "query_len": qlen, "candidate_len": clen if clen else "1..64", "candidates": n, "kernel_ms": round(ms, 4),
                    "gpairs_per_s": round(rate[label], 3), "bytes_read": round(n * 16.0 * read_chunks), "bytes_written": 4 * n,
                    "gbytes_per_s": round(moved / ms / 1e6, 1), "steps": args.steps, "warmup": args.warmup, "settle_steps": settle_steps,
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
        check = {"shape": name, "check": "sanity bounds", "hamming_at_least_levenshtein": rate["hamming (pad)"] >= rate["levenshtein"],
                 "prefix_above_hamming": rate["prefix"] > rate["hamming (pad)"], "postfix_above_hamming": rate["postfix"] > rate["hamming (pad)"]}
        print(json.dumps(check), flush=True)
        lines.append(check)
        del corpus, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
