"""Throughput of damerau_levenshtein one-vs-many with bench.py's method (bench.py has no such metric choice): synthetic corpus from utils/synth,
warm-up, clock settle, ONE pair of HIP events on the launch stream around the timed steps, results left on the device.  Beside every shape the
yardsticks of the same session on the same box: Levenshtein with the weight table (1, 2, 3) -- wf_reg_kernel / wf_kernel, the kernels with the same
loop structure -- and, for context, the OSA scan.  One JSON line per measurement on stdout; --out appends them to a file.

    python tools/bench_dl.py [--candidates 20000000] [--steps 5] [--warmup 2] [--shapes q64,q32,q16,ragged,q256] [--out profiles/damerau_levenshtein.txt]
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
    "q64": (64, 64, 1.0), "q32": (32, 64, 1.0), "q16": (16, 64, 1.0), "ragged": (64, None, 1.0), "q256": (256, 256, 0.1),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=20_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle-ms", type=float, default=200.0)
    ap.add_argument("--shapes", default="q64,q32,q16,ragged,q256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    lines = []
    corpora = {}
    for name in args.shapes.split(","):
        qlen, clen, share = SHAPES[name]
        n = max(64, int(args.candidates * share))
        key = (clen, n)
        if key not in corpora:
            corpora.clear()  # one corpus in HBM at a time
            if clen is None:
                data, offsets = synth.ragged_host(n, 64, seed=0xC0FFEE02, min_len=1)
                corpora[key] = (rf.Corpus.from_ragged(data, offsets, device=0), float(np.diff(offsets.astype(np.int64)).mean()))
            else:
                corpora[key] = (rf.Corpus.from_device_rows(synth.rows_device(n, clen, seed=0xC0FFEE02, device=dev)), float(clen))
        corpus, mean_len = corpora[key]
        q = synth.query(qlen, 0xC0FFEE02)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        runs = [("damerau_levenshtein", rf.distance.damerau_levenshtein.BatchComparator(q), {}),
                ("levenshtein weights (1,2,3)", rf.distance.levenshtein.BatchComparator(q), {"weights": (1, 2, 3)}),
                ("osa", rf.distance.osa.BatchComparator(q), {})]
        for label, bc, kw in runs:
            steps = max(1, args.steps // 2) if name == "q256" else args.steps
            ms, settle_steps = timed(lambda: bc.many(N.OP_DISTANCE, corpus, out=out, **kw), stream, steps, args.warmup, args.settle_ms)
            line = {"shape": name, "metric": label, "query_len": qlen, "candidate_len": clen if clen else "1..64", "candidates": n, "kernel_ms": round(ms, 4),
                    "gpairs_per_s": round(n / ms / 1e6, 4), "gcells_per_s": round(n * mean_len * qlen / ms / 1e6, 2), "steps": steps, "warmup": args.warmup,
                    "settle_steps": settle_steps, "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
