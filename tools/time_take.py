"""What reading candidates back out of a packed corpus costs: host time per rf_corpus_take call (the call synchronizes its stream, so the host clock around it is
the whole of it) for index lists of 16 / 1 024 / 1 048 576 random candidates and for the whole-corpus export, on a single-length corpus (n x 64) and a ragged one
(lengths uniform in 1..64), with host and with device output.  Every shape is warmed up, then repeated; median, fastest and slowest call are reported, with the
payload bytes delivered per second of the median next to them.  The sizing call (capacity 0: offsets only) is timed on its own.
    python tools/time_take.py [candidates] [--steps K] [--warmup W]        (profiles/corpus_take.txt is this script's output for 100 M)"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("candidates", nargs="?", type=int, default=100_000_000)
ap.add_argument("--steps", type=int, default=7, help="timed calls per shape (the whole-corpus export: at most 3)")
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()

import torch  # noqa: E402  (pay the one-off import before anything is timed)

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from rapidfuzz_rs_amd.utils import synth  # noqa: E402

assert torch.cuda.is_available(), "time_take.py measures on a GPU; there is no other road"
L = N.lib()
n = a.candidates


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # (rf_corpus_take synchronizes its stream before it returns)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def line(what, stats, nbytes):
    med, lo, hi = stats
    unit, k = ("us", 1e6) if med < 1e-3 else ("ms", 1e3)
    rate = f"{nbytes / med / 1e9:9.3f} GB/s of payload" if nbytes else ""
    print(f"  {what:58s} median {med * k:10.1f} {unit}  (fastest {lo * k:10.1f}, slowest {hi * k:10.1f})  {rate}", flush=True)


def measure(kind, corpus):
    rng = np.random.default_rng(7)
    print(f"==== {kind}: n={len(corpus)} payload={corpus.payload_bytes / 1e9:.2f} GB device_bytes={corpus.device_bytes / 1e9:.2f} GB", flush=True)
    for m in (16, 1024, 1 << 20, None):
        if m is not None and m > 64 * n:
            continue
        idx = None if m is None else rng.integers(0, n, m).astype(np.uint64)
        rows = n if m is None else m
        ptr = None if idx is None else idx.ctypes.data
        offsets = np.zeros(rows + 1, dtype=np.uint64)
        steps, warmup = (min(a.steps, 3), 1) if m is None else (a.steps, a.warmup)
        what = "whole corpus" if m is None else f"{m} random indices"

        def sizing():
            N.check(L.rf_corpus_take(corpus._h, ptr, rows, 0, None, 0, offsets.ctypes.data, N.MEM_HOST, None))

        line(f"{what}, sizing call (offsets only)", timed(sizing, steps, warmup), 0)
        total = int(offsets[rows])
        host = np.empty(total, dtype=np.uint8)
        host[:] = 0  # (touch the pages before anything is timed)
        dev = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        for where, out, mem in (("host", host.ctypes.data, N.MEM_HOST), ("device", dev.data_ptr(), N.MEM_DEVICE)):
            def take():
                N.check(L.rf_corpus_take(corpus._h, ptr, rows, 0, out, total, offsets.ctypes.data, mem, None))

            line(f"{what}, {where} output ({total / 1e6:.2f} MB)", timed(take, steps, warmup), total)
        del host, dev
    print(f"  device_bytes afterwards {corpus.device_bytes / 1e9:.2f} GB", flush=True)


rows64 = synth.rows_host(n, 64, seed=1)
corpus = rf.Corpus.from_rows(rows64)
del rows64
measure("rows64 (single length 64)", corpus)
del corpus
data, offs = synth.ragged_host(n, 64, seed=2, min_len=1)
corpus = rf.Corpus.from_ragged(data, offs)
del data, offs
measure("ragged (lengths 1..64)", corpus)
