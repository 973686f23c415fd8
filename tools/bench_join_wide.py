"""The join calls over `char` corpora, THIS build against the PARENT commit's library in one session: the parent answers every row of a `char` corpus down the
per-query road (a take, a comparator and a single-query scan with a host synchronization per row), this build fuses every row whose symbols the row map can place.
The two libraries cannot share a process (rapidfuzz_rs_amd loads the one RF_LIB names), so each measurement is a child process per library, the libraries
alternating as tools/ab.sh does, --rounds times; boxes differ by several percent, so only figures of one session are compared.

Measured: a self-join of `--queries` random rows (`join`, Levenshtein distance <= 2) and `join_topk` (Levenshtein distance, k = 1 and 16) over
  plain   1 M x 64 symbols drawn evenly from 120 symbols (Greek, Cyrillic, CJK): no overflow class, every row fuses
  zipf    the same shape over 3000 CJK symbols with probability ~ rank^-s (--zipf-s, default 2): the 254 most frequent are the alphabet, the rest the overflow
          class; `per_query_share` is the share of the query rows that hold an overflow symbol -- computed here from the symbols, by the packer's ranking rule
Every call returns host results, so it ends in a device synchronise: host wall-clock times (time.perf_counter) around the calls, one warm-up call first (at most
4096 rows: it loads the code objects), then up to --reps calls -- fewer once a measurement has taken --budget-s seconds, never less than one.  Each child prints
a checksum of what it returned; the parent process compares them between the libraries (`results_equal`).

--bytes: the byte-corpus shapes of profiles/join.txt that this change must not slow down (10 M x 64 single-length and ragged, 4096 rows, Levenshtein cutoff 2),
three runs per library alternating; `parent_spread_ms` is the spread of the three parent runs' medians and `within_spread` says whether this build's median of
medians is no slower than the parent's by more than that.

    python tools/bench_join_wide.py --parent-lib rapidfuzz_rs_amd/librfgpu_A.so [--candidates 1000000] [--queries 4096,65536] [--k 1,16] [--corpora plain,zipf]
                                    [--rounds 2] [--reps 3] [--out profiles/join_wide.txt]
    python tools/bench_join_wide.py --bytes --parent-lib rapidfuzz_rs_amd/librfgpu_A.so [--out profiles/join_wide.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

N_PLAIN, N_ZIPF, N_ALPHABET = 120, 3000, 254


def symbols_of(kind):
    if kind == "plain":
        return np.array([0x3B1 + i for i in range(24)] + [0x430 + i for i in range(32)] + [0x4E00 + i for i in range(N_PLAIN - 56)], dtype=np.uint32)
    return np.array([0x4E00 + i for i in range(N_ZIPF)], dtype=np.uint32)


def make_symbols(kind, n, length, zipf_s):
    """uint32 [n * length], seeded: the same corpus in every child"""
    rng = np.random.default_rng(0xC0FFEE05 if kind == "plain" else 0xC0FFEE06)
    table = symbols_of(kind)
    out = np.empty(n * length, dtype=np.uint32)
    cdf = None
    if kind == "zipf":
        p = np.arange(1, N_ZIPF + 1, dtype=np.float64) ** -zipf_s
        cdf = np.cumsum(p / p.sum())
    step = 1 << 23
    for at in range(0, len(out), step):
        m = min(step, len(out) - at)
        ids = rng.integers(0, N_PLAIN, size=m) if cdf is None else np.minimum(np.searchsorted(cdf, rng.random(m)), N_ZIPF - 1)
        out[at: at + m] = table[ids]
    return out


def overflow_share(data, length, qi):
    """share of the rows qi that hold a symbol outside the alphabet: the symbols ranked by count descending, then symbol ascending, the first 254 kept"""
    syms, counts = np.unique(data, return_counts=True)
    if len(syms) <= N_ALPHABET:
        return 0.0
    order = np.lexsort((syms, -counts.astype(np.int64)))
    rare = np.sort(syms[order[N_ALPHABET:]])
    rows = data.reshape(-1, length)[qi.astype(np.int64)]
    return float(np.isin(rows, rare).any(axis=1).mean())


def child(args):
    import torch

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N
    from rapidfuzz_rs_amd.utils import synth

    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.cuda.set_device(0)
    lev = rf.distance.levenshtein.BatchComparator
    lib = os.path.basename(N.LIB_PATH)
    n, length = args.candidates, 64

    def timed(fn):
        t = []
        while len(t) < args.reps and (not t or sum(t) < args.budget_s * 1e3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return t, res

    def measure(corpus, kind, nq, extra):
        qi = np.random.default_rng(nq).choice(n, size=nq, replace=False).astype(np.uint64)
        small = qi[: min(nq, 4096)]
        cap = 8 * nq  # (random rows of these corpora match themselves and little else)
        if args.bytes:  # a ragged corpus has many short rows within two edits of each other: count first
            lev.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, query_indices=qi, capacity=0)
            cap = max(int(lev.last_join_count), 1)
        ops = [("join_lev2", lambda rows: lev.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, query_indices=rows, capacity=cap))]
        ops += [(f"join_topk_k{k}", lambda rows, k=k: lev.join_topk(corpus, corpus, k, N.OP_DISTANCE, query_indices=rows)) for k in args.k]
        for name, fn in ops:
            fn(small)  # warm-up
            t, res = timed(lambda: fn(qi))
            if name == "join_lev2":
                assert lev.last_join_count <= cap, "the capacity cut the result"
                check = [int(lev.last_join_count), int(res[0].sum()), int(res[1].sum()), int(res[2].astype(np.uint64).sum())]
            else:
                cnt = res[2].astype(np.int64)
                keep = np.arange(res[0].shape[1])[None, :] < cnt[:, None]
                check = [int(cnt.sum()), int(res[0][keep].astype(np.uint64).sum()), int(res[1][keep].sum())]
            line = dict(extra, lib=lib, corpus=kind, op=name, candidates=n, queries=nq, ms=[round(x, 3) for x in t], check=check, device=torch.cuda.get_device_name(0))
            print("RESULT " + json.dumps(line), flush=True)

    if args.bytes:
        dev = torch.device("cuda", 0)
        for kind in ("rows", "ragged"):
            if kind == "ragged":
                data, offsets = synth.ragged_host(n, 64, seed=0xC0FFEE03, min_len=1)
                corpus = rf.Corpus.from_ragged(data, offsets, device=0)
                del data, offsets
            else:
                corpus = rf.Corpus.from_device_rows(synth.rows_device(n, 64, seed=0xC0FFEE03, device=dev))
            args.k = []
            for nq in args.queries:
                measure(corpus, kind, nq, {})
            del corpus
            torch.cuda.empty_cache()
        return
    for kind in args.corpora:
        data = make_symbols(kind, n, length, args.zipf_s)
        corpus = rf.Corpus.from_ragged_u32(data, np.arange(n + 1, dtype=np.uint64) * length, device=0)
        assert corpus.wide
        for nq in args.queries:
            qi = np.random.default_rng(nq).choice(n, size=nq, replace=False).astype(np.uint64)
            extra = {"distinct_symbols": int(len(np.unique(data))), "per_query_share": round(overflow_share(data, length, qi), 4)}
            if kind == "zipf":
                extra["zipf_s"] = args.zipf_s
            measure(corpus, kind, nq, extra)
        del corpus, data
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the parent commit's librfgpu.so (built from a checkout of that commit)")
    ap.add_argument("--candidates", type=int, default=None)
    ap.add_argument("--queries", default=None)
    ap.add_argument("--k", default="1,16")
    ap.add_argument("--corpora", default="plain,zipf")
    ap.add_argument("--zipf-s", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--budget-s", type=float, default=15.0)
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.candidates = args.candidates or (10_000_000 if args.bytes else 1_000_000)
    args.queries = [int(x) for x in (args.queries or ("4096" if args.bytes else "4096,65536")).split(",")]
    args.k = [int(x) for x in args.k.split(",") if x]
    args.corpora = args.corpora.split(",")
    args.rounds = args.rounds or (3 if args.bytes else 2)
    if args.child:
        return child(args)

    assert args.parent_lib and os.path.exists(args.parent_lib), "--parent-lib: the parent commit's library"
    libs = [("parent", os.path.abspath(args.parent_lib)), ("this", os.path.join(ROOT, "rapidfuzz_rs_amd", "librfgpu.so"))]
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--candidates", str(args.candidates), "--queries", ",".join(map(str, args.queries)), "--k",
            ",".join(map(str, args.k)), "--corpora", ",".join(args.corpora), "--zipf-s", str(args.zipf_s), "--reps", str(args.reps), "--budget-s", str(args.budget_s)]
    if args.bytes:
        argv.append("--bytes")
    runs = {}  # (corpus, op, queries) -> {"parent": [[ms of run 1], ...], "this": [...]} and the lines' other fields
    for rnd in range(args.rounds):
        for label, path in libs:
            env = {k: v for k, v in os.environ.items() if k != "RF_TRACE_PLAN"}
            r = subprocess.run(argv, capture_output=True, text=True, env=dict(env, RF_LIB=path), cwd=ROOT)
            assert r.returncode == 0, f"{label}, round {rnd}: {r.stdout[-2000:]}{r.stderr[-2000:]}"
            for ln in r.stdout.splitlines():
                if ln.startswith("RESULT "):
                    d = json.loads(ln[7:])
                    key = (d["corpus"], d["op"], d["queries"])
                    e = runs.setdefault(key, {"parent": [], "this": [], "check": {}, "meta": d})
                    e[label].append(d["ms"])
                    e["check"].setdefault(label, d["check"])
                    print(f"round {rnd} {label:6s} {d['corpus']:6s} {d['op']:14s} {d['queries']:6d} rows: {d['ms']} ms", flush=True)
    lines, failed = [], []
    for (corpus, op, nq), e in runs.items():
        meta = {k: v for k, v in e["meta"].items() if k not in ("lib", "ms", "check")}
        med = {label: [statistics.median(t) for t in e[label]] for label in ("parent", "this")}
        line = dict(meta, mode="bytes" if args.bytes else "char", rounds=args.rounds, results_equal=e["check"].get("parent") == e["check"].get("this"))
        for label in ("parent", "this"):
            flat = [x for t in e[label] for x in t]
            line[f"{label}_run_medians_ms"] = [round(x, 3) for x in med[label]]
            line[f"{label}_ms_median"] = round(statistics.median(med[label]), 3)
            line[f"{label}_ms_min"], line[f"{label}_ms_max"] = round(min(flat), 3), round(max(flat), 3)
        line["parent_over_this"] = round(line["parent_ms_median"] / line["this_ms_median"], 3)
        if args.bytes:
            line["parent_spread_ms"] = round(max(med["parent"]) - min(med["parent"]), 3)
            line["within_spread"] = bool(line["this_ms_median"] <= line["parent_ms_median"] + line["parent_spread_ms"])
            if not line["within_spread"]:
                failed.append(f"{corpus} {op}: {line['this_ms_median']} ms against the parent's {line['parent_ms_median']} ms (spread {line['parent_spread_ms']} ms)")
        elif meta.get("per_query_share", 0.0) == 0.0 and line["parent_over_this"] <= 1.0:
            failed.append(f"{corpus} {op} {nq} rows: the fused road is not faster than the parent ({line['this_ms_median']} ms against {line['parent_ms_median']} ms)")
        if not line["results_equal"]:
            failed.append(f"{corpus} {op} {nq} rows: the two libraries return different results")
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    assert not failed, "; ".join(failed)


if __name__ == "__main__":
    main()
