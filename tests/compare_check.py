"""Run by tests/test_gpu_compare.py::test_several_tiles_per_wavefront in a child process with RF_COMPARE_MAX_BLOCKS=1.

With the default grid a corpus of a few thousand candidates gives every wavefront of rf_compare.hip one tile: the tile loop's second pass -- the early-out
state re-armed, the hamming count reset, the next tile's shift and masks -- never runs in the other tests.  One workgroup makes four wavefronts walk every
tile of the corpus: a ragged corpus of 36 exact tiles + mixed blocks (9+ tiles per wavefront, lengths changing from tile to tile) and a single-length one.
Every value of every op is compared BY BITS with tests/compare_reference.py; the selecting roads run once over the same launch shape.

Exit status 0 = all equal.  Prints one line per (corpus, metric) so a failure names its kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402

import compare_reference as R  # noqa: E402

assert os.environ.get("RF_COMPARE_MAX_BLOCKS") == "1", "run with RF_COMPARE_MAX_BLOCKS=1"
MOD = {"hamming": rf.distance.hamming, "prefix": rf.distance.prefix, "postfix": rf.distance.postfix}
OPS = (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY)
failures = 0


def related(rng, q, length, i):
    fill = [int(v) for v in rng.integers(20, size=length)]
    p = int(rng.integers(0, min(len(q), length) + 1))
    if i % 3 == 0:
        return (q[:p] + fill[p:])[:length]
    if i % 3 == 1:
        return (fill[: length - p] + q[len(q) - p:])[:length] if p else fill
    c = (q + fill)[:length]
    for pos in rng.integers(0, max(length, 1), size=2 if length else 0):
        c[int(pos)] = 21
    return c


def check(tag, q, cands):
    global failures
    corpus = rf.Corpus.from_list([bytes(97 + v for v in c) for c in cands])
    rows, lens = R.pad_rows([[97 + v for v in c] for c in cands])
    qv = [97 + v for v in q]
    for metric in R.METRICS:
        bc = MOD[metric].BatchComparator(bytes(qv))
        bad = []
        for pad in ((False, True) if metric == "hamming" else (False,)):
            args = rf.Args().pad() if pad else None
            for op in OPS:
                uncut = R.ops(metric, op, qv, rows, lens, None, pad)
                some = uncut[R.keep(uncut)]
                cut = (int(np.median(some)) if op < 2 else float(np.median(some))) if some.size else None
                for cutoff in (None, cut):
                    exp = R.ops(metric, op, qv, rows, lens, cutoff, pad)
                    got = bc.many(op, corpus, args, score_cutoff=cutoff)
                    d = R.same_bits(got, exp)
                    if d.size:
                        bad.append((pad, op, cutoff, int(d.size), d[:4].tolist(), got[d[:4]].tolist(), exp[d[:4]].tolist()))
                # the selecting roads over the same launch shape
                exp = R.ops(metric, op, qv, rows, lens, cut, pad)
                keep = R.keep(exp)
                idx, sc = bc.filter_many(op, corpus, args, score_cutoff=cut)
                if idx.tolist() != keep.tolist() or R.same_bits(sc, exp[keep]).size:
                    bad.append((pad, op, "filter", idx[:4].tolist(), keep[:4].tolist()))
                desc = op in (N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY)
                order = sorted(keep.tolist(), key=lambda i: ((-float(exp[i]) if desc else float(exp[i])), i))[:7]
                scores, idx = bc.topk(corpus, 7, op=op, args=args, score_cutoff=cut)
                if idx.tolist() != order or R.same_bits(scores, exp[order]).size:
                    bad.append((pad, op, "topk", idx.tolist(), order))
        print(f"{tag} query {len(q)} {metric}: {'ok' if not bad else bad}", flush=True)
        failures += len(bad)


rng = np.random.default_rng(20261019)
for qlen in (23, 64, 70):
    q = [int(v) for v in rng.integers(20, size=qlen)]
    lengths = [L for L in (7, 16, 23, 40, 64, 65) for _ in range(64 * 6)] + [int(v) for v in rng.integers(0, 67, size=300)]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    check("ragged", q, [related(rng, q, L, i) for i, L in enumerate(lengths)])
    check("single length 40", q, [related(rng, q, 40, i) for i in range(64 * 30 + 5)])
print("FAILURES", failures)
sys.exit(1 if failures else 0)
