"""Run by tests/test_gpu_filter_multi_f64.py in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  multitile   with RF_SCAN_BLOCKS_PER_CU=1: the construction of tests/filter_multi_check.py -- a corpus of (CUs x 4 x 3 + 1) x 64 - 27 candidates gives
              every wavefront of filter_multi_kernel at least 3 tiles and the first one a fourth, partial one.  Single-length corpora of 64 and of 20
              symbols and a ragged one; Levenshtein with queries of 64 and 20 symbols and Indel, q = 4, normalized_similarity >= 0.9, every row (indices,
              doubles as bit patterns) against the oracle's Somes.  The plan lines must show a fused group of 4 for every call, and the planted rows must
              leave tiles that live to their end beside tiles that die at the first look: both kinds are counted on the host.
  roads       default switches, a small corpus: tight lists of 7 queries (both ops, the ratio, weights (2, 2, 2) and (2, 2, 5)) run as groups [4,2] + 1
              per query; the loose-cutoff list, the no-cutoff list and the lists under (1, 2, 3) and (1024, 1024, 1024) go per query
  roads_off   the same lists with RF_FILTER_MULTI=0: every query per query, the same rows

Exit status 0 = all as expected.  The plan lines go to stderr; this process reads its own through a pipe."""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402
from filter_multi_check import plant, variants  # noqa: E402

GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel}
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY


class PlanLines:
    """what the library wrote to stderr (file descriptor 2) inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] filter_multi_f64:")]
        return False


def parse(line):
    m = re.search(r"q=(\d+) fused_groups=\[([0-9,]*)\] per_query=(\d+)", line)
    assert m, line
    return {"q": int(m.group(1)), "groups": [int(x) for x in m.group(2).split(",") if x], "per_query": int(m.group(3))}


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).tolist()


def somes(scores, order=N.FILTER_BY_INDEX, descending=True):
    """(indices, score bit patterns) of the oracle's Somes: ascending index, or best first with ties by index"""
    idx = np.nonzero(~np.isnan(scores))[0]
    if order == N.FILTER_BY_SCORE:
        v = scores[idx]
        idx = idx[np.lexsort((idx, -v if descending else v))]
    return idx.tolist(), bits(scores[idx])


def oracle_scores(ob, op, host, ragged, **kw):
    return ob.rows(op, host, nthreads=8, **kw) if host is not None else ob.many(op, ragged[0], ragged[1], nthreads=8, **kw)


def multitile():
    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = cus * 4
    n = (waves * 3 + 1) * 64 - 27
    print(f"{cus} CUs: {waves} wavefronts, {n} candidates = {-(-n // 64)} tiles", flush=True)
    rng = np.random.default_rng(20261019)
    q64, q20 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8)), bytes(rng.integers(97, 122, size=20, dtype=np.uint8))
    failures = 0
    for shape in ("rows64", "rows20", "ragged"):
        if shape != "ragged":
            ln, base = (64, q64) if shape == "rows64" else (20, q20)
            host = rng.integers(48, 122, size=(n, ln), dtype=np.uint8)

            def put(r, row):
                host[r] = row

            at = plant(rng, put, n, variants(base), 4099)
            corpus, ragged = rf.Corpus.from_device_rows(torch.from_numpy(host).cuda()), None
            tiles = -(-n // 64)
            planted_tiles = {r // 64 for r in at}
            runs = [("levenshtein", base), ("indel", base)]
        else:
            # lengths 1..64, the multiples of 16 and the queries' lengths more often than the rest: exact tiles of many lengths, a mixed section, tails of every size
            lens = np.where(rng.random(n) < 0.5, rng.choice([16, 20, 32, 48, 64], size=n), rng.integers(0, 65, size=n))
            for j, q in enumerate(variants(q64) + variants(q20)):
                lens[7 + 11 * j: n - 1: 4099] = len(q)
                lens[8 + 11 * j: n: 4099] = len(q)
            offsets = np.zeros(n + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(lens)
            data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)

            def put(r, row):
                assert int(offsets[r + 1]) - int(offsets[r]) == len(row), r
                data[int(offsets[r]): int(offsets[r + 1])] = row

            at = plant(rng, put, n, variants(q64) + variants(q20), 4099)
            host, ragged = None, (data, offsets)
            corpus = rf.Corpus.from_ragged(data, offsets)
            tiles = corpus.slot_count // 64
            slot_of = {int(c): s for s, c in enumerate(corpus.slot_index().tolist()) if c != 0xFFFFFFFF}
            planted_tiles = {slot_of[r] // 64 for r in at}
            runs = [("levenshtein", q64), ("levenshtein", q20), ("indel", q64), ("indel", q20)]
        assert tiles >= waves * 3 + 1, (tiles, waves)
        # tiles that hold a planted row live to their end for some member; the others hold random candidates only and die at the first look
        assert 0 < len(planted_tiles) < tiles, (len(planted_tiles), tiles)
        print(f"{shape}: {tiles} tiles, {len(planted_tiles)} with a planted row", flush=True)
        for metric, base in runs:
            qs = variants(base)
            cs = [GPU[metric].BatchComparator(q) for q in qs]
            with PlanLines() as pl:
                got = GPU[metric].BatchComparator.filter_multi(cs, NS, corpus, capacity=1024, score_cutoff=0.9)  # (one call: a row holds n / 4099 planted matches)
            bad = []
            total = 0
            for j, q in enumerate(qs):
                ei, es = somes(oracle_scores(ORA[metric].BatchComparator(q), NS, host, ragged, score_cutoff=0.9))
                total += len(ei)
                if got[j][0].tolist() != ei or bits(got[j][1]) != es:
                    bad.append((j, list(zip(got[j][0].tolist(), got[j][1].tolist()))[:4], ei[:4], len(got[j][0]), len(ei)))
            if total == 0:
                bad.append("no candidate passed: the case checks nothing")
            road = [parse(ln) for ln in pl.lines]
            if len(road) != 1 or road[0]["groups"] != [4] or road[0]["per_query"] != 0:
                bad.append(("road", pl.lines))
            print(f"{shape} {metric} len1={len(base)} x4 normalized_similarity >= 0.9, {total} pairs: {'ok' if not bad else bad}", flush=True)
            failures += len(bad)
        del corpus
    print("FAILURES", failures)
    return failures


def roads(off):
    rng = np.random.default_rng(7)
    n = 64 * 6 + 9
    host = rng.integers(48, 122, size=(n, 64), dtype=np.uint8)
    q64 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8))
    qs = variants(q64) + [q64[:20], q64[5:25], q64[:33]]

    def put(r, row):
        host[r] = np.resize(row, 64)

    plant(rng, put, n, qs, 53)
    corpus = rf.Corpus.from_rows(host)
    lev, ratio = rf.distance.levenshtein.BatchComparator, rf.fuzz.RatioBatchComparator
    # (class, op, cutoff, weights) -> the fused groups and the per-query count the plan must name: 4 of 64 symbols fused, the one of 33 left over, 2 of 20 fused
    fused = ([4, 2], 1)
    want = {
        "tight similarity": (lev, NS, 0.9, None, fused),
        "tight distance": (lev, ND, 0.1, None, fused),
        "ratio": (ratio, N.OP_SIMILARITY, 0.9, None, fused),
        "weights 2 2 2": (lev, NS, 0.9, (2, 2, 2), fused),
        "weights 2 2 5": (lev, NS, 0.9, (2, 2, 5), fused),
        "loose": (lev, NS, 0.2, None, ([], 7)),
        "nan": (lev, NS, None, None, ([], 7)),
        "weights 1 2 3": (lev, NS, 0.9, (1, 2, 3), ([], 7)),
        "weights 1024": (lev, NS, 0.9, (1024, 1024, 1024), ([], 7)),
    }
    for name, (cls, op, cutoff, weights, (groups, per_query)) in want.items():
        cs = [cls(q) for q in qs]
        for order in (N.FILTER_BY_INDEX, N.FILTER_BY_SCORE):
            with PlanLines() as pl:
                got = cls.filter_multi(cs, op, corpus, capacity=n, order=order, score_cutoff=cutoff, weights=weights)  # (room for every row: one call, one line)
            road = [parse(ln) for ln in pl.lines]
            assert len(road) == 1, (name, pl.text)
            if off:
                groups, per_query = [], 7
            assert road[0]["groups"] == groups and road[0]["per_query"] == per_query and road[0]["q"] == 7, (name, road)
            for j, q in enumerate(qs):
                kw = {} if cutoff is None else {"score_cutoff": cutoff}
                if weights is not None:
                    kw["weights"] = weights
                ob = o.fuzz.RatioBatchComparator(q) if cls is ratio else o.levenshtein.BatchComparator(q)
                s = oracle_scores(ob, NS if cls is ratio else op, host, None, **kw)
                ei, es = somes(s, order, descending=op != ND)
                assert got[j][0].tolist() == ei and bits(got[j][1]) == es, (name, j, order)
            if cutoff == 0.9:
                assert sum(len(i) for i, _ in got) > 0, name
    print("roads_off ok" if off else "roads ok")
    return 0


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    sys.exit(1 if (multitile() if mode == "multitile" else roads(mode == "roads_off")) else 0)
