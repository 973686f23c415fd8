"""Run by tests/test_gpu_topk_multi.py in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  multitile   with RF_SCAN_BLOCKS_PER_CU=1 and RF_TOPK_SAMPLE=8.  topk_multi_kernel's grid is scan_grid(): at most CUs x RF_SCAN_BLOCKS_PER_CU
              workgroups of 4 wavefronts, so with the knob at 1 a corpus of (CUs x 4 x 3 + 1) x 64 - 27 candidates gives every wavefront at least
              3 tiles and the first one a fourth, partial one -- the chunk prefetched across tile ends, the state and `orig[]` re-armed per tile,
              the bound re-read between tiles, the lists carried from tile to tile.  A single-length corpus and a ragged one; Levenshtein with
              queries of 64 and 20 symbols and Indel, q = 4, k = 16, every row against the ranking of the oracle's scores.  The plan lines must
              show a fused group of 4 and a sample pass for every call: a loop over rf_topk_u32 would pass everything else.
  roads       default switches, a small corpus: a loose-cutoff list stays fused; the tight-cutoff list and the k = 65 list go per query
  roads_off   the same lists with RF_TOPK_MULTI=0: every query per query, the same rows

Exit status 0 = all as expected.  The plan lines go to stderr; this process reads its own through a pipe."""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402

GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel}
NONE32, U64MAX = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)


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
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] topk_multi:")]
        return False


def parse(line):
    m = re.search(r"q=(\d+) k=(\d+) fused_groups=\[([0-9,]*)\] per_query=(\d+) sample=(\d)", line)
    assert m, line
    return {"q": int(m.group(1)), "k": int(m.group(2)), "groups": [int(x) for x in m.group(3).split(",") if x], "per_query": int(m.group(4)),
            "sample": int(m.group(5))}


def ranking(scores, k, desc=False):
    s = np.where(scores == U64MAX, NONE32, scores.astype(np.uint32))
    idx = np.nonzero(s != NONE32)[0]
    v = s[idx].astype(np.int64)
    order = np.lexsort((idx, -v if desc else v))[:k]
    return s[idx][order].tolist(), idx[order].tolist()


def oracle_scores(metric, q, op, host, ragged, **kw):
    ob = ORA[metric].BatchComparator(q)
    return ob.rows(op, host, nthreads=8, **kw) if host is not None else ob.many(op, ragged[0], ragged[1], nthreads=8, **kw)


def variants(base):
    n = len(base)
    return [base, base[::-1], base[3:] + base[:3], base[: n // 2] + base[: n - n // 2]]


def plant(rng, rows_of, n, queries, every):
    """copies and near-copies (0..3 substitutions) of every query, `every` candidates apart: ties across tiles and wavefronts"""
    for j, q in enumerate(queries):
        for i, r in enumerate(range(7 + 11 * j, n, every)):
            row = np.frombuffer(q, dtype=np.uint8).copy()
            row[rng.integers(0, len(row), size=i % 4)] = 126
            rows_of(r, row)


def multitile():
    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1" and os.environ.get("RF_TOPK_SAMPLE") == "8", "run with RF_SCAN_BLOCKS_PER_CU=1 RF_TOPK_SAMPLE=8"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = cus * 4
    n = (waves * 3 + 1) * 64 - 27
    print(f"{cus} CUs: {waves} wavefronts, {n} candidates = {-(-n // 64)} tiles", flush=True)
    rng = np.random.default_rng(20261018)
    q64, q20 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8)), bytes(rng.integers(97, 122, size=20, dtype=np.uint8))
    failures = 0
    for shape in ("rows", "ragged"):
        if shape == "rows":
            host = rng.integers(48, 122, size=(n, 64), dtype=np.uint8)

            def put(r, row):
                host[r] = np.resize(row, 64)

            plant(rng, put, n, variants(q64) + variants(q20), 4099)
            corpus, ragged = rf.Corpus.from_device_rows(torch.from_numpy(host).cuda()), None
            tiles = -(-n // 64)
        else:
            # lengths 1..64, the multiples of 16 and the queries' lengths more often than the rest: exact tiles of many lengths, a mixed section, tails of every size
            lens = np.where(rng.random(n) < 0.5, rng.choice([16, 20, 32, 48, 64], size=n), rng.integers(0, 65, size=n))
            for j, q in enumerate(variants(q64) + variants(q20)):
                lens[7 + 11 * j:: 4099] = len(q)
            offsets = np.zeros(n + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(lens)
            data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)

            def put(r, row):
                data[int(offsets[r]): int(offsets[r + 1])] = row

            plant(rng, put, n, variants(q64) + variants(q20), 4099)
            host, ragged = None, (data, offsets)
            corpus = rf.Corpus.from_ragged(data, offsets)
            tiles = corpus.slot_count // 64
        assert tiles >= waves * 3 + 1, (tiles, waves)
        for metric, base in (("levenshtein", q64), ("levenshtein", q20), ("indel", q64)):
            qs = variants(base)
            cs = [GPU[metric].BatchComparator(q) for q in qs]
            for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
                with PlanLines() as pl:
                    got = GPU[metric].BatchComparator.topk_multi(cs, corpus, 16, op)
                bad = []
                for j, q in enumerate(qs):
                    es, ei = ranking(oracle_scores(metric, q, op, host, ragged), 16, op == N.OP_SIMILARITY)
                    if got[j][0].tolist() != es or got[j][1].tolist() != ei:
                        bad.append((j, list(zip(got[j][0].tolist(), got[j][1].tolist()))[:4], list(zip(es, ei))[:4]))
                road = [parse(ln) for ln in pl.lines]
                if len(road) != 1 or road[0]["groups"] != [4] or road[0]["per_query"] != 0 or road[0]["sample"] != 1:
                    bad.append(("road", pl.lines))
                print(f"{shape} {metric} len1={len(base)} op={op} x4 top-16: {'ok' if not bad else bad}", flush=True)
                failures += len(bad)
        del corpus
    print("FAILURES", failures)
    return failures


def roads(off):
    rng = np.random.default_rng(7)
    n = 64 * 6 + 9
    host = rng.integers(48, 122, size=(n, 64), dtype=np.uint8)
    q64 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8))
    qs = variants(q64) + [q64[:20], q64[5:25]]

    def put(r, row):
        host[r] = np.resize(row, 64)

    plant(rng, put, n, qs, 53)
    corpus = rf.Corpus.from_rows(host)
    lev = rf.distance.levenshtein.BatchComparator
    cs = [lev(q) for q in qs]
    # (list, k, cutoff) -> the fused groups and the per-query count the plan must name: 4 of 64 symbols + 2 of 20
    want = {"plain": (16, None, [4, 2], 0), "loose": (16, 48, [4, 2], 0), "tight": (16, 3, [], 6), "k65": (65, None, [], 6)}
    for name, (k, cutoff, groups, per_query) in want.items():
        with PlanLines() as pl:
            got = lev.topk_multi(cs, corpus, k, score_cutoff=cutoff)
        road = [parse(ln) for ln in pl.lines]
        assert len(road) == 1, (name, pl.text)
        if off:
            groups, per_query = [], 6
        assert road[0]["groups"] == groups and road[0]["per_query"] == per_query and road[0]["q"] == 6 and road[0]["k"] == k and road[0]["sample"] == 0, (name, road)
        for j, q in enumerate(qs):
            kw = {} if cutoff is None else {"score_cutoff": cutoff}
            es, ei = ranking(oracle_scores("levenshtein", q, N.OP_DISTANCE, host, None, **kw), k)
            assert got[j][0].tolist() == es and got[j][1].tolist() == ei, (name, j)
    print("roads_off ok" if off else "roads ok")
    return 0


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    sys.exit(1 if (multitile() if mode == "multitile" else roads(mode == "roads_off")) else 0)
