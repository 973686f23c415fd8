"""Shared by tests/test_gpu_join_f64.py (imported) and run by it in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).
The inputs are tests/join_check.py's (lengths_case, edits, expected_groups); the expected triples are the CPU oracle's Somes, query by query, and every double
is compared by its bit pattern.

  lengths     default switches: the plan line "[rf plan] join_f64:" must show the 65-symbol query per query and the other eight in two groups (<= 32 symbols /
              33..64), for every (metric, op, cutoff) of LENGTH_CASES, and every triple must equal the oracle's
  off         the same with RF_JOIN=0: every query per query, identical triples
  long        the lengths corpus plus one candidate of 65 600 symbols: the eight rows stay fused (the join orders no 32-bit key, so no maximum is too large)
  batch       RF_JOIN_BATCH=8: m in {1, 2, 3, 4, 5, 8, 9, 17} rows of the fusable queries (repeats, any order); batches and groups as join_check.expected_groups
  multitile   RF_SCAN_BLOCKS_PER_CU=1: join_check.check_multitile's construction ((CUs x 12 + 1) x 64 - 27 candidates, single length 20 and ragged) under
              Levenshtein normalized_distance <= 0.2 -- a planted row has at most 3 substitutions in at least 15 symbols, so every one passes -- with more
              units (by the f64 length window) than workgroups, and tiles with and without a planted row

Exit status 0 = all as expected."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402
from join_check import PlanLines as _PlanLines, QUERY_LENGTHS, edits, expected_groups, lengths_case  # noqa: E402,F401

ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
INDEL_RATIO = rf.Args().ratio_indel_normalization()
# (metric, op, cutoff, weights); "ratio" / "ratio_indel" are fuzz::RatioBatchComparator without / with RF_FLAG_RATIO_INDEL_NORMALIZATION.  Every cutoff is tight
# for every query length: the normalized distance still allowed is below 0.4
LENGTH_CASES = ([(metric, op, cutoff, None) for metric in ("levenshtein", "indel", "lcs_seq") for op, cutoff in ((ND, 0.05), (ND, 0.1), (NS, 0.9), (NS, 0.95))]
                + [(metric, op, 0.9, None) for metric in ("ratio", "ratio_indel") for op in (N.OP_SIMILARITY, NS)]
                + [("levenshtein", ND, 0.1, (2, 2, 2)), ("levenshtein", NS, 0.9, (2, 2, 5))])


class PlanLines(_PlanLines):
    """the "[rf plan] join_f64:" lines the library wrote to stderr inside the block"""

    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] join_f64:")]
        return False


def parse(line):
    m = re.search(r"join_f64: m=(\d+) batches=(\d+) groups=(\d+) per_query=(\d+)", line)
    assert m, line
    return {"m": int(m.group(1)), "batches": int(m.group(2)), "groups": int(m.group(3)), "per_query": int(m.group(4))}


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).tolist()


def gpu_class(metric):
    return rf.fuzz.RatioBatchComparator if metric.startswith("ratio") else getattr(rf.distance, metric).BatchComparator


def join(metric, queries, corpus, op, cutoff, weights=None, **kw):
    """BatchComparator.join_f64 of the class `metric` names"""
    return gpu_class(metric).join_f64(queries, corpus, op, INDEL_RATIO if metric == "ratio_indel" else None, score_cutoff=cutoff, weights=weights, **kw)


def got_triples(res):
    """(query, candidate, bit pattern of the score)"""
    return list(zip(res[0].tolist(), res[1].tolist(), bits(res[2])))


class Oracle:
    """the oracle's Somes of one (metric, op, cutoff, weights) over one corpus, cached per query string; NaN = None"""

    def __init__(self, metric, op, cutoff, data, offsets, weights=None):
        self.metric, self.op, self.cutoff, self.data, self.offsets, self.weights = metric, op, cutoff, data, offsets, weights
        self.cache = {}

    def row(self, q):
        if q not in self.cache:
            kw = {"score_cutoff": self.cutoff}
            if self.metric == "ratio":  # fuzz.rs:141: the inner lcs_seq comparator's normalization, for both similarity ops
                v = o.fuzz.RatioBatchComparator(q).many(NS, self.data, self.offsets, nthreads=8, **kw)
            elif self.metric == "ratio_indel":  # the documented ratio
                v = o.indel.BatchComparator(q).many(NS, self.data, self.offsets, nthreads=8, **kw)
            else:
                if self.weights is not None:
                    kw["weights"] = self.weights
                v = getattr(o, self.metric).BatchComparator(q).many(self.op, self.data, self.offsets, nthreads=8, **kw)
            v = np.asarray(v, dtype=np.float64)
            idx = np.nonzero(~np.isnan(v))[0]
            self.cache[q] = (idx.tolist(), bits(v[idx]))
        return self.cache[q]

    def triples(self, queries, query_indices=None, upper=False, query_base=0, index_base=0):
        """ascending (position in Q, candidate index): lists of (query, candidate, bit pattern of the score)"""
        rows = range(len(queries)) if query_indices is None else query_indices
        out = []
        for qi in rows:
            idx, sc = self.row(queries[int(qi)])
            for j, v in zip(idx, sc):
                if not upper or j > int(qi):
                    out.append((query_base + int(qi), index_base + j, v))
        return out


def empty_pair_score(op):
    """(empty query, empty candidate): the maximum is 0, so the normalized distance is 0.0 and the similarity 1.0"""
    return bits([0.0 if op == ND else 1.0])[0]


def check_lengths(off, long_candidate=False):
    queries, cands = lengths_case()
    if long_candidate:
        cands = cands + [bytes(np.random.default_rng(65600).integers(48, 122, size=65600, dtype=np.uint8))]
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    empties = [j for j, c in enumerate(cands) if len(c) == 0]
    assert len(queries[0]) == 0 and empties
    failures = 0
    cases = LENGTH_CASES if not long_candidate else [c for c in LENGTH_CASES if c[2] in (0.1, 0.9)]
    for metric, op, cutoff, weights in cases:
        with PlanLines() as pl:
            got = got_triples(join(metric, qc, cc, op, cutoff, weights))
        exp = Oracle(metric, op, cutoff, data, offsets, weights).triples(queries)
        road = [parse(ln) for ln in pl.lines]
        want = {"m": 9, "batches": 0, "groups": 0, "per_query": 9} if off else {"m": 9, "batches": 1, "groups": 2, "per_query": 1}
        ok = got == exp and len(exp) > 0 and road and all(r == want for r in road)
        ok = ok and all((0, j, empty_pair_score(ND if op == ND else NS)) in got for j in empties)
        print(f"{metric} op {op} cutoff {cutoff} weights {weights}: {len(exp)} triples (got {len(got)}), plan {road}: {'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def check_batch():
    assert os.environ.get("RF_JOIN_BATCH") == "8", "run with RF_JOIN_BATCH=8"
    queries, cands = lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    rng = np.random.default_rng(5)
    failures = 0
    for metric, op, cutoff in (("levenshtein", NS, 0.9), ("indel", ND, 0.1), ("ratio", N.OP_SIMILARITY, 0.9)):
        ora = Oracle(metric, op, cutoff, data, offsets)
        for m in (1, 2, 3, 4, 5, 8, 9, 17):
            qi = rng.integers(0, 8, size=m)  # (rows 0..7: the fusable ones; repeats, any order)
            with PlanLines() as pl:
                got = got_triples(join(metric, qc, cc, op, cutoff, query_indices=qi))
            exp = ora.triples(queries, qi)
            batches, groups = expected_groups([QUERY_LENGTHS[int(i)] for i in qi], 8)
            road = [parse(ln) for ln in pl.lines]
            want = {"m": m, "batches": batches, "groups": groups, "per_query": 0}
            ok = got == exp and len(exp) > 0 and road and all(r == want for r in road)
            print(f"{metric} m={m} rows {qi.tolist()}: {len(exp)} triples, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
            failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def in_window(len1, tile_lens, slack):
    """a tile length L lies in the f64 length window of a query of len1 symbols iff |len1 - L| / max(len1, L) <= slack (0 / 0 counts as 0.0)"""
    tl = tile_lens.astype(np.float64)
    mx = np.maximum(tl, float(len1))
    nd = np.where(mx == 0, 0.0, np.abs(tl - float(len1)) / np.where(mx == 0, 1.0, mx))
    return nd <= slack


def window_units(tile_lens, qlens, slack, span=128):
    """units of the work list for Levenshtein normalized_distance <= slack: groups of 4 neighbours in length order within a class, the union of their windows --
    a window is the tile range from the first to the last tile whose length is in the query's window -- in spans of 128 tiles"""
    units = 0
    for cls in (True, False):
        part = sorted(x for x in qlens if (x <= 32) == cls)
        for i in range(0, len(part), 4):
            lo, hi = None, None
            for ln in part[i: i + 4]:
                hit = np.nonzero(in_window(ln, tile_lens, slack))[0]
                if len(hit):
                    lo = int(hit[0]) if lo is None else min(lo, int(hit[0]))
                    hi = int(hit[-1]) + 1 if hi is None else max(hi, int(hit[-1]) + 1)
            if lo is not None:
                units += -(-(hi - lo) // span)
    return units


def check_multitile():
    import torch

    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus * 12 + 1) * 64 - 27
    rng = np.random.default_rng(20261021)
    failures = 0
    for shape in ("rows20", "ragged"):
        if shape == "rows20":
            lens = np.full(n, 20)
            qlens = [17 + (j % 7) for j in range(64)]  # 17..23: |len1 - 20| / max(len1, 20) <= 3 / 20, so every window is the whole corpus
        else:
            lens = np.where(rng.random(n) < 0.5, rng.choice([16, 20, 32, 48, 64], size=n), rng.integers(0, 65, size=n))
            qlens = [int(x) for x in rng.choice([15, 16, 17, 19, 20, 21, 31, 32, 33, 34, 47, 48, 49, 62, 63, 64], size=320)]
        offsets = np.zeros(n + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lens)
        data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)
        # the queries: a handful of distinct strings per length (the oracle answers each once), near-copies of which are planted 4099 candidates apart
        by_len = {}
        queries = []
        for j, ln in enumerate(qlens):
            pool = by_len.setdefault(ln, [bytes(rng.integers(48, 122, size=ln, dtype=np.uint8)) for _ in range(2)])
            queries.append(pool[j % 2])
        same = {}
        for r in range(n):
            same.setdefault(int(lens[r]), []).append(r)
        planted = []
        for k, q in enumerate(sorted(set(queries))):
            assert len(q) >= 15
            rows = [r for r in same.get(len(q), [])[11 * k:: 4099]][:12]
            for i, r in enumerate(rows):
                row = np.frombuffer(q, dtype=np.uint8).copy()
                row[rng.integers(0, len(row), size=i % 4)] = 126  # at most 3 substitutions in at least 15 symbols: normalized distance <= 0.2
                data[int(offsets[r]): int(offsets[r + 1])] = row
                planted.append(r)
        corpus = rf.Corpus.from_ragged(data, offsets)
        qc = rf.Corpus.from_list(queries)
        slot_index = corpus.slot_index()  # (a single-length corpus lists its n candidates: the last tile's padding slots are added here)
        slot_index = np.concatenate([slot_index, np.full(-len(slot_index) % 64, 0xFFFFFFFF, dtype=slot_index.dtype)])
        tiles = len(slot_index) // 64
        first = slot_index.reshape(tiles, 64)
        tile_lens = np.array([int(lens[int(row[row != 0xFFFFFFFF][0])]) if (row != 0xFFFFFFFF).any() else 0 for row in first])
        slot_of = {int(c): s for s, c in enumerate(slot_index.tolist()) if c != 0xFFFFFFFF}
        planted_tiles = {slot_of[r] // 64 for r in planted}
        units = window_units(tile_lens, qlens, 0.2)
        print(f"{shape}: {cus} CUs, {n} candidates, {tiles} tiles ({len(planted_tiles)} with a planted row), {len(queries)} queries, {units} units", flush=True)
        assert tiles >= cus * 12 + 1 and 0 < len(planted_tiles) < tiles  # tiles with and without a planted row
        assert units > cus, "no workgroup would stage tables twice"
        ora = Oracle("levenshtein", ND, 0.2, data, offsets)
        with PlanLines() as pl:
            got = got_triples(join("levenshtein", qc, corpus, ND, 0.2))
        exp = ora.triples(queries)
        batches, groups = expected_groups(qlens, 16384)
        road = [parse(ln) for ln in pl.lines]
        want = {"m": len(queries), "batches": batches, "groups": groups, "per_query": 0}
        pairs = {(t[0], t[1]) for t in exp}
        all_planted = all(any((qi, r) in pairs for qi in range(len(queries))) for r in planted)
        ok = got == exp and all_planted and len(exp) >= len(planted) and road and all(r == want for r in road)
        print(f"{shape} levenshtein normalized_distance <= 0.2: {len(exp)} triples (got {len(got)}), every planted row passes: {all_planted}, plan {road}, want {want}: "
              f"{'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
        del corpus, qc
    print("FAILURES", failures)
    return failures


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    fn = {"lengths": lambda: check_lengths(False), "off": lambda: check_lengths(True), "long": lambda: check_lengths(False, True), "batch": check_batch,
          "multitile": check_multitile}[mode]
    sys.exit(1 if fn() else 0)
