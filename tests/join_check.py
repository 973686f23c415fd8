"""Shared by tests/test_gpu_join.py (imported) and run by it in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  lengths     default switches, the inputs of the first test: the plan line must show the 65-symbol query per query and the other eight in two groups
              (<= 32 symbols / 33..64), and every triple must equal the oracle's
  off         the same inputs with RF_JOIN=0: every query per query, identical triples
  batch       RF_JOIN_BATCH=8: m in {1, 2, 3, 4, 5, 8, 9, 17} rows of the fusable queries (repeats, any order); the plan line must show the batches and the
              groups the rule says there must be -- sort by length, cut into batches of 8, per batch ceil(narrow / 4) + ceil(wide / 4)
  multitile   RF_SCAN_BLOCKS_PER_CU=1: join_kernel's grid is at most one workgroup per CU, a corpus of (CUs x 4 x 3 + 1) x 64 - 27 candidates -- one of a
              single length of 20 symbols, one ragged -- and so many queries of so many lengths that there are more units than workgroups: a workgroup
              stages tables more than once, a wavefront walks several tiles of a unit and several units.  Planted rows leave tiles that live to their end
              beside tiles that die at the first look (both kinds counted on the host).

Exit status 0 = all as expected.  The expected triples are the CPU oracle's Somes, query by query."""
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402

GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel, "lcs_seq": rf.distance.lcs_seq, "osa": rf.distance.osa}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel, "lcs_seq": o.lcs_seq, "osa": o.osa}
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
QUERY_LENGTHS = [0, 1, 5, 32, 33, 64, 64, 64, 65]
# (metric, op) -> two cutoffs, each tight for every query length over a corpus whose longest candidate has 70 symbols (plan()'s rule: the normalized
# distance still allowed below 0.7 for Levenshtein, 0.4 for the LCS family)
CUTOFFS = {("levenshtein", N.OP_DISTANCE): (1, 3), ("levenshtein", N.OP_SIMILARITY): (58, 62), ("indel", N.OP_DISTANCE): (2, 6), ("indel", N.OP_SIMILARITY): (120, 126),
           ("lcs_seq", N.OP_DISTANCE): (1, 3), ("lcs_seq", N.OP_SIMILARITY): (60, 64)}


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
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] join:")]
        return False


def parse(line):
    m = re.search(r"join: m=(\d+) batches=(\d+) groups=(\d+) per_query=(\d+)", line)
    assert m, line
    return {"m": int(m.group(1)), "batches": int(m.group(2)), "groups": int(m.group(3)), "per_query": int(m.group(4))}


class Oracle:
    """the oracle's Somes of one (metric, op, cutoff) over one corpus, cached per query string"""

    def __init__(self, metric, op, cutoff, data, offsets):
        self.metric, self.op, self.cutoff, self.data, self.offsets = metric, op, cutoff, data, offsets
        self.cache = {}

    def row(self, q):
        if q not in self.cache:
            bc = ORA[self.metric].BatchComparator(q)
            exp = bc.many(self.op, self.data, self.offsets, nthreads=8, score_cutoff=self.cutoff)
            if self.metric == "levenshtein" and self.op == N.OP_SIMILARITY:
                # Q2: above its cutoff the reference's Levenshtein similarity is a wrapped value where the device returns None: the expectation
                # is the oracle's own un-cut similarity, kept where it reaches the cutoff
                full = bc.many(self.op, self.data, self.offsets, nthreads=8)
                keep = full >= np.uint64(self.cutoff)
                assert (exp[keep] == full[keep]).all()
                exp = np.where(keep, full, U64MAX)
            idx = np.nonzero(exp != U64MAX)[0]
            self.cache[q] = (idx.astype(np.uint64), exp[idx].astype(np.uint32))
        return self.cache[q]

    def triples(self, queries, query_indices=None, upper=False, query_base=0, index_base=0):
        """ascending (position in Q, candidate index): lists of (query, candidate, score)"""
        rows = range(len(queries)) if query_indices is None else query_indices
        out = []
        for qi in rows:
            idx, sc = self.row(queries[int(qi)])
            for j, v in zip(idx.tolist(), sc.tolist()):
                if not upper or j > int(qi):
                    out.append((query_base + int(qi), index_base + j, v))
        return out


def got_triples(res):
    return list(zip(res[0].tolist(), res[1].tolist(), res[2].tolist()))


def edits(rng, q, k):
    """q after k random edits: substitutions, insertions and deletions ('~' is in no query and no random candidate)"""
    row = list(q)
    for _ in range(k):
        kind = int(rng.integers(0, 3))
        if kind == 0 and row:
            row[int(rng.integers(0, len(row)))] = 126
        elif kind == 1:
            row.insert(int(rng.integers(0, len(row) + 1)), 126)
        elif row:
            del row[int(rng.integers(0, len(row)))]
    return bytes(row)


def lengths_case():
    """queries of 0, 1, 5, 32, 33, 64, 64, 64 and 65 symbols as a packed corpus; ~300 candidates of 0..70 symbols with copies and near-copies of every query"""
    rng = np.random.default_rng(20261020)
    queries = [bytes(rng.integers(48, 122, size=ln, dtype=np.uint8)) for ln in QUERY_LENGTHS]
    cands = [bytes(rng.integers(48, 122, size=int(ln), dtype=np.uint8)) for ln in rng.integers(0, 71, size=307)]
    cands[0], cands[1] = bytes(rng.integers(48, 122, size=70, dtype=np.uint8)), b""
    at = 3
    for q in queries:
        for k in (0, 0, 1, 1, 2, 2, 3, 3):
            cands[at % len(cands)] = edits(rng, q, k)
            at += 37
    return queries, cands


def check_lengths(off):
    queries, cands = lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    failures = 0
    for (metric, op), cutoffs in CUTOFFS.items():
        for cutoff in cutoffs:
            with PlanLines() as pl:
                got = got_triples(GPU[metric].BatchComparator.join(qc, cc, op, score_cutoff=cutoff))
            exp = Oracle(metric, op, cutoff, data, offsets).triples(queries)
            road = [parse(ln) for ln in pl.lines]
            want = {"m": 9, "batches": 0, "groups": 0, "per_query": 9} if off else {"m": 9, "batches": 1, "groups": 2, "per_query": 1}
            ok = got == exp and len(exp) > 0 and road and all(r == want for r in road)
            print(f"{metric} op {op} cutoff {cutoff}: {len(exp)} triples, plan {road}: {'ok' if ok else 'FAILED'}", flush=True)
            failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def expected_groups(lens, batch):
    lens = sorted(lens)
    batches = groups = 0
    for i in range(0, len(lens), batch):
        part = lens[i: i + batch]
        narrow = sum(1 for x in part if x <= 32)
        groups += -(-narrow // 4) + -(-(len(part) - narrow) // 4)
        batches += 1
    return batches, groups


def check_batch():
    assert os.environ.get("RF_JOIN_BATCH") == "8", "run with RF_JOIN_BATCH=8"
    queries, cands = lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    rng = np.random.default_rng(5)
    failures = 0
    for metric, cutoff in (("levenshtein", 3), ("indel", 6)):
        ora = Oracle(metric, N.OP_DISTANCE, cutoff, data, offsets)
        for m in (1, 2, 3, 4, 5, 8, 9, 17):
            qi = rng.integers(0, 8, size=m)  # (rows 0..7: the fusable ones; repeats, any order)
            with PlanLines() as pl:
                got = got_triples(GPU[metric].BatchComparator.join(qc, cc, N.OP_DISTANCE, score_cutoff=cutoff, query_indices=qi))
            exp = ora.triples(queries, qi)
            batches, groups = expected_groups([QUERY_LENGTHS[int(i)] for i in qi], 8)
            road = [parse(ln) for ln in pl.lines]
            want = {"m": m, "batches": batches, "groups": groups, "per_query": 0}
            ok = got == exp and road and all(r == want for r in road)
            print(f"{metric} m={m} rows {qi.tolist()}: {len(exp)} triples, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
            failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def window_units(tile_lens, qlens, cutoff, span=128):
    """units of the work list for Levenshtein distance <= cutoff: groups of 4 neighbours in length order within a class, the union of their windows -- a window
    is the tile range from the first to the last tile whose length is within the cutoff of the query's -- in spans of 128 tiles"""
    units = 0
    for cls in (True, False):
        part = sorted(x for x in qlens if (x <= 32) == cls)
        for i in range(0, len(part), 4):
            lo, hi = None, None
            for ln in part[i: i + 4]:
                hit = np.nonzero(np.abs(tile_lens.astype(np.int64) - ln) <= cutoff)[0]
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
    n = (cus * 4 * 3 + 1) * 64 - 27
    rng = np.random.default_rng(20261021)
    failures = 0
    for shape in ("rows20", "ragged"):
        if shape == "rows20":
            lens = np.full(n, 20)
            qlens = [17 + (j % 7) for j in range(64)]  # 17..23: every window is the whole corpus under cutoff 3
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
            rows = [r for r in same.get(len(q), [])[11 * k:: 4099]][:12]
            for i, r in enumerate(rows):
                row = np.frombuffer(q, dtype=np.uint8).copy()
                row[rng.integers(0, len(row), size=i % 4)] = 126
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
        units = window_units(tile_lens, qlens, 3)
        print(f"{shape}: {cus} CUs, {n} candidates, {tiles} tiles ({len(planted_tiles)} with a planted row), {len(queries)} queries, {units} units", flush=True)
        assert tiles >= cus * 12 + 1 and 0 < len(planted_tiles) < tiles
        assert units > cus, "no workgroup would stage tables twice"
        ora = Oracle("levenshtein", N.OP_DISTANCE, 3, data, offsets)
        with PlanLines() as pl:
            got = got_triples(rf.distance.levenshtein.BatchComparator.join(qc, corpus, N.OP_DISTANCE, score_cutoff=3))
        exp = ora.triples(queries)
        batches, groups = expected_groups(qlens, 16384)
        road = [parse(ln) for ln in pl.lines]
        want = {"m": len(queries), "batches": batches, "groups": groups, "per_query": 0}
        ok = got == exp and len(exp) >= len(planted) and road and all(r == want for r in road)
        print(f"{shape} levenshtein cutoff 3: {len(exp)} triples (got {len(got)}), plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
        del corpus, qc
    print("FAILURES", failures)
    return failures


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    fn = {"lengths": lambda: check_lengths(False), "off": lambda: check_lengths(True), "batch": check_batch, "multitile": check_multitile}[mode]
    sys.exit(1 if fn() else 0)
