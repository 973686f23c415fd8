"""Shared by tests/test_gpu_join_topk.py (imported) and run by it in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  lengths     default switches, tests/join_check.py lengths_case(): the plan line must show the 65-symbol row per query and the other eight in two groups
              (<= 32 symbols / 33..64) of one batch; k = 65 sends every row per query; a loose cutoff keeps the rows fused, a tight one (J.CUTOFFS) sends every
              row per query; every row must equal the oracle's
  off         the same inputs with RF_JOIN=0: every row per query, identical rows
  batch       RF_JOIN_BATCH=8: m in {1, 2, 3, 4, 5, 8, 9, 17} rows of the fusable queries (repeats, any order); the plan line must show the batches and the
              groups the rule says there must be -- sort by length, cut into eights, per batch ceil(narrow / 4) + ceil(wide / 4) -- and every row must land at
              its position in Q
  multitile   RF_SCAN_BLOCKS_PER_CU=1 and RF_JOIN_TOPK_UNITS forced (the parent passes 256 units per group: spans of about a dozen tiles; or 1: one unit per
              group): a corpus of (CUs x 4 x 3 + 1) x 64 - 27 candidates -- one of a single length of 20 symbols, one ragged -- and 40 queries of a dozen lengths
              whose near-copies are planted in the corpus' first and last tile.  Forced high, the plan line must show more units than workgroups and more than
              one unit per group: a workgroup stages tables more than once, a wavefront walks several tiles of a unit, a row's answer is selected out of several
              units' lists.  The rows must equal the oracle's either way.

Exit status 0 = all as expected.  The expected rows are the CPU oracle's: the full many() row of the query -- or tests/join_check.py Oracle's Somes under a cutoff --
lexsorted by (score ascending, or descending for the similarity; then index), the first k."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
import join_check as J  # noqa: E402

# (metric, op) -> a cutoff that is loose for every query length over a corpus whose longest candidate has 70 symbols (plan() sets no early-out) and still
# answers None for many candidates
LOOSE = {("levenshtein", N.OP_DISTANCE): 50, ("levenshtein", N.OP_SIMILARITY): 5, ("indel", N.OP_DISTANCE): 60}
MULTITILE_QLENS = {"rows20": [14 + (j % 12) for j in range(40)], "ragged": [27 + (j % 12) for j in range(40)]}
MULTITILE_K = 5


class TopkOracle:
    """the oracle's rows of one (metric, op, cutoff or None) over one corpus, cached per query string: (indices, scores) of the Somes"""

    def __init__(self, metric, op, cutoff, data, offsets):
        self.metric, self.op, self.cutoff, self.data, self.offsets = metric, op, cutoff, data, offsets
        self.cut = J.Oracle(metric, op, cutoff, data, offsets) if cutoff is not None else None
        self.cache = {}

    def somes(self, q):
        if self.cut is not None:
            return self.cut.row(q)
        if q not in self.cache:
            full = J.ORA[self.metric].BatchComparator(q).many(self.op, self.data, self.offsets, nthreads=8)
            assert (full != J.U64MAX).all()
            self.cache[q] = (np.arange(len(full), dtype=np.uint64), full.astype(np.uint32))
        return self.cache[q]

    def row(self, q, k, skip=None):
        """(scores, indices) of the k best, best first; `skip`: a candidate index that is not offered"""
        idx, sc = self.somes(q)
        if skip is not None:
            keep = idx != np.uint64(skip)
            idx, sc = idx[keep], sc[keep]
        key = sc.astype(np.int64)
        order = np.lexsort((idx, -key if self.op == N.OP_SIMILARITY else key))[:k]
        return sc[order], idx[order]


def mismatches(res, exp_rows, k, index_base=0):
    """positions of Q whose row differs from the expected (scores, indices)"""
    scores, idx, cnt = res
    assert scores.dtype == np.uint32 and idx.dtype == np.uint64 and cnt.dtype == np.uint32
    assert scores.shape == (len(exp_rows), k) and idx.shape == (len(exp_rows), k) and cnt.shape == (len(exp_rows),)
    bad = []
    for j, (es, ei) in enumerate(exp_rows):
        c = int(cnt[j])
        if c != len(es) or not (scores[j, :c] == es).all() or not (idx[j, :c] == ei + np.uint64(index_base)).all():
            bad.append(j)
    return bad


class TopkPlanLines(J.PlanLines):
    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] join_topk:")]
        return False


def parse(line):
    m = re.search(r"join_topk: m=(\d+) k=(\d+) batches=(\d+) groups=(\d+) units=(\d+) per_query=(\d+)", line)
    assert m, line
    return dict(zip(("m", "k", "batches", "groups", "units", "per_query"), (int(g) for g in m.groups())))


def check_lengths(off):
    queries, cands = J.lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    failures = 0

    def one(label, metric, op, k, cutoff, want):
        nonlocal failures
        ora = TopkOracle(metric, op, cutoff, data, offsets)
        with TopkPlanLines() as pl:
            res = J.GPU[metric].BatchComparator.join_topk(qc, cc, k, op, score_cutoff=cutoff)
        exp = [ora.row(q, k) for q in queries]
        bad = mismatches(res, exp, k)
        road = [parse(ln) for ln in pl.lines]
        short = sum(1 for es, _ in exp if len(es) < k)
        ok = not bad and len(road) == 1 and all(road[0][key] == v for key, v in want.items())
        print(f"{label}: {metric} op {op} k {k} cutoff {cutoff}: rows differing {bad}, {short} rows short of k, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
        return exp

    per_query = {"m": 9, "batches": 0, "groups": 0, "units": 0, "per_query": 9}
    fused = per_query if off else {"m": 9, "batches": 1, "groups": 2, "units": 2, "per_query": 1}
    for metric in ("levenshtein", "indel", "lcs_seq"):
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
            one("no cutoff", metric, op, 3, None, dict(fused, k=3))
    one("k beyond the lists", "levenshtein", N.OP_DISTANCE, 65, None, dict(per_query, k=65))
    for (metric, op), cutoff in LOOSE.items():
        exp = one("loose cutoff", metric, op, 64, cutoff, dict(fused, k=64))
        if not any(len(es) < 64 for es, _ in exp):
            print("FAILED: the loose cutoff leaves no row short of k")
            failures += 1
    for (metric, op), cutoffs in J.CUTOFFS.items():
        one("tight cutoff", metric, op, 3, cutoffs[1], dict(per_query, k=3))
    print("FAILURES", failures)
    return failures


def check_batch():
    assert os.environ.get("RF_JOIN_BATCH") == "8", "run with RF_JOIN_BATCH=8"
    queries, cands = J.lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    rng = np.random.default_rng(5)
    failures = 0
    for metric, op, k in (("levenshtein", N.OP_DISTANCE, 3), ("indel", N.OP_SIMILARITY, 7)):
        ora = TopkOracle(metric, op, None, data, offsets)
        for m in (1, 2, 3, 4, 5, 8, 9, 17):
            qi = rng.integers(0, 8, size=m)  # (rows 0..7: the fusable ones; repeats, any order)
            with TopkPlanLines() as pl:
                res = J.GPU[metric].BatchComparator.join_topk(qc, cc, k, op, query_indices=qi)
            bad = mismatches(res, [ora.row(queries[int(i)], k) for i in qi], k)
            batches, groups = J.expected_groups([J.QUERY_LENGTHS[int(i)] for i in qi], 8)
            road = [parse(ln) for ln in pl.lines]
            want = {"m": m, "k": k, "batches": batches, "groups": groups, "units": groups, "per_query": 0}  # (fewer tiles than a span: one unit per group)
            ok = not bad and road == [want]
            print(f"{metric} m={m} rows {qi.tolist()}: rows differing {bad}, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
            failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def multitile_groups(shape):
    return J.expected_groups(MULTITILE_QLENS[shape], 16384)[1]


def check_multitile(shape):
    import torch

    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    forced = int(os.environ["RF_JOIN_TOPK_UNITS"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus * 4 * 3 + 1) * 64 - 27
    rng = np.random.default_rng(20261022)
    qlens = MULTITILE_QLENS[shape]
    # the corpus' lengths; the ragged one's shortest (20) and longest (44) candidates fill its first and last tile
    lens = np.full(n, 20) if shape == "rows20" else np.where(rng.random(n) < 0.5, rng.choice([20, 24, 32, 40, 44], size=n), rng.integers(20, 45, size=n))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)
    # two distinct strings per length; query j is one of its length's two
    pool = {ln: [bytes(rng.integers(48, 122, size=ln, dtype=np.uint8)) for _ in range(2)] for ln in sorted(set(qlens))}
    queries = [pool[ln][(j // 12) % 2] for j, ln in enumerate(qlens)]
    distinct = sorted(set(queries))
    # the layout follows from the lengths alone: pack once to learn which candidates sit in the first and in the last tile, plant, pack again
    slot_index = rf.Corpus.from_ragged(data, offsets).slot_index()
    slot_index = np.concatenate([slot_index, np.full(-len(slot_index) % 64, 0xFFFFFFFF, dtype=slot_index.dtype)])
    tiles = len(slot_index) // 64
    first = [int(c) for c in slot_index[:64] if c != 0xFFFFFFFF]
    last = [int(c) for c in slot_index[-64:] if c != 0xFFFFFFFF]
    assert len(first) >= len(distinct) and len(last) >= len(distinct) and not set(first) & set(last)
    for i, q in enumerate(distinct):
        for r in (first[i], last[i]):  # the query cut or filled up ('~' is in no query) to the candidate's length
            ln = int(lens[r])
            data[int(offsets[r]): int(offsets[r + 1])] = np.frombuffer(q[:ln].ljust(ln, b"~"), dtype=np.uint8)
    corpus = rf.Corpus.from_ragged(data, offsets)
    qc = rf.Corpus.from_list(queries)
    failures = 0
    for metric, op in (("levenshtein", N.OP_DISTANCE), ("indel", N.OP_SIMILARITY)):
        ora = TopkOracle(metric, op, None, data, offsets)
        with TopkPlanLines() as pl:
            res = J.GPU[metric].BatchComparator.join_topk(qc, corpus, MULTITILE_K, op)
        exp = [ora.row(q, MULTITILE_K) for q in queries]
        # the planted candidates of the first and of the last tile are in every row's answer: a unit's list that is lost or misplaced changes it
        planted_in = all(set(ei.tolist()) & set(first) and set(ei.tolist()) & set(last) for _, ei in exp)
        bad = mismatches(res, exp, MULTITILE_K)
        road = [parse(ln) for ln in pl.lines]
        groups = multitile_groups(shape)
        ok = not bad and planted_in and len(road) == 1 and road[0]["groups"] == groups and road[0]["per_query"] == 0 and road[0]["batches"] == 1
        if forced == 1:
            ok = ok and road[0]["units"] == groups
        else:
            ok = ok and road[0]["units"] > cus and road[0]["units"] > 8 * groups
        print(f"{shape} {metric} op {op}: {cus} CUs, {n} candidates, {tiles} tiles, forced {forced}: rows differing {bad}, planted in every answer {planted_in}, "
              f"plan {road}, {groups} groups: {'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    fn = {"lengths": lambda: check_lengths(False), "off": lambda: check_lengths(True), "batch": check_batch,
          "multitile_rows20": lambda: check_multitile("rows20"), "multitile_ragged": lambda: check_multitile("ragged")}[mode]
    sys.exit(1 if fn() else 0)
