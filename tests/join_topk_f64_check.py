"""Shared by tests/test_gpu_join_topk_f64.py (imported) and run by it in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  lengths     default switches, tests/join_check.py lengths_case(): the plan line must show the 65-symbol row per query and the other eight in two groups
              (<= 32 symbols / 33..64) of one batch, for levenshtein / indel / lcs_seq with both normalized ops and for fuzz::ratio with both of its ops, with and
              without the Indel normalization; k = 65 sends every row per query; a loose cutoff keeps the rows fused (and leaves rows short of k), a tight one
              sends every row per query, NaN is no cutoff; Indel-like weights stay fused, a general weight table goes per query -- both equal to topk_multi of
              comparators over the same strings; every row must equal the oracle's
  off         the same inputs with RF_JOIN=0: every row per query, identical rows
  border      indel over a corpus whose longest candidate has 65471 bytes, then 65472: queries of 63 and 64 symbols.  64 + 65471 = 65535 is the largest maximum
              the 32-bit score image is exact for: every row fuses.  With 65472 the 64-symbol rows go per query and the 63-symbol rows stay fused
              (norm_key_fits is asked per row); k is beyond the corpus, so the long candidate -- the one whose maximum sits at the border -- is in every row
  batch       RF_JOIN_BATCH=8: m in {1, 2, 3, 4, 5, 8, 9, 17} rows of the fusable queries (repeats, any order); the plan line must show the batches and the
              groups the rule says there must be and every row must land at its position in Q
  multitile   RF_SCAN_BLOCKS_PER_CU=1 and RF_JOIN_TOPK_UNITS forced (256 units per group, or 1): tests/join_topk_check.py's corpora and queries.  Forced high,
              the plan line must show more units than workgroups and more than one unit per group; the rows must equal the oracle's either way.

Exit status 0 = all as expected.  The expected rows are the CPU oracle's: the full float64 many() row of the query, NaN (None) dropped, lexsorted by (score ascending
for the distance, descending for the similarity; then index), the first k -- compared bit for bit."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402
import join_check as J  # noqa: E402
import join_topk_check as T  # noqa: E402

ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
INDEL_RATIO = rf.Args().ratio_indel_normalization()
# "ratio" / "ratio_indel": fuzz::RatioBatchComparator without / with RF_FLAG_RATIO_INDEL_NORMALIZATION
GPU = {"levenshtein": rf.distance.levenshtein.BatchComparator, "indel": rf.distance.indel.BatchComparator, "lcs_seq": rf.distance.lcs_seq.BatchComparator,
       "osa": rf.distance.osa.BatchComparator, "jaro": rf.distance.jaro.BatchComparator, "jaro_winkler": rf.distance.jaro_winkler.BatchComparator,
       "ratio": rf.fuzz.RatioBatchComparator, "ratio_indel": rf.fuzz.RatioBatchComparator}
ORA = {"levenshtein": o.levenshtein.BatchComparator, "indel": o.indel.BatchComparator, "lcs_seq": o.lcs_seq.BatchComparator, "osa": o.osa.BatchComparator,
       "jaro": o.jaro.BatchComparator, "jaro_winkler": o.jaro_winkler.BatchComparator}
# the fused families with the ops each has
FUSED_OPS = [(m, op) for m in ("levenshtein", "indel", "lcs_seq") for op in (ND, NS)] + [(m, op) for m in ("ratio", "ratio_indel") for op in (N.OP_SIMILARITY, NS)]
# (metric, op) -> (loose, tight): plan() sets the early-out when the normalized distance a cutoff still allows is below 0.7 (Levenshtein) / 0.4 (the LCS family);
# the loose ones still answer None for most candidates of a random corpus
CUTOFFS = {("levenshtein", NS): (0.2, 0.9), ("levenshtein", ND): (0.8, 0.1), ("indel", NS): (0.5, 0.9), ("ratio", N.OP_SIMILARITY): (0.5, 0.9)}


def call_args(metric):
    return INDEL_RATIO if metric == "ratio_indel" else None


def descending(op):
    return op in (N.OP_SIMILARITY, NS)


class F64Oracle:
    """the oracle's float64 rows of one (metric, op, cutoff or None, weights or None) over one corpus, cached per query string: (indices, scores) of the Somes"""

    def __init__(self, metric, op, cutoff, data, offsets, weights=None):
        self.metric, self.op, self.data, self.offsets = metric, op, data, offsets
        self.kw = {}
        if cutoff is not None:
            self.kw["score_cutoff"] = cutoff
        if weights is not None:
            self.kw["weights"] = weights
        self.cache = {}

    def somes(self, q):
        if q not in self.cache:
            if self.metric == "ratio":  # fuzz.rs:141: the inner lcs_seq comparator's normalization; both of its ops return the same value
                full = o.fuzz.RatioBatchComparator(q).many(NS, self.data, self.offsets, nthreads=8, **self.kw)
            elif self.metric == "ratio_indel":  # the documented ratio
                full = o.indel.BatchComparator(q).many(NS, self.data, self.offsets, nthreads=8, **self.kw)
            else:
                full = ORA[self.metric](q).many(self.op, self.data, self.offsets, nthreads=8, **self.kw)
            assert full.dtype == np.float64
            idx = np.nonzero(~np.isnan(full))[0]
            self.cache[q] = (idx.astype(np.uint64), full[idx])
        return self.cache[q]

    def row(self, q, k, skip=None):
        """(scores, indices) of the k best, best first; `skip`: a candidate index that is not offered"""
        idx, sc = self.somes(q)
        if skip is not None:
            keep = idx != np.uint64(skip)
            idx, sc = idx[keep], sc[keep]
        order = np.lexsort((idx, -sc if descending(self.op) else sc))[:k]
        return sc[order], idx[order]


def mismatches(res, exp_rows, k, index_base=0):
    """positions of Q whose row differs from the expected (scores, indices): the doubles bit for bit"""
    scores, idx, cnt = res
    assert scores.dtype == np.float64 and idx.dtype == np.uint64 and cnt.dtype == np.uint32
    assert scores.shape == (len(exp_rows), k) and idx.shape == (len(exp_rows), k) and cnt.shape == (len(exp_rows),)
    bad = []
    for j, (es, ei) in enumerate(exp_rows):
        c = int(cnt[j])
        es = np.ascontiguousarray(es, dtype=np.float64)
        if c != len(es) or not (np.ascontiguousarray(scores[j, :c]).view(np.uint64) == es.view(np.uint64)).all() or not (idx[j, :c] == np.asarray(ei, dtype=np.uint64) + np.uint64(index_base)).all():
            bad.append(j)
    return bad


class PlanLines(J.PlanLines):
    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith("[rf plan] join_topk_f64:")]
        return False


def parse(line):
    m = re.search(r"join_topk_f64: m=(\d+) k=(\d+) batches=(\d+) groups=(\d+) units=(\d+) per_query=(\d+)", line)
    assert m, line
    return dict(zip(("m", "k", "batches", "groups", "units", "per_query"), (int(g) for g in m.groups())))


def join(metric, qc, cc, k, op, **kw):
    return GPU[metric].join_topk_f64(qc, cc, k, op, args=call_args(metric), **kw)


def check_lengths(off):
    queries, cands = J.lengths_case()
    assert b"" in cands and b"" in queries  # (a maximum of 0 occurs: the empty row against the empty candidate)
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    failures = 0

    def one(label, metric, op, k, cutoff, want, weights=None, exp=None):
        nonlocal failures
        with PlanLines() as pl:
            res = join(metric, qc, cc, k, op, score_cutoff=cutoff, weights=weights)
        if exp is None:
            ora = F64Oracle(metric, op, None if cutoff is None or np.isnan(cutoff) else cutoff, data, offsets, weights)
            exp = [ora.row(q, k) for q in queries]
        bad = mismatches(res, exp, k)
        road = [parse(ln) for ln in pl.lines]
        short = sum(1 for es, _ in exp if len(es) < k)
        ok = not bad and len(road) == 1 and all(road[0][key] == v for key, v in want.items())
        print(f"{label}: {metric} op {op} k {k} cutoff {cutoff} weights {weights}: rows differing {bad}, {short} rows short of k, plan {road}, want {want}: "
              f"{'ok' if ok else 'FAILED'}", flush=True)
        failures += 0 if ok else 1
        return exp

    per_query = {"m": 9, "batches": 0, "groups": 0, "units": 0, "per_query": 9}
    fused = per_query if off else {"m": 9, "batches": 1, "groups": 2, "units": 2, "per_query": 1}
    for metric, op in FUSED_OPS:
        one("no cutoff", metric, op, 3, None, dict(fused, k=3))
    one("k beyond the lists", "levenshtein", NS, 65, None, dict(per_query, k=65))
    for (metric, op), (loose, tight) in CUTOFFS.items():
        exp = one("loose cutoff", metric, op, 64, loose, dict(fused, k=64))
        if not any(len(es) < 64 for es, _ in exp):
            print("FAILED: the loose cutoff leaves no row short of k")
            failures += 1
        one("tight cutoff", metric, op, 3, tight, dict(per_query, k=3))
    one("NaN is no cutoff", "levenshtein", NS, 3, float("nan"), dict(fused, k=3))
    # weights: (2, 2, 5) runs as Indel x 2 and (2, 2, 2) as Levenshtein x 2 -- the maximum follows the weights -- and both fuse; (1, 2, 3) is a general table.  The
    # expectation is the sibling's: topk_multi(op = normalized) of comparators built from the same strings
    lev = GPU["levenshtein"]
    for weights, want in (((2, 2, 5), fused), ((2, 2, 2), fused), ((1, 2, 3), per_query)):
        for op in (ND, NS):
            sib = lev.topk_multi([lev(q) for q in queries], cc, 5, op, weights=weights)
            one("weights", "levenshtein", op, 5, None, dict(want, k=5), weights=weights, exp=sib)
            one("weights, the oracle", "levenshtein", op, 5, None, dict(want, k=5), weights=weights)
    print("FAILURES", failures)
    return failures


def border_case(longest):
    rng = np.random.default_rng(65535)
    queries = [bytes(rng.integers(97, 123, size=ln, dtype=np.uint8)) for ln in (63, 64, 63, 64, 63)]
    cands = [bytes(rng.integers(97, 123, size=int(ln), dtype=np.uint8)) for ln in (40, 0, 63, 64, 70, 12)]
    cands += [queries[0], queries[1][:60], J.edits(rng, queries[2], 2), J.edits(rng, queries[3], 3)]
    cands.insert(4, bytes(rng.integers(97, 123, size=longest, dtype=np.uint8)))  # (the queries' alphabet: a long common subsequence, a distance well below the maximum)
    return queries, cands


def check_border():
    failures = 0
    for longest, per_query, groups in ((65471, 0, 2), (65472, 2, 1)):
        queries, cands = border_case(longest)
        assert max(len(c) for c in cands) == longest and [len(q) for q in queries] == [63, 64, 63, 64, 63]
        qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
        data, offsets = rf.ragged(cands)
        for op in (ND, NS):
            ora = F64Oracle("indel", op, None, data, offsets)
            for k in (3, 16):  # (16: beyond the corpus -- the long candidate is in every row)
                with PlanLines() as pl:
                    res = join("indel", qc, cc, k, op)
                exp = [ora.row(q, k) for q in queries]
                bad = mismatches(res, exp, k)
                road = [parse(ln) for ln in pl.lines]
                want = {"m": 5, "k": k, "batches": 1, "groups": groups, "units": groups, "per_query": per_query}
                ok = not bad and road == [want] and (k == 3 or all(len(es) == len(cands) for es, _ in exp))
                print(f"longest {longest} indel op {op} k {k}: rows differing {bad}, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
                failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def check_batch():
    assert os.environ.get("RF_JOIN_BATCH") == "8", "run with RF_JOIN_BATCH=8"
    queries, cands = J.lengths_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    rng = np.random.default_rng(5)
    failures = 0
    for metric, op, k in (("levenshtein", NS, 3), ("ratio", N.OP_SIMILARITY, 7)):
        ora = F64Oracle(metric, op, None, data, offsets)
        for m in (1, 2, 3, 4, 5, 8, 9, 17):
            qi = rng.integers(0, 8, size=m)  # (rows 0..7: the fusable ones; repeats, any order)
            with PlanLines() as pl:
                res = join(metric, qc, cc, k, op, query_indices=qi)
            bad = mismatches(res, [ora.row(queries[int(i)], k) for i in qi], k)
            batches, groups = J.expected_groups([J.QUERY_LENGTHS[int(i)] for i in qi], 8)
            road = [parse(ln) for ln in pl.lines]
            want = {"m": m, "k": k, "batches": batches, "groups": groups, "units": groups, "per_query": 0}  # (fewer tiles than a span: one unit per group)
            ok = not bad and road == [want]
            print(f"{metric} m={m} rows {qi.tolist()}: rows differing {bad}, plan {road}, want {want}: {'ok' if ok else 'FAILED'}", flush=True)
            failures += 0 if ok else 1
    print("FAILURES", failures)
    return failures


def check_multitile(shape):
    import torch

    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    forced = int(os.environ["RF_JOIN_TOPK_UNITS"])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = (cus * 4 * 3 + 1) * 64 - 27
    rng = np.random.default_rng(20261022)
    qlens = T.MULTITILE_QLENS[shape]
    # (tests/join_topk_check.py check_multitile's shapes: the ragged corpus' shortest (20) and longest (44) candidates fill its first and last tile)
    lens = np.full(n, 20) if shape == "rows20" else np.where(rng.random(n) < 0.5, rng.choice([20, 24, 32, 40, 44], size=n), rng.integers(20, 45, size=n))
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)
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
    for metric, op in (("levenshtein", NS), ("indel", ND)):
        ora = F64Oracle(metric, op, None, data, offsets)
        with PlanLines() as pl:
            res = join(metric, qc, corpus, T.MULTITILE_K, op)
        exp = [ora.row(q, T.MULTITILE_K) for q in queries]
        # the planted candidates of the first and of the last tile are in every row's answer: a unit's list that is lost or misplaced changes it
        planted_in = all(set(ei.tolist()) & set(first) and set(ei.tolist()) & set(last) for _, ei in exp)
        bad = mismatches(res, exp, T.MULTITILE_K)
        road = [parse(ln) for ln in pl.lines]
        groups = T.multitile_groups(shape)
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
    fn = {"lengths": lambda: check_lengths(False), "off": lambda: check_lengths(True), "border": check_border, "batch": check_batch,
          "multitile_rows20": lambda: check_multitile("rows20"), "multitile_ragged": lambda: check_multitile("ragged")}[mode]
    sys.exit(1 if fn() else 0)
