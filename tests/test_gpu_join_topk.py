"""rf_join_topk_u32 / BatchComparator.join_topk on the device: the k best candidates for every row of a packed corpus equal the CPU oracle's rows ranked by
(score, index) (tests/join_topk_check.py holds the oracle wrapper and the child-process checks that read the road from RF_TRACE_PLAN).

  lengths and classes   queries of 0, 1, 5, 32, 33, 64, 64, 64 and 65 symbols against 307 ragged candidates; three metrics x two ops x k in {1, 3, 64}
  k                     beyond the corpus (40 candidates, k = 64) and beyond the lists (k = 65: per query)
  ties                  200 identical candidates on both sides, single-length and length-bucketed, with and without no_self
  units                 one workgroup per CU, units forced: several tiles per wavefront, several units per workgroup and per row; and one unit per group
  batch borders         RF_JOIN_BATCH=8 with 1 .. 17 rows
  no_self               compares with the row index, not the position in Q; both roads
  renaming              corpora with different symbol-frequency ranks, bytes 0x00 and 0xFF, query symbols the scanned corpus never stores; both directions
  cutoffs               loose: fused, with rows short of k; tight: per query
  per-query road        osa, a `char` corpus on either side: equal to the loop of topk(); RF_JOIN=0 equal to the default
  bases and empties     an index base beyond 32 bits, an index out of range, either corpus empty
  the sibling           equal to topk_multi of comparators built from the same byte strings"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import join_check as J  # noqa: E402
import join_topk_check as T  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEV = rf.distance.levenshtein.BatchComparator


@functools.lru_cache(maxsize=None)
def lengths():
    queries, cands = J.lengths_case()
    data, offsets = rf.ragged(cands)
    return queries, cands, rf.Corpus.from_list(queries), rf.Corpus.from_list(cands), data, offsets


@functools.lru_cache(maxsize=None)
def lengths_oracle(metric, op):
    _, _, _, _, data, offsets = lengths()
    return T.TopkOracle(metric, op, None, data, offsets)


@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
@pytest.mark.parametrize("metric", ["levenshtein", "indel", "lcs_seq"])
def test_rows_equal_the_oracle(metric, op, k):
    queries, _, qc, cc, _, _ = lengths()
    res = J.GPU[metric].BatchComparator.join_topk(qc, cc, k, op)
    exp = [lengths_oracle(metric, op).row(q, k) for q in queries]
    assert all(len(es) == k for es, _ in exp)
    assert T.mismatches(res, exp, k) == []


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_topk_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, r.stdout[-4000:] + r.stderr[-3000:]
    return r


def test_the_plan_line_shows_the_roads_with_and_without_cutoffs():
    _child("lengths")


def test_join_off_sends_everything_per_query_with_identical_results():
    _child("off", RF_JOIN="0")


def test_group_and_batch_borders():
    _child("batch", RF_JOIN_BATCH="8")


@pytest.mark.parametrize("shape", ["rows20", "ragged"])
def test_several_tiles_per_wavefront_and_several_units_per_row(shape):
    _child("multitile_" + shape, RF_SCAN_BLOCKS_PER_CU="1", RF_JOIN_TOPK_UNITS=str(256 * T.multitile_groups(shape)))


@pytest.mark.parametrize("shape", ["rows20", "ragged"])
def test_one_unit_per_group_gives_identical_rows(shape):
    _child("multitile_" + shape, RF_SCAN_BLOCKS_PER_CU="1", RF_JOIN_TOPK_UNITS="1")


def test_k_beyond_the_corpus_and_beyond_the_lists():
    queries, cands, qc, cc, data, offsets = lengths()
    small = cands[:40]
    sdata, soffsets = rf.ragged(small)
    res = LEV.join_topk(qc, rf.Corpus.from_list(small), 64)
    assert (res[2] == 40).all()
    ora = T.TopkOracle("levenshtein", N.OP_DISTANCE, None, sdata, soffsets)
    assert T.mismatches(res, [ora.row(q, 64) for q in queries], 64) == []
    # k = 65: the lists hold 64, every row goes per query
    res = LEV.join_topk(qc, cc, 65)
    assert T.mismatches(res, [lengths_oracle("levenshtein", N.OP_DISTANCE).row(q, 65) for q in queries], 65) == []


@pytest.mark.parametrize("bucketed", [False, True])
def test_ties_go_to_the_smaller_index(bucketed):
    """200 identical 20-byte candidates -- 3 full tiles and a partial one -- as both sides: every candidate ties at score 0"""
    rows = [b"the same twenty bytes"[:20]] * 200 + ([b"another"] if bucketed else [])
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    ora = T.TopkOracle("levenshtein", N.OP_DISTANCE, None, data, offsets)
    scores, idx, cnt = LEV.join_topk(corpus, corpus, 5)
    assert (cnt == 5).all() and (scores[:200] == 0).all() and (idx[:200] == np.arange(5, dtype=np.uint64)).all()
    assert T.mismatches((scores, idx, cnt), [ora.row(q, 5) for q in rows], 5) == []
    scores, idx, cnt = LEV.join_topk(corpus, corpus, 5, no_self=True)
    for r in range(200):
        assert idx[r].tolist() == [i for i in range(6) if i != r][:5] and (scores[r] == 0).all(), r
    assert T.mismatches((scores, idx, cnt), [ora.row(q, 5, skip=r) for r, q in enumerate(rows)], 5) == []


def test_no_self_compares_with_the_row_index_not_the_position_in_q():
    """One corpus on both sides with exact duplicates of some rows, so that self is not the only candidate at distance 0; rows in any order and repeated, no
    position equal to its row index: a compare against the position (or a wrongly filled row index in the work list) changes the rows.  Both roads: fused
    rows and the 65-symbol row."""
    queries, cands, _, _, _, _ = lengths()
    rows = queries + cands[:120] + [queries[3], queries[7], queries[8], cands[40 - 9], queries[0]]  # (duplicates of rows 3, 7, 8, 40 and 0)
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    qi = [40, 7, 3, 8, 7, 128, 0, 5, 3, 77, 6, 4]
    assert all(p != r for p, r in enumerate(qi))
    for k in (1, 4):
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
            ora = T.TopkOracle("levenshtein", op, None, data, offsets)
            plain = [ora.row(rows[r], k) for r in qi]
            exp = [ora.row(rows[r], k, skip=r) for r in qi]
            wrong = [ora.row(rows[r], k, skip=p) for p, r in enumerate(qi)]
            differ = lambda a, b: any(x[1].tolist() != y[1].tolist() for x, y in zip(a, b))  # noqa: E731
            assert differ(exp, plain) and differ(exp, wrong)
            assert T.mismatches(LEV.join_topk(corpus, corpus, k, op, query_indices=qi), plain, k) == []
            assert T.mismatches(LEV.join_topk(corpus, corpus, k, op, query_indices=qi, no_self=True), exp, k) == []
    # a row with a duplicate still finds a record at distance 0, and never itself
    res = LEV.join_topk(corpus, corpus, 1, query_indices=[3, 8, 129, 131], no_self=True)
    assert (res[0][:, 0] == 0).all() and all(int(i) != r for i, r in zip(res[1][:, 0], [3, 8, 129, 131]))


def test_renaming_between_two_corpora():
    """the query corpus is mostly 'z' and 0xFF, the scanned corpus mostly 'a' and 0x00: their frequency ranks -- the stored symbols -- differ; the queries hold
    symbols (0xFF, 'q') the scanned corpus never stores"""
    rng = np.random.default_rng(9)
    qa, ca = np.array([122, 255, 0, 97, 113, 98], dtype=np.uint8), np.array([97, 0, 98, 122, 99, 100], dtype=np.uint8)
    queries = [bytes(qa[np.minimum(rng.geometric(0.45, size=ln) - 1, 5)]) for ln in rng.integers(3, 41, size=24)]
    cands = [bytes(ca[np.minimum(rng.geometric(0.45, size=int(ln)) - 1, 5)]) for ln in rng.integers(0, 45, size=260)]
    at = 1
    for q in queries:  # near-copies: the symbols the scanned corpus lacks turned into ones it has, or left out
        cands[at % 260] = q.replace(b"\xff", b"\x00").replace(b"q", b"c")
        cands[(at + 7) % 260] = q.replace(b"\xff", b"").replace(b"q", b"")
        at += 11
    assert not any(b"\xff" in c or b"q" in c for c in cands) and any(b"\xff" in q for q in queries) and any(b"\x00" in c for c in cands)
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    for metric, op in (("levenshtein", N.OP_DISTANCE), ("indel", N.OP_SIMILARITY)):
        ora = T.TopkOracle(metric, op, None, data, offsets)
        assert T.mismatches(J.GPU[metric].BatchComparator.join_topk(qc, cc, 3, op), [ora.row(q, 3) for q in queries], 3) == []
    # and the other way round: the roles of the two corpora swapped
    data, offsets = rf.ragged(queries)
    ora = T.TopkOracle("levenshtein", N.OP_DISTANCE, None, data, offsets)
    assert T.mismatches(LEV.join_topk(cc, qc, 3), [ora.row(c, 3) for c in cands], 3) == []


def _loop_of_topk(cls, queries, corpus, k, op):
    return [cls(q).topk(corpus, k, op) for q in queries]


def test_per_query_road_equals_the_loop_of_topk():
    queries, cands, qc, cc, _, _ = lengths()
    osa = rf.distance.osa.BatchComparator  # osa has no fused kernel
    for k, op in ((4, N.OP_DISTANCE), (70, N.OP_SIMILARITY)):
        assert T.mismatches(osa.join_topk(qc, cc, k, op), _loop_of_topk(osa, queries, cc, k, op), k) == []
    # a `char` corpus, on either side
    greek = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()]
    rng = np.random.default_rng(4)
    wq = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=ln)) for ln in (0, 3, 20, 40)]
    wc = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=int(ln))) for ln in rng.integers(0, 45, size=150)]
    for j, q in enumerate(wq):
        wc[5 + 9 * j] = q
        wc[6 + 9 * j] = q[1:] + "Ω"
    wqc, wcc = rf.Corpus.from_list(wq), rf.Corpus.from_list(wc)
    res = LEV.join_topk(wqc, wcc, 4)
    assert T.mismatches(res, _loop_of_topk(LEV, wq, wcc, 4, N.OP_DISTANCE), 4) == []
    assert res[1][1:, 0].tolist() == [5 + 9 * j for j in range(1, 4)] and (res[0][1:, 0] == 0).all()
    # ... and with no_self on a `char` corpus joined with itself: the per-query road drops the row's own entry
    res = LEV.join_topk(wcc, wcc, 3, no_self=True, query_indices=[5 + 9 * 2, 6 + 9 * 2, 0])
    exp = []
    for r in (5 + 9 * 2, 6 + 9 * 2, 0):
        sc, ix = LEV(wc[r]).topk(wcc, 4)
        keep = ix != r
        exp.append((sc[keep][:3], ix[keep][:3]))
    assert T.mismatches(res, exp, 3) == []


def test_index_base_indices_out_of_range_and_empties():
    queries, _, qc, cc, _, _ = lengths()
    ora = lengths_oracle("levenshtein", N.OP_DISTANCE)
    qi = [7, 2, 7, 0, 8, 3, 3, 5]  # unordered, repeats, the 65-symbol row among them
    base = 2**32 + 5
    res = LEV.join_topk(qc, cc, 6, query_indices=qi, index_base=base)
    assert T.mismatches(res, [ora.row(queries[r], 6) for r in qi], 6, index_base=base) == []
    assert int(res[1].min()) >= base
    with pytest.raises(rf.RfError) as e:
        LEV.join_topk(qc, cc, 6, query_indices=[1, 9])
    assert e.value.status == N.RF_ERR_INVALID_ARG
    # ... with the outputs untouched; and m != count with NULL indices
    args = rf.Args().to_c(False)
    idx = np.array([1, 9], dtype=np.uint64)
    for qi_ptr, m in ((idx.ctypes.data, 2), (None, len(qc) - 1), (None, len(qc) + 1)):
        sc, oi, cnt = np.full(60, 77, dtype=np.uint32), np.full(60, 77, dtype=np.uint64), np.full(10, 77, dtype=np.uint32)
        st = N.lib().rf_join_topk_u32(N.LEVENSHTEIN, qc._h, qi_ptr, m, cc._h, N.OP_DISTANCE, C.byref(args), 0, 6, 0, sc.ctypes.data, oi.ctypes.data, cnt.ctypes.data, None)
        assert st == N.RF_ERR_INVALID_ARG
        assert (sc == 77).all() and (oi == 77).all() and (cnt == 77).all()
    # either corpus empty: RF_OK with every count 0
    empty = rf.Corpus.from_list([])
    assert LEV.join_topk(empty, cc, 3)[2].shape == (0,)
    res = LEV.join_topk(qc, empty, 3)
    assert res[2].shape == (9,) and (res[2] == 0).all()
    res = LEV.join_topk(empty, cc, 3, query_indices=[])
    assert res[0].shape == (0, 3)


def test_rows_equal_topk_multi_of_comparators_over_the_same_bytes():
    queries, _, qc, cc, _, _ = lengths()
    for metric, op, k in (("levenshtein", N.OP_DISTANCE, 16), ("indel", N.OP_SIMILARITY, 16), ("lcs_seq", N.OP_DISTANCE, 64)):
        cls = J.GPU[metric].BatchComparator
        rows = list(range(8))  # the fusable rows
        sib = cls.topk_multi([cls(queries[r]) for r in rows], cc, k, op)
        assert T.mismatches(cls.join_topk(qc, cc, k, op, query_indices=rows), sib, k) == []
