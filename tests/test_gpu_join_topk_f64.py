"""rf_join_topk_f64 / BatchComparator.join_topk_f64 on the device: every row's k best candidates by normalized score equal the CPU oracle's float64 rows ranked by
(score, index), bit for bit (tests/join_topk_f64_check.py holds the oracle wrapper and the child-process checks that read the road from RF_TRACE_PLAN).

  lengths and classes   queries of 0, 1, 5, 32, 33, 64, 64, 64 and 65 symbols against 307 ragged candidates, an empty one among them (a maximum of 0);
                        levenshtein / indel / lcs_seq x both normalized ops, fuzz::ratio x both of its ops x with and without the Indel normalization, k in {1, 3, 64}
  equal ratios          2/4 and 4/8 (the query `aaaa` against `aa` and `aaaaaaaa`), in both index orders, tie by index; for indel 8/20 and 16/40.  (The issue
                        asks for "a 5/20 versus 10/40 pair for indel".  No such pair exists: an Indel distance len1 + len2 - 2 lcs has the parity of its maximum
                        len1 + len2, so 5/20 is no Indel score; and with the maximum doubling from 20 to 40 for ONE query, 2 lcs1 = lcs2 <= len1 and
                        lcs1 <= 20 - len1 leave 8/20 = 16/40 at len1 = 12 or 14 as the pairs there are.  The test plants that one and asserts from the oracle
                        alone that the two candidates score the same double.)
  ties                  200 identical candidates on both sides, single-length and length-bucketed, with and without no_self
  no_self               compares with the row index, not the position in Q; both roads
  the 65535 border      a longest candidate of 65471 bytes, then 65472, under indel with rows of 63 and 64 symbols: norm_key_fits is asked per row
  weights               Indel-like weights fuse, a general table goes per query; both equal topk_multi(op = normalized) over the same strings (the `lengths` child)
  cutoffs               loose: fused, with rows short of k; tight: per query; NaN: none (the `lengths` child)
  units and batches     one workgroup per CU with the units forced to many and to 1; RF_JOIN_BATCH=8 with 1 .. 17 rows: identical rows
  per-query road        jaro, jaro_winkler, osa, a `char` corpus on either side: equal to the loop of topk(); RF_JOIN=0 equal to the default; k = 65; k beyond the corpus
  bases and empties     an index base beyond 32 bits, an index out of range, either corpus empty
  the sibling           equal to topk_multi(op = normalized) of comparators built from the same byte strings"""
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
import join_topk_f64_check as F  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NS = F.ND, F.NS
LEV = rf.distance.levenshtein.BatchComparator


@functools.lru_cache(maxsize=None)
def lengths():
    queries, cands = J.lengths_case()
    data, offsets = rf.ragged(cands)
    return queries, cands, rf.Corpus.from_list(queries), rf.Corpus.from_list(cands), data, offsets


@functools.lru_cache(maxsize=None)
def lengths_oracle(metric, op):
    _, _, _, _, data, offsets = lengths()
    return F.F64Oracle(metric, op, None, data, offsets)


@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("metric,op", F.FUSED_OPS)
def test_rows_equal_the_oracle(metric, op, k):
    queries, cands, qc, cc, _, _ = lengths()
    assert b"" in cands
    res = F.join(metric, qc, cc, k, op)
    exp = [lengths_oracle(metric, op).row(q, k) for q in queries]
    assert all(len(es) == k for es, _ in exp)
    assert F.mismatches(res, exp, k) == []


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_topk_f64_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, r.stdout[-4000:] + r.stderr[-3000:]
    return r


def test_the_plan_line_shows_the_roads_under_cutoffs_and_weights():
    _child("lengths")


def test_join_off_sends_everything_per_query_with_identical_results():
    _child("off", RF_JOIN="0")


def test_the_65535_border_is_decided_row_by_row():
    _child("border")


def test_group_and_batch_borders():
    _child("batch", RF_JOIN_BATCH="8")


@pytest.mark.parametrize("shape", ["rows20", "ragged"])
def test_several_tiles_per_wavefront_and_several_units_per_row(shape):
    _child("multitile_" + shape, RF_SCAN_BLOCKS_PER_CU="1", RF_JOIN_TOPK_UNITS=str(256 * T.multitile_groups(shape)))


@pytest.mark.parametrize("shape", ["rows20", "ragged"])
def test_one_unit_per_group_gives_identical_rows(shape):
    _child("multitile_" + shape, RF_SCAN_BLOCKS_PER_CU="1", RF_JOIN_TOPK_UNITS="1")


def test_equal_ratios_from_different_fractions_tie_by_index():
    """`aaaa` against `aa` (2/4) and `aaaaaaaa` (4/8), in both index orders, for every fused family; for indel also 8/20 against 16/40 (the module docstring has
    why not 5/20 against 10/40).  Candidates of different lengths sit in different tiles and have different maxima: only the key's equality makes the index decide."""
    q4, q12 = b"aaaa", b"abcdefghijkl"
    c8, c28 = b"abcdef~~", q12 + b"~" * 16
    cands = [b"aaaaaaaa", b"aa", c28, c8, b"zzzz", b"aa", b"aaaaaaaa", c8, c28, b"aaa", b"", b"abcdefgh"]
    queries = [q4, q12]
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    # from the oracle alone: the planted pairs score the same double
    for metric in ("levenshtein", "lcs_seq", "indel", "ratio", "ratio_indel"):
        idx, sc = F.F64Oracle(metric, NS, None, data, offsets).somes(q4)
        assert len(idx) == len(cands) and sc[0] == sc[1] == sc[5] == sc[6], metric
    idx, sc = F.F64Oracle("indel", ND, None, data, offsets).somes(q12)
    assert sc[2] == sc[3] == sc[7] == sc[8] == 0.4 and 8 / 20 == 16 / 40
    for metric, op in F.FUSED_OPS:
        ora = F.F64Oracle(metric, op, None, data, offsets)
        for k in (3, 5, len(cands)):
            res = F.join(metric, qc, cc, k, op)
            assert F.mismatches(res, [ora.row(q, k) for q in queries], k) == [], (metric, op, k)
    # ... and spelled out once: by normalized Levenshtein similarity `aaaa` ranks `aaa` (0.75) first, then the four candidates at 0.5 in index order
    sc, ix, cnt = LEV.join_topk_f64(qc, cc, 5, NS, query_indices=[0])
    assert cnt.tolist() == [5] and sc[0].tolist() == [0.75, 0.5, 0.5, 0.5, 0.5] and ix[0].tolist() == [9, 0, 1, 5, 6]
    # ... and by Indel distance `abcdefghijkl` ranks `abcdefgh` (4/20) first, then the four at 0.4 in index order: 16/40, 8/20, 8/20, 16/40
    sc, ix, cnt = rf.distance.indel.BatchComparator.join_topk_f64(qc, cc, 5, ND, query_indices=[1])
    assert sc[0].tolist() == [0.2, 0.4, 0.4, 0.4, 0.4] and ix[0].tolist() == [11, 2, 3, 7, 8]


@pytest.mark.parametrize("bucketed", [False, True])
def test_ties_go_to_the_smaller_index(bucketed):
    """200 identical 20-byte candidates -- 3 full tiles and a partial one -- as both sides: every candidate ties at similarity 1.0"""
    rows = [b"the same twenty bytes"[:20]] * 200 + ([b"another"] if bucketed else [])
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    for metric, op, best in (("levenshtein", NS, 1.0), ("ratio", N.OP_SIMILARITY, 1.0), ("indel", ND, 0.0)):
        ora = F.F64Oracle(metric, op, None, data, offsets)
        scores, idx, cnt = F.join(metric, corpus, corpus, 5, op)
        assert (cnt == 5).all() and (scores[:200] == best).all() and (idx[:200] == np.arange(5, dtype=np.uint64)).all()
        assert F.mismatches((scores, idx, cnt), [ora.row(q, 5) for q in rows], 5) == []
        scores, idx, cnt = F.join(metric, corpus, corpus, 5, op, no_self=True)
        for r in range(200):
            assert idx[r].tolist() == [i for i in range(6) if i != r][:5] and (scores[r] == best).all(), r
        assert F.mismatches((scores, idx, cnt), [ora.row(q, 5, skip=r) for r, q in enumerate(rows)], 5) == []


def test_no_self_compares_with_the_row_index_not_the_position_in_q():
    """One corpus on both sides with exact duplicates of some rows, so that self is not the only candidate at similarity 1.0; rows in any order and repeated, no
    position equal to its row index: a compare against the position (or a wrongly filled row index in the work list) changes the rows.  Both roads: fused
    rows and the 65-symbol row."""
    queries, cands, _, _, _, _ = lengths()
    rows = queries + cands[:120] + [queries[3], queries[7], queries[8], cands[40 - 9], queries[0]]  # (duplicates of rows 3, 7, 8, 40 and 0)
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    qi = [40, 7, 3, 8, 7, 128, 0, 5, 3, 77, 6, 4]
    assert all(p != r for p, r in enumerate(qi))
    for k in (1, 4):
        for metric, op in (("levenshtein", NS), ("levenshtein", ND), ("ratio", N.OP_SIMILARITY)):
            ora = F.F64Oracle(metric, op, None, data, offsets)
            plain = [ora.row(rows[r], k) for r in qi]
            exp = [ora.row(rows[r], k, skip=r) for r in qi]
            wrong = [ora.row(rows[r], k, skip=p) for p, r in enumerate(qi)]
            differ = lambda a, b: any(x[1].tolist() != y[1].tolist() for x, y in zip(a, b))  # noqa: E731
            assert differ(exp, plain) and differ(exp, wrong)
            assert F.mismatches(F.join(metric, corpus, corpus, k, op, query_indices=qi), plain, k) == []
            assert F.mismatches(F.join(metric, corpus, corpus, k, op, query_indices=qi, no_self=True), exp, k) == []
    # a row with a duplicate still finds a record at similarity 1.0, and never itself
    res = LEV.join_topk_f64(corpus, corpus, 1, NS, query_indices=[3, 8, 129, 131], no_self=True)
    assert (res[0][:, 0] == 1.0).all() and all(int(i) != r for i, r in zip(res[1][:, 0], [3, 8, 129, 131]))


def _loop_of_topk(cls, queries, corpus, k, op, **kw):
    return [cls(q).topk(corpus, k, op, **kw) for q in queries]


def test_per_query_road_equals_the_loop_of_topk():
    queries, cands, qc, cc, _, _ = lengths()
    # jaro / jaro_winkler (every op) and osa (the normalized ops) have no fused kernel
    jaro, jw, osa = F.GPU["jaro"], F.GPU["jaro_winkler"], F.GPU["osa"]
    for cls, k, op in ((jaro, 4, N.OP_SIMILARITY), (jaro, 3, ND), (jw, 4, NS), (jw, 70, N.OP_DISTANCE), (osa, 4, ND), (osa, 70, NS)):
        assert F.mismatches(cls.join_topk_f64(qc, cc, k, op), _loop_of_topk(cls, queries, cc, k, op), k) == [], (cls, k, op)
    # the float classes' default op is the similarity, the usize metrics' the normalized similarity
    assert F.mismatches(jaro.join_topk_f64(qc, cc, 2), _loop_of_topk(jaro, queries, cc, 2, N.OP_SIMILARITY), 2) == []
    assert F.mismatches(LEV.join_topk_f64(qc, cc, 2), _loop_of_topk(LEV, queries, cc, 2, NS), 2) == []
    # a `char` corpus, on either side
    greek = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()]
    rng = np.random.default_rng(4)
    wq = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=ln)) for ln in (0, 3, 20, 40)]
    wc = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=int(ln))) for ln in rng.integers(0, 45, size=150)]
    for j, q in enumerate(wq):
        wc[5 + 9 * j] = q
        wc[6 + 9 * j] = q[1:] + "Ω"
    wqc, wcc = rf.Corpus.from_list(wq), rf.Corpus.from_list(wc)
    res = LEV.join_topk_f64(wqc, wcc, 4, NS)
    assert F.mismatches(res, _loop_of_topk(LEV, wq, wcc, 4, NS), 4) == []
    assert res[1][1:, 0].tolist() == [5 + 9 * j for j in range(1, 4)] and (res[0][1:, 0] == 1.0).all()
    # (a `char` corpus on one side only: byte rows against the `char` corpus)
    latin = [b"abc", b"", b"hello world"]
    assert F.mismatches(LEV.join_topk_f64(rf.Corpus.from_list(latin), wcc, 3, ND), _loop_of_topk(LEV, latin, wcc, 3, ND), 3) == []
    # ... and with no_self on a `char` corpus joined with itself: the per-query road drops the row's own entry
    res = LEV.join_topk_f64(wcc, wcc, 3, NS, no_self=True, query_indices=[5 + 9 * 2, 6 + 9 * 2, 0])
    exp = []
    for r in (5 + 9 * 2, 6 + 9 * 2, 0):
        sc, ix = LEV(wc[r]).topk(wcc, 4, NS)
        keep = ix != r
        exp.append((sc[keep][:3], ix[keep][:3]))
    assert F.mismatches(res, exp, 3) == []


def test_k_beyond_the_corpus_and_beyond_the_lists():
    queries, cands, qc, cc, data, offsets = lengths()
    small = cands[:40]
    sdata, soffsets = rf.ragged(small)
    res = LEV.join_topk_f64(qc, rf.Corpus.from_list(small), 64, NS)
    assert (res[2] == 40).all()
    ora = F.F64Oracle("levenshtein", NS, None, sdata, soffsets)
    assert F.mismatches(res, [ora.row(q, 64) for q in queries], 64) == []
    # k = 65: the lists hold 64, every row goes per query
    res = F.join("ratio", qc, cc, 65, N.OP_SIMILARITY)
    assert F.mismatches(res, [lengths_oracle("ratio", N.OP_SIMILARITY).row(q, 65) for q in queries], 65) == []


def test_index_base_indices_out_of_range_and_empties():
    queries, _, qc, cc, _, _ = lengths()
    ora = lengths_oracle("levenshtein", NS)
    qi = [7, 2, 7, 0, 8, 3, 3, 5]  # unordered, repeats, the 65-symbol row among them
    base = 2**32 + 5
    res = LEV.join_topk_f64(qc, cc, 6, NS, query_indices=qi, index_base=base)
    assert F.mismatches(res, [ora.row(queries[r], 6) for r in qi], 6, index_base=base) == []
    assert int(res[1].min()) >= base
    with pytest.raises(rf.RfError) as e:
        LEV.join_topk_f64(qc, cc, 6, NS, query_indices=[1, 9])
    assert e.value.status == N.RF_ERR_INVALID_ARG
    # ... with the outputs untouched; and m != count with NULL indices
    args = rf.Args().to_c(True)
    idx = np.array([1, 9], dtype=np.uint64)
    for qi_ptr, m in ((idx.ctypes.data, 2), (None, len(qc) - 1), (None, len(qc) + 1)):
        sc, oi, cnt = np.full(60, 77.0, dtype=np.float64), np.full(60, 77, dtype=np.uint64), np.full(10, 77, dtype=np.uint32)
        st = N.lib().rf_join_topk_f64(N.LEVENSHTEIN, qc._h, qi_ptr, m, cc._h, NS, C.byref(args), 0, 6, 0, sc.ctypes.data, oi.ctypes.data, cnt.ctypes.data, None)
        assert st == N.RF_ERR_INVALID_ARG
        assert (sc == 77).all() and (oi == 77).all() and (cnt == 77).all()
    # either corpus empty: RF_OK with every count 0
    empty = rf.Corpus.from_list([])
    assert LEV.join_topk_f64(empty, cc, 3)[2].shape == (0,)
    res = LEV.join_topk_f64(qc, empty, 3)
    assert res[2].shape == (9,) and (res[2] == 0).all() and res[0].dtype == np.float64
    res = LEV.join_topk_f64(empty, cc, 3, query_indices=[])
    assert res[0].shape == (0, 3)


def test_rows_equal_topk_multi_of_comparators_over_the_same_bytes():
    queries, _, qc, cc, _, _ = lengths()
    for metric, op, k in (("levenshtein", ND, 16), ("indel", NS, 16), ("lcs_seq", ND, 64), ("ratio", N.OP_SIMILARITY, 16), ("ratio_indel", NS, 16)):
        cls = F.GPU[metric]
        rows = list(range(8))  # the fusable rows
        sib = cls.topk_multi([cls(queries[r]) for r in rows], cc, k, op, args=F.call_args(metric))
        assert F.mismatches(F.join(metric, qc, cc, k, op, query_indices=rows), sib, k) == []
