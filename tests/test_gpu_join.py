"""rf_join_u32 / BatchComparator.join on the device: the triples of two packed corpora within a cutoff equal the CPU oracle's Somes, query by query
(tests/join_check.py holds the inputs, the oracle wrapper and the child-process checks that read the road from RF_TRACE_PLAN).

  lengths and classes   queries of 0, 1, 5, 32, 33, 64, 64, 64 and 65 symbols against ~300 ragged candidates with planted near-copies; three metrics x two ops x two cutoffs
  batch borders         RF_JOIN_BATCH=8 with 1 .. 17 rows
  several tiles / items one workgroup per CU, more units than workgroups
  self-join             the same handle on both sides, with and without RF_JOIN_UPPER
  contention            200 identical candidates: 40 000 triples onto one counter; capacity 0, 1000 and full
  renaming              corpora with different symbol-frequency ranks, bytes 0x00 and 0xFF, query symbols the scanned corpus never stores
  indices               unordered with repeats, bases beyond 32 bits, an index out of range
  per-query road        osa, a `char` corpus, a loose cutoff: equal to the loop of filter_many; RF_JOIN=0 equal to the default"""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEV = rf.distance.levenshtein.BatchComparator


@functools.lru_cache(maxsize=None)
def lengths():
    queries, cands = J.lengths_case()
    data, offsets = rf.ragged(cands)
    return queries, cands, rf.Corpus.from_list(queries), rf.Corpus.from_list(cands), data, offsets


@functools.lru_cache(maxsize=None)
def lengths_oracle(metric, op, cutoff):
    _, _, _, _, data, offsets = lengths()
    return J.Oracle(metric, op, cutoff, data, offsets)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
@pytest.mark.parametrize("metric", ["levenshtein", "indel", "lcs_seq"])
def test_by_query_output_equals_the_oracle(metric, op, which):
    queries, _, qc, cc, _, _ = lengths()
    cutoff = J.CUTOFFS[(metric, op)][which]
    res = J.GPU[metric].BatchComparator.join(qc, cc, op, score_cutoff=cutoff)
    assert res[0].dtype == np.uint64 and res[1].dtype == np.uint64 and res[2].dtype == np.uint32
    exp = lengths_oracle(metric, op, cutoff).triples(queries)
    assert len(exp) > 0
    assert J.got_triples(res) == exp
    # RF_JOIN_ANY: the same set
    res = J.GPU[metric].BatchComparator.join(qc, cc, op, score_cutoff=cutoff, order=N.JOIN_ANY)
    assert sorted(J.got_triples(res)) == exp


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_the_plan_line_shows_the_long_query_per_query_and_the_rest_fused():
    _child("lengths")


def test_join_off_sends_everything_per_query_with_identical_results():
    _child("off", RF_JOIN="0")


def test_group_and_batch_borders():
    _child("batch", RF_JOIN_BATCH="8")


def test_several_tiles_and_items_per_wavefront():
    _child("multitile", RF_SCAN_BLOCKS_PER_CU="1")


def test_self_join_with_and_without_upper():
    rng = np.random.default_rng(3)
    base = [bytes(rng.integers(97, 101, size=20, dtype=np.uint8)) for _ in range(40)]
    rows = [base[int(i)] for i in rng.integers(0, 40, size=129)]  # duplicates
    for i in range(0, 129, 5):  # and near-duplicates
        rows[i] = J.edits(rng, rows[i], 1)[:20].ljust(20, b"a")
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    ora = J.Oracle("levenshtein", N.OP_DISTANCE, 2, data, offsets)
    full = J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2))
    assert full == ora.triples(rows)
    have = set(full)
    assert all((i, i, 0) in have for i in range(129))
    assert all((j, i, v) in have for i, j, v in full)
    up = J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, upper=True))
    assert up == [t for t in full if t[0] < t[1]] == ora.triples(rows, upper=True)
    assert len(up) > 129 // 2


def test_upper_compares_with_the_row_index_not_the_position_in_q():
    """RF_JOIN_UPPER with rows in any order and repeated: position in Q and row index differ for every entry, so a compare against the position (or a
    wrongly filled row index in the work list) changes the set.  Both roads: fused rows and the 65-symbol row."""
    queries, cands, _, _, _, _ = lengths()
    rows = queries + cands[:120]  # one corpus on both sides; its first nine rows are the queries, whose near-copies sit further down
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    ora = J.Oracle("levenshtein", N.OP_DISTANCE, 3, data, offsets)
    qi = [40, 7, 3, 8, 7, 128, 0, 5, 3, 77, 6, 4]
    assert all(p != r for p, r in enumerate(qi))
    plain = ora.triples(rows, qi)
    exp = ora.triples(rows, qi, upper=True)
    assert 0 < len(exp) < len(plain)
    assert exp != [t for p, r in enumerate(qi) for t in ora.triples(rows, [r]) if t[1] > p]  # (the wrong compare gives another set here)
    assert J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=3, query_indices=qi)) == plain
    assert J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=3, query_indices=qi, upper=True)) == exp
    assert sorted(J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=3, query_indices=qi, upper=True, order=N.JOIN_ANY))) == sorted(exp)


def test_null_indices_need_m_equal_to_the_count():
    _, _, qc, cc, _, _ = lengths()
    args = rf.Args().score_cutoff(3).to_c(False)
    for m in (len(qc) - 1, len(qc) + 1):
        oq, oi, sc, cnt = np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint32), np.full(1, 77, dtype=np.uint64)
        st = N.lib().rf_join_u32(N.LEVENSHTEIN, qc._h, None, m, cc._h, N.OP_DISTANCE, C.byref(args), 0, 0, 0, 8, oq.ctypes.data, oi.ctypes.data, sc.ctypes.data,
                                 cnt.ctypes.data_as(C.POINTER(C.c_uint64)), N.JOIN_BY_QUERY, None)
        assert st == N.RF_ERR_INVALID_ARG
        assert (oq == 77).all() and (oi == 77).all() and (sc == 77).all() and (cnt == 77).all()


def test_contention_and_capacity():
    rows = [b"the same twenty bytes"[:20]] * 200
    corpus = rf.Corpus.from_list(rows)
    everything = {(i, j, 0) for i in range(200) for j in range(200)}
    res = LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=1, capacity=0)
    assert len(res[0]) == 0 and LEV.last_join_count == 40000
    for order in (N.JOIN_BY_QUERY, N.JOIN_ANY):
        res = J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=1, capacity=1000, order=order))
        assert LEV.last_join_count == 40000
        assert len(res) == 1000 and len(set(res)) == 1000 and set(res) <= everything
        if order == N.JOIN_BY_QUERY:
            assert res == sorted(res)
    res = J.got_triples(LEV.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=1))
    assert LEV.last_join_count == 40000 and len(res) == 40000 and set(res) == everything and res == sorted(res)


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
    for metric, cutoff in (("levenshtein", 4), ("indel", 5)):
        exp = J.Oracle(metric, N.OP_DISTANCE, cutoff, data, offsets).triples(queries)
        assert len(exp) >= 24
        assert J.got_triples(J.GPU[metric].BatchComparator.join(qc, cc, N.OP_DISTANCE, score_cutoff=cutoff)) == exp
    # and the other way round: the roles of the two corpora swapped
    data, offsets = rf.ragged(queries)
    exp = J.Oracle("levenshtein", N.OP_DISTANCE, 4, data, offsets).triples(cands)
    assert J.got_triples(LEV.join(cc, qc, N.OP_DISTANCE, score_cutoff=4)) == exp


def test_query_indices_and_bases():
    queries, _, qc, cc, _, _ = lengths()
    ora = lengths_oracle("levenshtein", N.OP_DISTANCE, 3)
    qi = [7, 2, 7, 0, 8, 3, 3, 5]  # unordered, repeats, the 65-symbol row among them
    base = 2**32 + 5
    res = LEV.join(qc, cc, N.OP_DISTANCE, score_cutoff=3, query_indices=qi, query_base=base, index_base=base)
    exp = ora.triples(queries, qi, query_base=base, index_base=base)
    assert J.got_triples(res) == exp and len(exp) > 8
    with pytest.raises(rf.RfError) as e:
        LEV.join(qc, cc, N.OP_DISTANCE, score_cutoff=3, query_indices=[1, 9])
    assert e.value.status == N.RF_ERR_INVALID_ARG
    # ... with the outputs untouched
    args = rf.Args().score_cutoff(3).to_c(False)
    idx = np.array([1, 9], dtype=np.uint64)
    oq, oi, sc, cnt = np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint32), np.full(1, 77, dtype=np.uint64)
    st = N.lib().rf_join_u32(N.LEVENSHTEIN, qc._h, idx.ctypes.data, 2, cc._h, N.OP_DISTANCE, C.byref(args), 0, 0, 0, 8, oq.ctypes.data, oi.ctypes.data, sc.ctypes.data,
                             cnt.ctypes.data_as(C.POINTER(C.c_uint64)), N.JOIN_BY_QUERY, None)
    assert st == N.RF_ERR_INVALID_ARG
    assert (oq == 77).all() and (oi == 77).all() and (sc == 77).all() and (cnt == 77).all()
    # either corpus empty: RF_OK with count 0
    empty = rf.Corpus.from_list([])
    assert len(LEV.join(empty, cc, N.OP_DISTANCE, score_cutoff=3)[0]) == 0 and LEV.last_join_count == 0
    assert len(LEV.join(qc, empty, N.OP_DISTANCE, score_cutoff=3)[0]) == 0 and LEV.last_join_count == 0


def _loop_of_filter_many(cls, queries, corpus, op, cutoff):
    out = []
    for qi, q in enumerate(queries):
        idx, sc = cls(q).filter_many(op, corpus, score_cutoff=cutoff)
        out += [(qi, int(j), int(v)) for j, v in zip(idx.tolist(), sc.tolist())]
    return out


def test_per_query_road_equals_the_loop_of_filter_many():
    queries, cands, qc, cc, _, _ = lengths()
    # osa has no fused kernel
    osa = rf.distance.osa.BatchComparator
    exp = _loop_of_filter_many(osa, queries, cc, N.OP_DISTANCE, 3)
    assert J.got_triples(osa.join(qc, cc, N.OP_DISTANCE, score_cutoff=3)) == exp and len(exp) > 9
    # a loose cutoff: plan() sets no early-out
    exp = _loop_of_filter_many(LEV, queries, cc, N.OP_DISTANCE, 60)
    assert J.got_triples(LEV.join(qc, cc, N.OP_DISTANCE, score_cutoff=60)) == exp and len(exp) > 300
    # a `char` corpus, on either side
    greek = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()]
    rng = np.random.default_rng(4)
    wq = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=ln)) for ln in (0, 3, 20, 40)]
    wc = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=int(ln))) for ln in rng.integers(0, 45, size=150)]
    for k, q in enumerate(wq):
        wc[5 + 9 * k] = q
        wc[6 + 9 * k] = q[1:] + "Ω"
    wqc, wcc = rf.Corpus.from_list(wq), rf.Corpus.from_list(wc)
    exp = _loop_of_filter_many(LEV, wq, wcc, N.OP_DISTANCE, 3)
    assert J.got_triples(LEV.join(wqc, wcc, N.OP_DISTANCE, score_cutoff=3)) == exp and len(exp) >= 8
