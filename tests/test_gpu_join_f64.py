"""rf_join_f64 / BatchComparator.join_f64 on the device: the triples of two packed corpora within an f64 cutoff equal the CPU oracle's Somes, query by query,
every double by its bit pattern (tests/join_f64_check.py holds the oracle wrapper and the child-process checks that read the road from RF_TRACE_PLAN; the
inputs are tests/join_check.py's).

  lengths and classes   queries of 0, 1, 5, 32, 33, 64, 64, 64 and 65 symbols against 307 ragged candidates: three metrics x four cutoffs, the ratio with both
                        ops and both normalizations, weights (2, 2, 2) and (2, 2, 5); the pair (empty query, empty candidate)
  plan line             the eight short rows fused in two groups, the 65-symbol row per query; RF_JOIN=0; a candidate of 65 600 symbols changes nothing
  batch borders         RF_JOIN_BATCH=8 with 1 .. 17 rows
  several tiles / units one workgroup per CU, more units than workgroups
  cutoff = a score      the cutoff at a planted score and one ulp to either side
  self-join             the same handle on both sides, with and without RF_JOIN_UPPER; rows in any order with repeats
  contention            200 identical candidates: 40 000 triples onto one counter; capacity 0, 1000 and full
  renaming              corpora with different symbol-frequency ranks, bytes 0x00 and 0xFF, query symbols the scanned corpus never stores
  bases                 beyond 32 bits, an index out of range, empty corpora
  per-query road        jaro_winkler, osa, a loose cutoff, a `char` corpus: equal to the loop of filter_many"""
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
import join_f64_check as F  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NS = F.ND, F.NS
LEV = rf.distance.levenshtein.BatchComparator


@functools.lru_cache(maxsize=None)
def lengths():
    queries, cands = F.lengths_case()
    data, offsets = rf.ragged(cands)
    return queries, cands, rf.Corpus.from_list(queries), rf.Corpus.from_list(cands), data, offsets


@functools.lru_cache(maxsize=None)
def lengths_oracle(metric, op, cutoff, weights=None):
    _, _, _, _, data, offsets = lengths()
    return F.Oracle(metric, op, cutoff, data, offsets, weights)


@pytest.mark.parametrize("metric,op,cutoff,weights", F.LENGTH_CASES)
def test_by_query_output_equals_the_oracle(metric, op, cutoff, weights):
    queries, cands, qc, cc, _, _ = lengths()
    res = F.join(metric, qc, cc, op, cutoff, weights)
    assert res[0].dtype == np.uint64 and res[1].dtype == np.uint64 and res[2].dtype == np.float64
    exp = lengths_oracle(metric, op, cutoff, weights).triples(queries)
    assert len(exp) > 0
    got = F.got_triples(res)
    assert got == exp
    # (empty query, empty candidate): the maximum is 0
    empties = [j for j, c in enumerate(cands) if len(c) == 0]
    assert len(queries[0]) == 0 and empties
    assert all((0, j, F.empty_pair_score(ND if op == ND else NS)) in got for j in empties)
    # RF_JOIN_ANY: the same set
    res = F.join(metric, qc, cc, op, cutoff, weights, order=N.JOIN_ANY)
    assert sorted(F.got_triples(res)) == exp


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "join_f64_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_the_plan_line_shows_the_long_query_per_query_and_the_rest_fused():
    _child("lengths")


def test_join_off_sends_everything_per_query_with_identical_results():
    _child("off", RF_JOIN="0")


def test_a_candidate_of_65600_symbols_leaves_the_rows_fused():
    _child("long")


def test_group_and_batch_borders():
    _child("batch", RF_JOIN_BATCH="8")


def test_several_tiles_and_units_per_wavefront():
    _child("multitile", RF_SCAN_BLOCKS_PER_CU="1")


def _boundary_rows(length, seed):
    """three query rows of `length` symbols; candidates: each query with 0..5 substitutions ('~', at distinct places) and 40 unrelated rows"""
    rng = np.random.default_rng(seed)
    queries = [bytes(rng.integers(48, 122, size=length, dtype=np.uint8)) for _ in range(3)]
    cands = [bytes(rng.integers(48, 122, size=length, dtype=np.uint8)) for _ in range(40)]
    for q in queries:
        for k in range(6):
            row = bytearray(q)
            for at in rng.choice(length, size=k, replace=False):
                row[int(at)] = 126
            cands.insert(int(rng.integers(0, len(cands) + 1)), bytes(row))
    return queries, cands


# metric, row length, op, the cutoff computed in Python f64: three substitutions are a Levenshtein distance of 3 in 20, an Indel distance of 6 in 128 / in 40
BOUNDARY = [("levenshtein", 20, ND, 3 / 20), ("levenshtein", 20, NS, 1.0 - 3 / 20), ("indel", 64, ND, 6 / 128), ("indel", 64, NS, 1.0 - 6 / 128),
            ("ratio", 20, NS, 1.0 - 6 / 40), ("ratio_indel", 20, NS, 1.0 - 6 / 40)]


@pytest.mark.parametrize("metric,length,op,cutoff", BOUNDARY)
def test_a_cutoff_equal_to_a_score_and_one_ulp_to_either_side(metric, length, op, cutoff):
    queries, cands = _boundary_rows(length, 7 + length)
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    data, offsets = rf.ragged(cands)
    sets = []
    for c in (float(np.nextafter(cutoff, -np.inf)), cutoff, float(np.nextafter(cutoff, np.inf))):
        exp = F.Oracle(metric, op, c, data, offsets).triples(queries)
        assert len(exp) >= 3
        assert F.got_triples(F.join(metric, qc, cc, op, c)) == exp
        sets.append(frozenset((t[0], t[1]) for t in exp))
    assert len(set(sets)) >= 2  # (the planted rows sit exactly on the cutoff: the case tells `<` from `<=`)


def test_self_join_with_and_without_upper():
    rng = np.random.default_rng(3)
    base = [bytes(rng.integers(97, 101, size=20, dtype=np.uint8)) for _ in range(40)]
    rows = [base[int(i)] for i in rng.integers(0, 40, size=129)]  # duplicates
    for i in range(0, 129, 5):  # and near-duplicates
        rows[i] = F.edits(rng, rows[i], 1)[:20].ljust(20, b"a")
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    ora = F.Oracle("levenshtein", NS, 0.9, data, offsets)
    one = F.bits([1.0])[0]
    full = F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9))
    assert full == ora.triples(rows)
    have = set(full)
    assert all((i, i, one) in have for i in range(129))
    assert all((j, i, v) in have for i, j, v in full)
    up = F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, upper=True))
    assert up == [t for t in full if t[0] < t[1]] == ora.triples(rows, upper=True)
    assert len(up) > 129 // 2


def test_upper_compares_with_the_row_index_not_the_position_in_q():
    """RF_JOIN_UPPER with rows in any order and repeated: position in Q and row index differ for every entry, so a compare against the position (or a
    wrongly filled row index in the work list) changes the set.  Both roads: fused rows and the 65-symbol row."""
    queries, cands, _, _, _, _ = lengths()
    rows = queries + cands[:120]  # one corpus on both sides; its first nine rows are the queries, whose near-copies sit further down
    corpus = rf.Corpus.from_list(rows)
    data, offsets = rf.ragged(rows)
    ora = F.Oracle("levenshtein", NS, 0.9, data, offsets)
    qi = [40, 7, 3, 8, 7, 128, 0, 5, 3, 77, 6, 4]
    assert all(p != r for p, r in enumerate(qi))
    plain = ora.triples(rows, qi)
    exp = ora.triples(rows, qi, upper=True)
    assert 0 < len(exp) < len(plain)
    assert exp != [t for p, r in enumerate(qi) for t in ora.triples(rows, [r]) if t[1] > p]  # (the wrong compare gives another set here)
    assert F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, query_indices=qi)) == plain
    assert F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, query_indices=qi, upper=True)) == exp
    assert sorted(F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, query_indices=qi, upper=True, order=N.JOIN_ANY))) == sorted(exp)


def test_contention_and_capacity():
    rows = [b"the same twenty bytes"[:20]] * 200
    corpus = rf.Corpus.from_list(rows)
    one = F.bits([1.0])[0]
    everything = {(i, j, one) for i in range(200) for j in range(200)}
    res = LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, capacity=0)
    assert len(res[0]) == 0 and res[2].dtype == np.float64 and LEV.last_join_count == 40000
    for order in (N.JOIN_BY_QUERY, N.JOIN_ANY):
        res = F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9, capacity=1000, order=order))
        assert LEV.last_join_count == 40000
        assert len(res) == 1000 and len(set(res)) == 1000 and set(res) <= everything
        if order == N.JOIN_BY_QUERY:
            assert res == sorted(res)
    res = F.got_triples(LEV.join_f64(corpus, corpus, NS, score_cutoff=0.9))
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
    # (a near-copy differs from its query in every 0xFF and 'q' -- about a third of the symbols -- so the cutoffs are the widest the planner still calls tight)
    for metric, op, cutoff in (("levenshtein", ND, 0.6), ("indel", NS, 0.65), ("ratio", N.OP_SIMILARITY, 0.65)):
        exp = F.Oracle(metric, op, cutoff, data, offsets).triples(queries)
        assert len(exp) >= 24
        assert any(b"\xff" in queries[t[0]] or b"q" in queries[t[0]] for t in exp)
        assert F.got_triples(F.join(metric, qc, cc, op, cutoff)) == exp
    # and the other way round: the roles of the two corpora swapped
    data, offsets = rf.ragged(queries)
    exp = F.Oracle("levenshtein", ND, 0.6, data, offsets).triples(cands)
    assert len(exp) >= 24
    assert F.got_triples(LEV.join_f64(cc, qc, ND, score_cutoff=0.6)) == exp


def test_query_indices_and_bases():
    queries, _, qc, cc, _, _ = lengths()
    ora = lengths_oracle("levenshtein", NS, 0.9)
    qi = [7, 2, 7, 0, 8, 3, 3, 5]  # unordered, repeats, the 65-symbol row among them
    base = 2**32 + 5
    res = LEV.join_f64(qc, cc, NS, score_cutoff=0.9, query_indices=qi, query_base=base, index_base=base)
    exp = ora.triples(queries, qi, query_base=base, index_base=base)
    assert F.got_triples(res) == exp and len(exp) > 8
    with pytest.raises(rf.RfError) as e:
        LEV.join_f64(qc, cc, NS, score_cutoff=0.9, query_indices=[1, 9])
    assert e.value.status == N.RF_ERR_INVALID_ARG
    # ... with the outputs untouched; so with m != count and no indices
    args = rf.Args().score_cutoff(0.9).to_c(True)
    idx = np.array([1, 9], dtype=np.uint64)
    for indices, m in ((idx.ctypes.data, 2), (None, len(qc) - 1), (None, len(qc) + 1)):
        oq, oi, sc, cnt = np.full(8, 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint64), np.full(8, 77.0, dtype=np.float64), np.full(1, 77, dtype=np.uint64)
        st = N.lib().rf_join_f64(N.LEVENSHTEIN, qc._h, indices, m, cc._h, NS, C.byref(args), 0, 0, 0, 8, oq.ctypes.data, oi.ctypes.data, sc.ctypes.data,
                                 cnt.ctypes.data_as(C.POINTER(C.c_uint64)), N.JOIN_BY_QUERY, None)
        assert st == N.RF_ERR_INVALID_ARG
        assert (oq == 77).all() and (oi == 77).all() and (sc == 77).all() and (cnt == 77).all()
    # either corpus empty: RF_OK with count 0
    empty = rf.Corpus.from_list([])
    assert len(LEV.join_f64(empty, cc, NS, score_cutoff=0.9)[0]) == 0 and LEV.last_join_count == 0
    assert len(LEV.join_f64(qc, empty, NS, score_cutoff=0.9)[0]) == 0 and LEV.last_join_count == 0


def _loop_of_filter_many(cls, queries, corpus, op, cutoff):
    out = []
    for qi, q in enumerate(queries):
        idx, sc = cls(q).filter_many(op, corpus, score_cutoff=cutoff)
        assert sc.dtype == np.float64
        out += [(qi, int(j), v) for j, v in zip(idx.tolist(), F.bits(sc))]
    return out


def test_per_query_road_equals_the_loop_of_filter_many():
    queries, cands, qc, cc, _, _ = lengths()
    # jaro_winkler and osa have no fused kernel
    jw = rf.distance.jaro_winkler.BatchComparator
    exp = _loop_of_filter_many(jw, queries, cc, N.OP_SIMILARITY, 0.9)
    assert F.got_triples(jw.join_f64(qc, cc, N.OP_SIMILARITY, score_cutoff=0.9)) == exp and len(exp) > 9
    osa = rf.distance.osa.BatchComparator
    exp = _loop_of_filter_many(osa, queries, cc, NS, 0.9)
    assert F.got_triples(osa.join_f64(qc, cc, NS, score_cutoff=0.9)) == exp and len(exp) > 9
    # a loose cutoff: the slack of 0.5 is not below 0.4, so plan() sets no early-out
    indel = rf.distance.indel.BatchComparator
    exp = _loop_of_filter_many(indel, queries, cc, NS, 0.5)
    assert F.got_triples(indel.join_f64(qc, cc, NS, score_cutoff=0.5)) == exp and len(exp) > 9
    # a `char` corpus, on either side
    greek = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()]
    rng = np.random.default_rng(4)
    wq = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=ln)) for ln in (0, 3, 20, 40)]
    wc = ["".join(greek[int(i)] for i in rng.integers(0, len(greek), size=int(ln))) for ln in rng.integers(0, 45, size=150)]
    for k, q in enumerate(wq):
        wc[5 + 9 * k] = q
        wc[6 + 9 * k] = q[1:] + "Ω"
    wqc, wcc = rf.Corpus.from_list(wq), rf.Corpus.from_list(wc)
    exp = _loop_of_filter_many(LEV, wq, wcc, NS, 0.6)
    assert F.got_triples(LEV.join_f64(wqc, wcc, NS, score_cutoff=0.6)) == exp and len(exp) >= 6
    latin_q = [b"alpha", b"beta", b""]
    exp = _loop_of_filter_many(LEV, [q.decode() for q in latin_q], wcc, NS, 0.6)
    assert F.got_triples(LEV.join_f64(rf.Corpus.from_list(latin_q), wcc, NS, score_cutoff=0.6)) == exp
    # ... and rows of a `char` corpus against a byte corpus: the rows whose symbols a byte corpus can hold are served, one that holds others is refused as the
    # single-query call refuses it -- an error, not an empty answer
    mixed_q, latin_c = ["alpha", "αβγ", ""], rf.Corpus.from_list([b"alpha", b"alphb", b"", b"beta", b"alpha"])
    mixed_qc = rf.Corpus.from_list(mixed_q)
    assert mixed_qc.wide and not latin_c.wide
    exp = [((0, 2)[qi], j, v) for qi, j, v in _loop_of_filter_many(LEV, ["alpha", ""], latin_c, NS, 0.6)]
    assert F.got_triples(LEV.join_f64(mixed_qc, latin_c, NS, score_cutoff=0.6, query_indices=[0, 2])) == exp and len(exp) == 4
    with pytest.raises(rf.RfError) as e:
        LEV.join_f64(mixed_qc, latin_c, NS, score_cutoff=0.6)
    assert e.value.status == N.RF_ERR_UNSUPPORTED
